"""bin/sw_spectra with the key rayleigh=FILE as a user would run it: the two-stream fluxes of its output file per wavenumber
and per g point against tests/rayleigh_ref.py (two_stream_closed on the merged column), the variables, long names and the
attribute the key adds, rayleigh_optical_depth against the oracle's transmission average, the host mirror
pipeline.sw_spectra(rayleigh=...) bit for bit, the unchanged output without the key, and the exit codes.

The files hold FLOAT, and the device follows the restatement to 1e-9 of the incoming flux (test_lbl_fluxes_sw_rayleigh_gpu.py:5):
a value may differ from the reference by 2^-23 of itself plus 1e-9 mu0 ssi (per g point: mu0 times the g point's ssi)."""
import numpy as np
import pytest
from scipy.io import netcdf_file

import rayleigh_ref as rr
from test_cli_sw_spectra_gpu import ALBEDO, F32, MU0, NAMES, NCOL, NG, NLAY, NWAV, _args, _make_files, _merged, _nc, run_tool

pytestmark = pytest.mark.gpu

NEW = ("flux_dn_sw", "spectral_flux_dn_sw")


def _spectrum_file(path, p, wn, od):
    """a spectrum file like a gas file's: od (ncol, nlay, nwav) FLOAT"""
    ncol, nlay, nwav = od.shape
    w = netcdf_file(str(path), "w", version=2)
    for name, n in (("column", ncol), ("half_level", nlay + 1), ("level", nlay), ("wavenumber", nwav)):
        w.createDimension(name, n)
    w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p[:nlay + 1], (ncol, 1))
    w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn[:nwav]
    w.createVariable("optical_depth", "f", ("column", "level", "wavenumber"))[:] = od
    w.constituent_id = "rayleigh"
    w.close()


def _make_rayleigh(d, p, wn):
    """Rayleigh optical depth ~ wavenumber^4, shared among the layers by their pressure thickness, a little more per column;
    besides the good file one with fewer wavenumbers and one with fewer levels -> od (NCOL, NLAY, NWAV) as the file holds it"""
    col = 0.4 * (wn / 25000.0) ** 4
    od0 = np.diff(p)[:, None] / p[-1] * col[None, :]
    od = np.stack([(od0 * (1.0 + 0.1 * c)).astype(np.float32) for c in range(NCOL)])
    _spectrum_file(d / "rayleigh.nc", p, wn, od)
    _spectrum_file(d / "rayleigh_short.nc", p, wn, od[:, :, :-7])
    _spectrum_file(d / "rayleigh_levels.nc", p, wn, od[:, :-1, :])
    return od


def _reference_column(ssi, od, ray):
    """(direct, dn, up), each (nsza, nlay+1, nwav), of the merged column in float64"""
    out = [rr.two_stream_closed(od, ray, mu, ALBEDO, ssi) for mu in MU0]
    d, diffuse, up = (np.stack([o[i] for o in out]) for i in range(3))
    return d, d + diffuse, up


def _close(got, ref, scale):
    """FLOAT in the file, 1e-9 of the incoming flux `scale` between the device and the restatement"""
    return np.all(np.abs(got.astype(np.float64) - ref) <= F32 * np.abs(ref) + 1e-9 * scale)


def test_sw_spectra_rayleigh_per_wavenumber(ctx, tmp_path):
    p, t, wn, ssi, g_point, ods = _make_files(tmp_path)
    ray = _make_rayleigh(tmp_path, p, wn)
    out = tmp_path / "spectra.nc"
    r = run_tool("sw_spectra", *_args(tmp_path), "rayleigh=rayleigh.nc", f"output={out}")
    assert r.returncode == 0, r.stderr
    f = _nc(out)
    assert f.rayleigh_scattering == b"two-stream"
    assert set(f.variables) == set(NAMES) | set(NEW) | {"wavenumber", "mu0"}
    assert f.variables["flux_dn_sw"].dimensions == ("column", "mu0", "half_level")
    assert f.variables["spectral_flux_dn_sw"].dimensions == ("column", "mu0", "half_level", "wavenumber")
    assert f.variables["flux_dn_sw"].long_name == b"Downwelling shortwave flux" and f.variables["flux_dn_sw"].units == b"W m-2"
    assert f.variables["spectral_flux_dn_sw"].long_name == b"Downwelling shortwave spectral flux"
    merged = _merged(ods)
    mu = np.array(MU0)
    for c in range(NCOL):
        d, dn, up = _reference_column(ssi, merged[c], ray[c].astype(np.float64))
        point, whole = mu[:, None, None] * ssi[None, None, :], mu[:, None] * ssi.sum()
        assert _close(f.variables["spectral_flux_dn_direct_sw"][c], d, point)
        assert _close(f.variables["spectral_flux_dn_sw"][c], dn, point)
        assert _close(f.variables["spectral_flux_up_sw"][c], up, point)
        assert _close(f.variables["flux_dn_direct_sw"][c], d.sum(2), whole)
        assert _close(f.variables["flux_dn_sw"][c], dn.sum(2), whole)
        assert _close(f.variables["flux_up_sw"][c], up.sum(2), whole)
        assert np.all(f.variables["spectral_flux_dn_sw"][c] >= f.variables["spectral_flux_dn_direct_sw"][c])
        assert np.array_equal(f.variables["optical_depth"][c], merged[c].astype(np.float32))
    assert np.any(f.variables["spectral_flux_dn_sw"][:] > f.variables["spectral_flux_dn_direct_sw"][:])   # it does scatter
    # the host mirror's file and arrays, bit for bit
    from ecckd_amd import pipeline
    m = pipeline.sw_spectra(ctx, [tmp_path / "h2o.nc", tmp_path / "co2.nc"], ssi, tmp_path / "mirror.nc", scaling=[1.0, 2.5],
                            cos_sza=MU0, rayleigh=tmp_path / "rayleigh.nc")
    g = _nc(tmp_path / "mirror.nc")
    assert set(g.variables) == set(f.variables) and g.dimensions == f.dimensions and g.rayleigh_scattering == f.rayleigh_scattering
    for name in NAMES + NEW + ("wavenumber", "mu0"):
        assert np.array_equal(g.variables[name][:], f.variables[name][:]), name
        assert g.variables[name].dimensions == f.variables[name].dimensions
        assert g.variables[name].data.dtype == f.variables[name].data.dtype
        assert g.variables[name]._attributes == f.variables[name]._attributes, name
    for name in NAMES + NEW:
        assert np.array_equal(m[name].astype(np.float32), f.variables[name][:]), name


def test_sw_spectra_rayleigh_per_g_point(ctx, oracle, tmp_path):
    p, t, wn, ssi, g_point, ods = _make_files(tmp_path)
    ray = _make_rayleigh(tmp_path, p, wn)
    out = tmp_path / "gspectra.nc"
    r = run_tool("sw_spectra", *_args(tmp_path), "gpoints=gpoints.nc", "rayleigh=rayleigh.nc", f"output={out}")
    assert r.returncode == 0, r.stderr
    f = _nc(out)
    assert f.rayleigh_scattering == b"two-stream"
    assert set(f.variables) == set(NAMES) | set(NEW) | {"rayleigh_optical_depth", "solar_irradiance", "mu0"}
    assert f.variables["spectral_flux_dn_sw"].dimensions == ("column", "mu0", "half_level", "g_point")
    assert f.variables["rayleigh_optical_depth"].dimensions == ("column", "level", "g_point")
    # names and long names of the ckdmip_sw --ckd --rayleigh-scattering output
    assert f.variables["flux_dn_sw"].long_name == b"Downwelling shortwave flux"
    assert f.variables["spectral_flux_dn_sw"].long_name == b"Downwelling shortwave flux per g point"
    assert f.variables["spectral_flux_up_sw"].long_name == b"Upwelling shortwave flux per g point"
    assert f.variables["spectral_flux_dn_direct_sw"].long_name == b"Downwelling direct shortwave flux per g point"
    assert f.variables["rayleigh_optical_depth"].long_name == b"Layer optical depth due to Rayleigh scattering"
    per_g = lambda x: np.stack([x[:, :, g_point == g].sum(2) for g in range(NG)], axis=2)
    ssi_g = np.array([ssi[g_point == g].sum() for g in range(NG)])
    merged = _merged(ods)
    mu = np.array(MU0)
    for c in range(NCOL):
        d, dn, up = _reference_column(ssi, merged[c], ray[c].astype(np.float64))
        column, whole = mu[:, None, None] * ssi_g[None, None, :], mu[:, None] * ssi.sum()
        assert _close(f.variables["spectral_flux_dn_direct_sw"][c], per_g(d), column)
        assert _close(f.variables["spectral_flux_dn_sw"][c], per_g(dn), column)
        assert _close(f.variables["spectral_flux_up_sw"][c], per_g(up), column)
        assert _close(f.variables["flux_dn_direct_sw"][c], d.sum(2), whole)                         # every wavenumber, -1 included
        assert _close(f.variables["flux_dn_sw"][c], dn.sum(2), whole)
        assert _close(f.variables["flux_up_sw"][c], up.sum(2), whole)
        assert np.all(f.variables["flux_dn_sw"][c] >= f.variables["flux_dn_direct_sw"][c])
        assert np.all(f.variables["spectral_flux_dn_sw"][c] >= f.variables["spectral_flux_dn_direct_sw"][c])
        weight = np.tile(ssi, (NLAY, 1))
        oray, _, _, _ = oracle.average_optical_depth_to_g_point(NG, 0.0, p, g_point, ray[c].astype(np.float64), weight, "transmission")
        assert np.allclose(f.variables["rayleigh_optical_depth"][c], oray, rtol=F32, atol=1e-45)
        oabs, _, _, _ = oracle.average_optical_depth_to_g_point(NG, 0.0, p, g_point, merged[c], weight, "transmission")
        assert np.allclose(f.variables["optical_depth"][c], oabs, rtol=F32, atol=1e-45)                # the absorbers alone
    from ecckd_amd import pipeline
    m = pipeline.sw_spectra(ctx, [tmp_path / "h2o.nc", tmp_path / "co2.nc"], ssi, tmp_path / "gmirror.nc", scaling=[1.0, 2.5],
                            g_point=g_point, cos_sza=MU0, rayleigh=tmp_path / "rayleigh.nc")
    g = _nc(tmp_path / "gmirror.nc")
    assert set(g.variables) == set(f.variables) and g.dimensions == f.dimensions and g.rayleigh_scattering == f.rayleigh_scattering
    for name in NAMES + NEW + ("rayleigh_optical_depth", "solar_irradiance", "mu0"):
        assert np.array_equal(g.variables[name][:], f.variables[name][:]), name
        assert g.variables[name].dimensions == f.variables[name].dimensions
        assert g.variables[name]._attributes == f.variables[name]._attributes, name
    for name in NAMES + NEW + ("rayleigh_optical_depth", "solar_irradiance"):
        assert np.array_equal(np.asarray(m[name]).astype(np.float32), f.variables[name][:]), name


def test_without_the_key_the_output_is_todays(tmp_path):
    """The variable set of today and no attribute; the key adds exactly its variables and leaves what does not scatter alone."""
    p, t, wn, ssi, g_point, ods = _make_files(tmp_path)
    _make_rayleigh(tmp_path, p, wn)
    for extra, names, added in (((), {"wavenumber", "mu0"}, set(NEW)),
                                (("gpoints=gpoints.nc",), {"solar_irradiance", "mu0"}, set(NEW) | {"rayleigh_optical_depth"})):
        plain, scat = tmp_path / "plain.nc", tmp_path / "scattered.nc"
        r = run_tool("sw_spectra", *_args(tmp_path), *extra, "iprofile=0", f"output={plain}")
        assert r.returncode == 0, r.stderr
        r = run_tool("sw_spectra", *_args(tmp_path), *extra, "iprofile=0", "rayleigh=rayleigh.nc", f"output={scat}")
        assert r.returncode == 0, r.stderr
        f, g = _nc(plain), _nc(scat)
        assert set(f.variables) == set(NAMES) | names and not hasattr(f, "rayleigh_scattering")
        assert set(g.variables) == set(f.variables) | added and g.dimensions == f.dimensions
        for name in ("pressure_hl", "temperature_hl", "vmr_fl", "optical_depth") + tuple(names):
            assert np.array_equal(g.variables[name][:], f.variables[name][:]), name


def test_exit_codes(tmp_path):
    p, t, wn, ssi, g_point, ods = _make_files(tmp_path)
    _make_rayleigh(tmp_path, p, wn)
    args = _args(tmp_path)
    out = f"output={tmp_path / 'x.nc'}"
    assert run_tool("sw_spectra", *args, "rayleigh=rayleigh.nc", "iprofile=0", out).returncode == 0
    assert run_tool("sw_spectra", *args, "rayleigh=rayleigh_short.nc", out).returncode == 147      # another wavenumber count
    assert run_tool("sw_spectra", *args, "rayleigh=rayleigh_levels.nc", out).returncode == 147     # another level count
    lw = (f"append_path={tmp_path}", "input=h2o.nc co2.nc", "scaling=1.0 2.5")
    assert run_tool("lw_spectra", *lw, "rayleigh=rayleigh.nc", out).returncode == 147
