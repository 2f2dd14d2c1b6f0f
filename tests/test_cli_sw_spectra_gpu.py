"""bin/sw_spectra as a user would run it (`exe [key=value ...] [file.cfg]` on NetCDF files): variables, dimensions, attributes
and values of its output file per wavenumber and per g point for three solar zenith angles, against the oracle's
radiative_transfer_norayleigh_sw on the merged optical depths; iprofile, a NetCDF-4 output, exit codes.  The tool's file is
also compared with the file of the host mirror pipeline.sw_spectra, which makes the same library calls in the same order."""
import os
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

from ecckd_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
NCOL, NLAY, NWAV, NG = 3, 12, 3001, 6
MU0 = (0.3, 0.5, 0.8)
ALBEDO = 0.15
F32 = 2.0 ** -23        # FLOAT precision: the files hold FLOAT (half an ulp of rounding, 1e-11 of the device against the oracle)
NAMES = ("pressure_hl", "temperature_hl", "vmr_fl", "flux_dn_direct_sw", "flux_up_sw", "optical_depth",
         "spectral_flux_dn_direct_sw", "spectral_flux_up_sw")


def run_tool(name, *args, cwd=None):
    exe = os.path.join(BIN, name)
    if not os.path.exists(exe):                      # a fresh checkout: build the library and the tools first
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    assert os.path.exists(exe), f"{exe} not built (python -c 'import __graft_entry__ as g; g.build()')"
    return subprocess.run([exe, *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=600)


def _nc(path):
    return netcdf_file(str(path), "r", mmap=False)


def _make_files(d):
    """Two gas files of NCOL columns, an ssi file and a g-point file; -> pressure_hl, temperature_hl[c], wavenumber, ssi,
    g_point, {gas: od[c]}"""
    p = syn.pressure_grid(NLAY)
    t0 = syn.temperature_profile(p)
    t = np.stack([t0 + 3.0 * c for c in range(NCOL)])
    wn, dwn = syn.wavenumber_grid(NWAV, 250.0, 50000.0)
    ods = {}
    for g, (seed, scale, vmr) in {"h2o": (41, 3.0, 5e-3), "co2": (43, 0.8, 4e-4)}.items():
        od0 = syn.optical_depth(np, p, wn, syn.SEED_BASE + seed, nlines=40, column_scale=scale, dtype="float32", lo=250.0, hi=50000.0)
        od = np.stack([(od0 * np.float32(1.0 + 0.25 * c)).astype(np.float32) for c in range(NCOL)])
        w = netcdf_file(str(d / f"{g}.nc"), "w", version=2)
        for name, n in (("column", NCOL), ("half_level", NLAY + 1), ("level", NLAY), ("wavenumber", NWAV)):
            w.createDimension(name, n)
        w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p, (NCOL, 1))
        w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = t
        w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
        w.createVariable("mole_fraction_fl", "d", ("column", "level"))[:] = np.full((NCOL, NLAY), vmr)
        w.createVariable("optical_depth", "f", ("column", "level", "wavenumber"))[:] = od
        w.createVariable("reference_surface_mole_fraction", "d", ())[...] = vmr
        w.constituent_id = g
        w.close()
        ods[g] = od
    ssi = syn.solar_spectral_irradiance(wn, dwn)
    w = netcdf_file(str(d / "ssi.nc"), "w", version=2)
    w.createDimension("wavenumber", NWAV)
    w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
    w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = ssi
    w.close()
    rng = np.random.default_rng(5)
    g_point = rng.integers(0, NG, size=NWAV).astype(np.int32)
    g_point[rng.random(NWAV) < 0.05] = -1
    for name, gp in (("gpoints.nc", g_point), ("gpoints_short.nc", g_point[:-7])):
        w = netcdf_file(str(d / name), "w", version=2)
        w.createDimension("wavenumber", gp.size)
        w.createVariable("g_point", "i", ("wavenumber",))[:] = gp
        w.close()
    return p, t, wn, ssi, g_point, ods


def _merged(ods):
    """float64 sum of the two gases, co2 scaled by 2.5 (the `scaling` key)"""
    return ods["h2o"].astype(np.float64) + 2.5 * ods["co2"].astype(np.float64)


def _oracle_column(oracle, ssi, od):
    """(nsza, nlay+1, nwav) down and up"""
    f = [oracle.radiative_transfer_norayleigh_sw(mu, ssi, od, np.full(NWAV, ALBEDO)) for mu in MU0]
    return np.stack([a for a, _ in f]), np.stack([b for _, b in f])


def _args(d):
    return (f"append_path={d}", "input=h2o.nc co2.nc", "scaling=1.0 2.5", "ssi=ssi.nc", "cos_solar_zenith_angle=0.3 0.5 0.8")


def test_sw_spectra_per_wavenumber(ctx, oracle, tmp_path):
    from ecckd_amd import ncio
    p, t, wn, ssi, g_point, ods = _make_files(tmp_path)
    out = tmp_path / "spectra.nc"
    args = _args(tmp_path)
    r = run_tool("sw_spectra", *args, f"output={out}")
    assert r.returncode == 0, r.stderr
    f = _nc(out)
    assert f.dimensions["column"] is None and f.dimensions["wavenumber"] == NWAV and f.dimensions["mu0"] == 3
    assert f.dimensions["gas"] == 2 and "g_point" not in f.dimensions and "solar_irradiance" not in f.variables
    assert int.from_bytes(out.read_bytes()[4:8], "big") == NCOL    # numrecs
    assert f.variables["spectral_flux_dn_direct_sw"].dimensions == ("column", "mu0", "half_level", "wavenumber")
    assert f.variables["spectral_flux_up_sw"].dimensions == ("column", "mu0", "half_level", "wavenumber")
    assert f.variables["flux_dn_direct_sw"].dimensions == ("column", "mu0", "half_level")
    assert f.variables["optical_depth"].dimensions == ("column", "level", "wavenumber")
    assert f.variables["flux_dn_direct_sw"].long_name == b"Downwelling direct shortwave flux"
    assert f.variables["flux_up_sw"].long_name == b"Upwelling shortwave flux" and f.variables["flux_up_sw"].units == b"W m-2"
    assert f.variables["mu0"].long_name == b"Cosine of solar zenith angle"
    assert f.molecules == b"h2o co2" and b"sw_spectra" in f.history and b"ssi" in f.config
    assert f.variables["wavenumber"].data.dtype == np.dtype(">f8") and f.variables["flux_up_sw"].data.dtype == np.dtype(">f4")
    assert np.array_equal(f.variables["mu0"][:], np.array(MU0, dtype=np.float32))
    assert np.array_equal(f.variables["wavenumber"][:], wn)
    merged = _merged(ods)
    for c in range(NCOL):
        fdn, fup = _oracle_column(oracle, ssi, merged[c])
        assert np.allclose(f.variables["flux_dn_direct_sw"][c], fdn.sum(2), rtol=F32, atol=0.0)
        assert np.allclose(f.variables["flux_up_sw"][c], fup.sum(2), rtol=F32, atol=0.0)
        assert np.allclose(f.variables["spectral_flux_dn_direct_sw"][c], fdn, rtol=F32, atol=1e-45)
        assert np.allclose(f.variables["spectral_flux_up_sw"][c], fup, rtol=F32, atol=1e-45)
        assert np.array_equal(f.variables["optical_depth"][c], merged[c].astype(np.float32))
        assert np.array_equal(f.variables["temperature_hl"][c], t[c].astype(np.float32))
    # iprofile = 1: exactly one record, equal to record 1 of the full run
    one = tmp_path / "one.nc"
    r = run_tool("sw_spectra", *args, "iprofile=1", f"output={one}")
    assert r.returncode == 0, r.stderr
    h = _nc(one)
    assert h.variables["flux_up_sw"].shape[0] == 1
    for name in NAMES:
        assert np.array_equal(h.variables[name][0], f.variables[name][1]), name
    # a *.h5 output (NetCDF-4) reads back equal to the classic one through the repository's readers
    h5 = tmp_path / "spectra.h5"
    r = run_tool("sw_spectra", *args, f"output={h5}")
    assert r.returncode == 0, r.stderr
    assert h5.read_bytes()[:8] == b"\x89HDF\r\n\x1a\n"
    with ncio.NcFile(h5) as a, ncio.NcFile(out) as b:
        assert a.dim("column") == NCOL and a.dim("wavenumber") == NWAV and a.dim("mu0") == 3
        for name in NAMES + ("wavenumber", "mu0"):
            assert a.var_info(name) == b.var_info(name), name
            assert np.array_equal(a.read(name), b.read(name)), name
        assert a.att_text("long_name", "flux_up_sw") == "Upwelling shortwave flux" and a.att_text("molecules") == "h2o co2"
    # the host mirror's file, bit for bit (the file holds the FLOAT casts of its arrays)
    from ecckd_amd import pipeline
    m = pipeline.sw_spectra(ctx, [tmp_path / "h2o.nc", tmp_path / "co2.nc"], ssi, tmp_path / "mirror.nc", scaling=[1.0, 2.5],
                            cos_sza=MU0)
    g = _nc(tmp_path / "mirror.nc")
    assert set(g.variables) == set(f.variables) and g.dimensions == f.dimensions
    for name in NAMES + ("wavenumber", "mu0"):
        assert np.array_equal(g.variables[name][:], f.variables[name][:]), name
        assert g.variables[name].dimensions == f.variables[name].dimensions
        assert g.variables[name].data.dtype == f.variables[name].data.dtype
        assert g.variables[name]._attributes == f.variables[name]._attributes, name
    for name in NAMES:
        assert np.array_equal(m[name].astype(np.float32), f.variables[name][:]), name
    assert g.molecules == f.molecules
    # the default angle is 0.5
    r = run_tool("sw_spectra", f"append_path={tmp_path}", "input=h2o.nc co2.nc", "scaling=1.0 2.5", "ssi=ssi.nc", "iprofile=0",
                 f"output={tmp_path / 'default.nc'}")
    assert r.returncode == 0, r.stderr
    d = _nc(tmp_path / "default.nc")
    assert np.array_equal(d.variables["mu0"][:], np.float32([0.5]))
    assert np.array_equal(d.variables["spectral_flux_up_sw"][0, 0], f.variables["spectral_flux_up_sw"][0, 1])


def test_sw_spectra_per_g_point(ctx, oracle, tmp_path):
    p, t, wn, ssi, g_point, ods = _make_files(tmp_path)
    out = tmp_path / "gspectra.nc"
    args = _args(tmp_path)
    r = run_tool("sw_spectra", *args, "gpoints=gpoints.nc", f"output={out}")
    assert r.returncode == 0, r.stderr
    f = _nc(out)
    assert f.dimensions["g_point"] == NG and f.dimensions["column"] is None and f.dimensions["mu0"] == 3
    assert "wavenumber" not in f.variables and "wavenumber" not in f.dimensions
    assert f.variables["spectral_flux_up_sw"].dimensions == ("column", "mu0", "half_level", "g_point")
    assert f.variables["spectral_flux_up_sw"].long_name == b"Upwelling shortwave flux per g point"
    assert f.variables["spectral_flux_dn_direct_sw"].long_name == b"Downwelling direct shortwave flux per g point"
    assert f.variables["solar_irradiance"].long_name == b"Solar irradiance across each g point"
    ssi_g = np.array([ssi[g_point == g].sum() for g in range(NG)])
    assert np.allclose(f.variables["solar_irradiance"][:], ssi_g, rtol=F32, atol=0.0)
    merged = _merged(ods)
    for c in range(NCOL):
        fdn, fup = _oracle_column(oracle, ssi, merged[c])
        gdn = np.stack([fdn[:, :, g_point == g].sum(2) for g in range(NG)], axis=2)
        gup = np.stack([fup[:, :, g_point == g].sum(2) for g in range(NG)], axis=2)
        assert np.allclose(f.variables["spectral_flux_dn_direct_sw"][c], gdn, rtol=F32, atol=0.0)
        assert np.allclose(f.variables["spectral_flux_up_sw"][c], gup, rtol=F32, atol=0.0)
        assert np.allclose(f.variables["flux_dn_direct_sw"][c], fdn.sum(2), rtol=F32, atol=0.0)      # every wavenumber, -1 included
        assert np.allclose(f.variables["flux_up_sw"][c], fup.sum(2), rtol=F32, atol=0.0)
        oma, _, _, ne = oracle.average_optical_depth_to_g_point(NG, 0.0, p, g_point, merged[c], np.tile(ssi, (NLAY, 1)), "transmission")
        assert np.allclose(f.variables["optical_depth"][c], oma, rtol=F32, atol=1e-45)
    # the tool's file and the host mirror's file and arrays: bit for bit
    from ecckd_amd import pipeline
    m = pipeline.sw_spectra(ctx, [tmp_path / "h2o.nc", tmp_path / "co2.nc"], ssi, tmp_path / "gmirror.nc", scaling=[1.0, 2.5],
                            g_point=g_point, cos_sza=MU0)
    g = _nc(tmp_path / "gmirror.nc")
    assert set(g.variables) == set(f.variables) and g.dimensions == f.dimensions
    for name in NAMES + ("solar_irradiance", "mu0"):
        assert np.array_equal(g.variables[name][:], f.variables[name][:]), name
        assert g.variables[name].dimensions == f.variables[name].dimensions
        assert g.variables[name]._attributes == f.variables[name]._attributes, name
    for name in NAMES + ("solar_irradiance",):
        assert np.array_equal(np.asarray(m[name]).astype(np.float32), f.variables[name][:]), name


def test_sw_spectra_exit_codes(tmp_path):
    _make_files(tmp_path)
    args = _args(tmp_path)
    out = f"output={tmp_path / 'x.nc'}"
    assert run_tool("sw_spectra", *args).returncode == 147                                          # no output
    assert run_tool("sw_spectra", f"append_path={tmp_path}", "input=h2o.nc", out).returncode == 147   # no ssi
    assert run_tool("sw_spectra", *args, "gpoints=gpoints_short.nc", out).returncode == 147         # g points of the wrong length
    assert run_tool("sw_spectra", *args[:-1], "cos_solar_zenith_angle=1.5", out).returncode == 147
