"""bin/lw_spectra with the key nangle=N (the CKDMIP tool's zenith-angle quadrature, test/run_ckd_lw.sh:28): the fluxes of both
output modes are those of N Gauss-Legendre angles per hemisphere, bit for bit the host mirror's pipeline.lw_spectra(nangle=N),
and per band those of bin/ckdmip_lw run with the same key in its namelist; nangle=0 is the file the tool wrote before it knew
the key; bin/sw_spectra refuses the key.  Files as in test_cli_spectra_gpu.py: 3 columns, 12 layers, 4003 wavenumbers."""
import numpy as np
import pytest
from scipy.io import netcdf_file

from test_cli_spectra_gpu import NCOL, NWAV, _make_files, _nc, run_tool

pytestmark = pytest.mark.gpu

NAMES = ("pressure_hl", "temperature_hl", "vmr_fl", "flux_dn_lw", "flux_up_lw", "optical_depth", "spectral_flux_dn_lw",
         "spectral_flux_up_lw")
FLUXES = NAMES[3:5] + NAMES[6:]
NG = 5


def _write_g_point(path, g_point):
    w = netcdf_file(str(path), "w", version=2)
    w.createDimension("wavenumber", g_point.size)
    w.createVariable("g_point", "i", ("wavenumber",))[:] = g_point
    w.close()


def _g_point():
    rng = np.random.default_rng(17)
    g = rng.integers(0, NG, size=NWAV).astype(np.int32)
    g[rng.random(NWAV) < 0.05] = -1
    g[:3] = -1
    return g


@pytest.mark.parametrize("with_gpoints", [False, True], ids=["per_wavenumber", "per_g_point"])
def test_lw_spectra_nangle(ctx, tmp_path, with_gpoints):
    """nangle=4: the attribute, every variable bit for bit the FLOAT cast of the host mirror's, fluxes that are not the
    two-stream ones next to variables that do not depend on the key; nangle=0: the bytes of every variable of the run without
    the key, and no attribute; iprofile=1: record 1 of the full run."""
    from ecckd_amd import pipeline
    _make_files(tmp_path)
    args = [f"append_path={tmp_path}", "input=h2o.nc co2.nc", "scaling=1.0 2.5"]
    g_point = None
    if with_gpoints:
        g_point = _g_point()
        _write_g_point(tmp_path / "gpoints.nc", g_point)
        args.append("gpoints=gpoints.nc")
    files = {}
    for tag, extra in (("plain", []), ("zero", ["nangle=0"]), ("four", ["nangle=4"]), ("one", ["nangle=4", "iprofile=1"])):
        files[tag] = tmp_path / f"{tag}.nc"
        r = run_tool("lw_spectra", *args, *extra, f"output={files[tag]}")
        assert r.returncode == 0, r.stderr
    plain, zero, four, one = (_nc(files[k]) for k in ("plain", "zero", "four", "one"))
    assert four.nangle == 4 and four.variables["spectral_flux_up_lw"].dimensions == plain.variables["spectral_flux_up_lw"].dimensions
    assert not hasattr(plain, "nangle") and not hasattr(zero, "nangle")
    m = pipeline.lw_spectra(ctx, [tmp_path / "h2o.nc", tmp_path / "co2.nc"], tmp_path / "mirror.nc", scaling=[1.0, 2.5], g_point=g_point,
                            nangle=4)
    mirror = _nc(tmp_path / "mirror.nc")
    assert mirror.nangle == 4
    for name in NAMES:
        a = four.variables[name][:]
        assert a.shape[0] == NCOL
        assert np.array_equal(m[name].astype(np.float32), a), name
        assert np.array_equal(mirror.variables[name][:], a), name
        assert zero.variables[name][:].tobytes() == plain.variables[name][:].tobytes(), name
        assert np.array_equal(one.variables[name][0], a[1]), name
        if name in FLUXES:
            # the quadrature is another number; in the thin limit an emission of 2 tau B stands against 1.66 tau B
            b = plain.variables[name][:].astype(np.float64)
            rel = np.abs(a.astype(np.float64) - b).max() / b.max()
            assert 1e-5 < rel < 2.0 / 1.66 - 1.0, (name, rel)
        else:
            assert a.tobytes() == plain.variables[name][:].tobytes(), name
    assert one.nangle == 4 and one.variables["flux_up_lw"].shape[0] == 1
    assert b"nangle=4" in four.config and b"nangle=" not in plain.config


def test_lw_spectra_against_ckdmip_lw(ctx, tmp_path):
    """gpoints = the band index over two contiguous bands: the per-band fluxes of lw_spectra nangle=4 against band_flux_* of
    ckdmip_lw with `nangle = 4` in its namelist and the same bands.  Both files hold FLOAT casts of doubles that agree to 1e-12
    (test_lbl_gpoint_fluxes_lw_angles_gpu.py::test_band_kernel_consistency): rtol 1.01 x 2^-23, one FLOAT step where such a
    double lies next to a rounding boundary."""
    from ecckd_amd import api
    p, t, wn, dwn, ods = _make_files(tmp_path)
    iband, begin, end = api.band_ranges(wn, [0.0, 1300.0], [1300.0, 3260.0])
    assert begin[0] == 0 and end[1] == NWAV - 1 and begin[1] == end[0] + 1
    _write_g_point(tmp_path / "bands.nc", iband.astype(np.int32))
    (tmp_path / "lw4.nam").write_text("&longwave_config\noptical_depth_name = \"optical_depth\",\nnspectralstride = 1,\nnangle = 4,\n"
                                      "do_write_spectral_boundary_fluxes = false,\nband_wavenumber1(1:2) = 0, 1300,\n"
                                      "band_wavenumber2(1:2) = 1300, 3260,\n/\n")
    r = run_tool("ckdmip_lw", "--config", "lw4.nam", "h2o.nc", "co2.nc", "--output", "lbl4.nc", cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    r = run_tool("lw_spectra", f"append_path={tmp_path}", "input=h2o.nc co2.nc", "gpoints=bands.nc", "nangle=4", "iprofile=1",
                 f"output={tmp_path / 'bands4.nc'}")
    assert r.returncode == 0, r.stderr
    a, b = _nc(tmp_path / "bands4.nc"), _nc(tmp_path / "lbl4.nc")
    rtol = 1.01 * 2.0 ** -23
    for x in ("dn", "up"):
        got = a.variables[f"spectral_flux_{x}_lw"][0].astype(np.float64)            # (half_level, band)
        want = b.variables[f"band_flux_{x}_lw"][1].astype(np.float64)
        assert got.shape == want.shape == (p.size, 2)
        print(x, "max rel diff / 2^-23", np.max(np.abs(got - want) / np.maximum(want, 1e-300)) * 2.0 ** 23)
        assert np.allclose(got, want, rtol=rtol, atol=0.0)
    assert np.all(a.variables["spectral_flux_up_lw"][0] > 0.0)


def test_refusals(tmp_path):
    """nangle outside 0..16, and the key given to sw_spectra: PARAMETER_ERROR with `nangle` in the message before anything is
    read or written."""
    _make_files(tmp_path)
    for tool, extra in (("lw_spectra", ["nangle=17"]), ("lw_spectra", ["nangle=-1"]), ("sw_spectra", ["ssi=ssi.nc", "nangle=4"])):
        out = tmp_path / "refused.nc"
        r = run_tool(tool, f"append_path={tmp_path}", "input=h2o.nc co2.nc", *extra, f"output={out}")
        assert r.returncode == 147 and "nangle" in r.stderr, (tool, extra, r.returncode, r.stderr)
        assert not out.exists()
    r = run_tool("lw_spectra", f"append_path={tmp_path}", "input=h2o.nc co2.nc", "nangle=16", "iprofile=0", f"output={tmp_path / 'ok.nc'}")
    assert r.returncode == 0 and _nc(tmp_path / "ok.nc").nangle == 16, r.stderr
