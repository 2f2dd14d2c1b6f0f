"""`--scenarios` of bin/ckdmip_lw and bin/ckdmip_sw: one call with a table of scenarios writes, per scenario, the file that the
single-scenario command line writes (the loop of test/run_lw_lbl_evaluation.sh:286-323 and test/run_sw_lbl_evaluation.sh:70-260
as one call).  The reference is today's tool run once per scenario; the files hold FLOAT, so one rounding flip is allowed
(rtol 2e-7)."""
import numpy as np
import pytest

from ecckd_amd import synthetic as syn
from test_cli_gpu import _nc, _write_columns_from, run_tool

pytestmark = pytest.mark.gpu

# NAME, then per spectrum file (spec of the table, the same as command-line words)
SCENARIOS = [
    ("present", [("asis", []), ("asis", [])]),
    ("first-half", [("scale=0.5", ["--scale", "0.5"]), ("asis", [])]),
    ("second-conc", [("asis", []), ("conc=8e-4", ["--conc", "8e-4"])]),
    ("mixed", [("scale=2", ["--scale", "2"]), ("const=6e-4", ["--const", "6e-4"])]),
]
VARIANTS = ["plain", "boundary", "column-range"]


def _compare(d, files, tool, common, variant):
    """One --scenarios call against one single-scenario call per line of the table."""
    extra = ["--column-range", "2", "3"] if variant == "column-range" else []
    lines = ["# NAME OUTPUT one spec per spectrum file", ""]
    for name, specs in SCENARIOS:
        lines.append(f"{name} multi_{name}.nc " + " ".join(s for s, _ in specs) + "   # trailing comment")
    (d / "table.txt").write_text("\n".join(lines) + "\n")
    r = run_tool(tool, *common, *extra, "--scenarios", "table.txt", *files, cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    for name, specs in SCENARIOS:
        words = []
        for f, (_, flags) in zip(files, specs):
            words += flags + [f]
        r = run_tool(tool, *common, *extra, "--scenario", name, *words, "--output", f"single_{name}.nc", cwd=d)
        assert r.returncode == 0, r.stderr + r.stdout
        a, b = _nc(d / f"multi_{name}.nc"), _nc(d / f"single_{name}.nc")
        assert a.scenario == b.scenario == name.encode() and a.constituent_id == b.constituent_id
        assert dict(a.dimensions) == dict(b.dimensions) and list(a.dimensions) == list(b.dimensions)
        assert list(a.variables) == list(b.variables)
        for k, vb in b.variables.items():
            va = a.variables[k]
            assert va.shape == vb.shape and va.dimensions == vb.dimensions and va.typecode() == vb.typecode(), k
            assert np.allclose(va[...], vb[...], rtol=2e-7, atol=1e-30), (name, k)
        ncol = 2 if variant == "column-range" else 3
        assert a.dimensions["column"] == ncol and ("wavenumber" in a.dimensions) == (variant == "boundary")
        a.close(); b.close()
    # the scenarios differ: the table was not ignored
    a, b = _nc(d / "multi_present.nc"), _nc(d / "multi_mixed.nc")
    k = "flux_dn_lw" if tool == "ckdmip_lw" else "flux_dn_direct_sw"
    assert not np.allclose(a.variables[k][...], b.variables[k][...], rtol=1e-3)
    a.close(); b.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_ckdmip_lw_scenarios(ctx, tmp_path, variant):
    from test_pipeline_gpu import make_do_all_inputs
    d = tmp_path
    make_do_all_inputs(ctx, d)
    boundary = "true" if variant == "boundary" else "false"
    (d / "lw.nam").write_text("&longwave_config\noptical_depth_name = \"optical_depth\",\nnspectralstride = 1,\nnangle = 0, ! classic\n"
                              f"do_write_spectral_boundary_fluxes = {boundary},\nband_wavenumber1(1:2) = 0, 1300,\n"
                              "band_wavenumber2(1:2) = 1300, 3260,\niverbose = 3\n/\n")
    _compare(d, ["ideal_h2o.nc", "ideal_co2.nc"], "ckdmip_lw", ["--config", "lw.nam"], variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_ckdmip_sw_scenarios(ctx, tmp_path, variant):
    from scipy.io import netcdf_file
    d = tmp_path
    # the inputs of test_cli_gpu.test_ckdmip_sw_stand_in
    nlay, nwav, lo, hi = 16, 8000, 250.0, 50000.0
    p1 = syn.pressure_grid(nlay)
    wn, dwn = syn.wavenumber_grid(nwav, lo, hi)
    ssi = syn.solar_spectral_irradiance(wn, dwn)
    w = netcdf_file(str(d / "ssi.nc"), "w", version=2)
    w.createDimension("wavenumber", nwav)
    w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = ssi
    w.close()
    t0 = syn.temperature_profile(p1)
    base = {"h2o": (syn.optical_depth(np, p1, wn, syn.SEED_BASE + 81, nlines=60, column_scale=3.0, dtype="float32", lo=lo, hi=hi), 5e-3),
            "o3": (syn.optical_depth(np, p1, wn, syn.SEED_BASE + 83, nlines=30, column_scale=0.8, dtype="float32", lo=lo, hi=hi), 1e-6)}
    for g, (od, vmr) in base.items():
        _write_columns_from(d / f"ideal_{g}.nc", g, p1, [t0 - 20.0, t0, t0 + 20.0], wn, od, vmr)
    boundary = "\ndo_write_spectral_boundary_fluxes = true," if variant == "boundary" else ""
    (d / "sw.nam").write_text("&shortwave_config\noptical_depth_name = \"optical_depth\",\nsurf_albedo = 0.15,\nuse_mu0_dimension = true,\n"
                              f"cos_solar_zenith_angle(1:5) = 0.1, 0.3, 0.5, 0.7, 0.9,\nnspectralstride = 1,{boundary}\n"
                              "band_wavenumber1(1:2) = 250, 10000,\nband_wavenumber2(1:2) = 10000, 50000,\niverbose = 3\n/\n")
    _compare(d, ["ideal_h2o.nc", "ideal_o3.nc"], "ckdmip_sw", ["--config", "sw.nam", "--ssi", "ssi.nc"], variant)
    f = _nc(d / "multi_present.nc")
    assert f.variables["band_flux_up_sw"].shape == (2 if variant == "column-range" else 3, 5, nlay + 1, 2)
    f.close()
