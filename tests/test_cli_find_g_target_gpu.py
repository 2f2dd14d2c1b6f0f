"""bin/find_g_points target_g_points=N and its mirror pipeline.find_g_points(target_g_points=N): the tool asks for a NUMBER of
g points, finds the tolerances that give it and records them; a plain run with exactly those tolerances must write the same
g points, and the next tool of the chain must take the file as it takes a plain one."""
import os
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

from ecckd_amd import synthetic as syn
from test_cli_gpu import BIN, LW_CFG, _make_lw_files, _nc, _same_files, _write_columns, run_tool
from test_pipeline_gpu import NLAY, _write_spectrum

pytestmark = pytest.mark.gpu

NEW_VARIABLES = {"target_g_points", "target_search_status", "heating_rate_tolerance_scaling", "heating_rate_tolerance",
                 "target_trial_scaling", "target_trial_n_g_points"}


def _ok(r):
    assert r.returncode == 0, r.stderr + r.stdout
    return r


def _tolerances(path):
    f = _nc(path)
    tol = f.variables["heating_rate_tolerance"][:].astype(np.float64).copy()
    f.close()
    return tol


def _check_round_trip(target_file, plain_file, n_asked, first_guess):
    """Every variable of the plain file is in the target-mode file with the same values and external type; the new variables
    are in the target-mode file only and say what was done."""
    ft, fp = _nc(target_file), _nc(plain_file)
    assert not NEW_VARIABLES & set(fp.variables)
    assert set(ft.variables) == set(fp.variables) | NEW_VARIABLES
    for k, vp in fp.variables.items():
        vt = ft.variables[k]
        assert vt.typecode() == vp.typecode() and vt.dimensions == vp.dimensions and vt.shape == vp.shape, k
        assert np.array_equal(vt[...], vp[...]), k
    assert ft.constituent_id == fp.constituent_id and ft.title == fp.title
    v = ft.variables
    assert [v[k].typecode() for k in ("target_g_points", "target_search_status", "heating_rate_tolerance_scaling", "heating_rate_tolerance",
                                      "target_trial_scaling", "target_trial_n_g_points")] == ["i", "i", "d", "d", "d", "i"]
    assert v["heating_rate_tolerance"].dimensions == ("band",) and v["target_trial_scaling"].dimensions == ("target_trial",)
    scaling, status, ng = float(v["heating_rate_tolerance_scaling"][...]), int(v["target_search_status"][...]), v["band_number"].shape[0]
    assert int(v["target_g_points"][...]) == n_asked
    assert np.array_equal(v["heating_rate_tolerance"][:], scaling * np.asarray(first_guess, dtype=np.float64))
    trials = list(zip(v["target_trial_scaling"][:].tolist(), v["target_trial_n_g_points"][:].tolist()))
    assert trials[0][0] == 1.0 and (scaling, ng) in trials
    assert (status == 0) == (ng == n_asked)
    ft.close(); fp.close()
    return status, ng


@pytest.fixture(scope="module")
def lw(tmp_path_factory):
    """Two gases, two bands: ordering files, a plain run at tolerance 0.05 (N = its g points), the target run for N from the
    configured first guess 0.08 and the plain run at the tolerances the target run reports."""
    d = tmp_path_factory.mktemp("target_lw")
    _make_lw_files(d)
    os.symlink(d / "h2o.nc", d / "co2_bg_is_h2o.nc")
    for g in ("h2o", "co2"):
        _ok(run_tool("reorder_spectrum", f"input={d}/{g}.nc", f"output={d}/order_{g}.nc", "wavenumber1=0 1300", "wavenumber2=1300 3260",
                     "iprofile=0"))
    (d / "find_g.cfg").write_text(LW_CFG.format(d=d))
    _ok(run_tool("find_g_points", d / "find_g.cfg", f"output={d}/other.nc", "heating_rate_tolerance=0.05", cwd="/"))
    f = _nc(d / "other.nc")
    n = f.variables["band_number"].shape[0]
    f.close()
    r = _ok(run_tool("find_g_points", d / "find_g.cfg", f"output={d}/target.nc", f"target_g_points={n}", cwd="/"))
    tol = _tolerances(d / "target.nc")
    _ok(run_tool("find_g_points", d / "find_g.cfg", f"output={d}/plain.nc", "heating_rate_tolerance=" + " ".join(repr(float(t)) for t in tol),
                 cwd="/"))
    return dict(d=d, n=n, stdout=r.stdout, tol=tol)


def test_longwave_round_trip(lw):
    d = lw["d"]
    status, ng = _check_round_trip(d / "target.nc", d / "plain.nc", lw["n"], [0.08, 0.08])
    assert status in (0, 1)
    assert "Trial 0: scaling 1:" in lw["stdout"] and "h2o" in lw["stdout"].split("Trial 0:")[1].split("\n")[0]
    assert "heating_rate_tolerance used: " + " ".join("%.17g" % t for t in lw["tol"]) in lw["stdout"]
    f = _nc(d / "target.nc")
    assert (b"target_g_points=%d" % lw["n"]) in f.config
    f.close()


def test_the_mirror_writes_the_file_of_the_tool(ctx, lw):
    from ecckd_amd import pipeline
    d = lw["d"]
    f = _nc(d / "order_h2o.nc")                                   # the bands as the ordering files have them (clamped to the data)
    b1, b2 = f.variables["wavenumber1_band"][:].astype(np.float64), f.variables["wavenumber2_band"][:].astype(np.float64)
    f.close()
    res = pipeline.find_g_points(ctx, [dict(name="h2o", input=d / "h2o.nc", reordering_input=d / "order_h2o.nc",
                                            background=[dict(path=d / "co2.nc")]),
                                       dict(name="co2", input=d / "co2.nc", reordering_input=d / "order_co2.nc",
                                            background=[dict(path=d / "h2o.nc")], min_g_points=[2, 1])],
                                 b1, b2, 0.08, output_path=d / "py_target.nc", tolerance_tolerance=0.02, max_iterations=40,
                                 target_g_points=lw["n"])
    _same_files(d / "target.nc", d / "py_target.nc")
    assert res["target"]["target_g_points"] == lw["n"] and res["target"]["ng"] == res["ng"]
    assert np.array_equal(res["target"]["tolerance_used"], lw["tol"])


def test_create_look_up_table_takes_the_target_mode_file(lw):
    d = lw["d"]
    nlay, ncol = 12, 3
    p1 = syn.pressure_grid(nlay)
    wn, _ = syn.wavenumber_grid(12000)                                # the grid of the g-points files
    t = np.stack([syn.temperature_profile(p1) + 15.0 * (c - 1) for c in range(ncol)])
    _write_columns(d / "lut_h2o.nc", "h2o", p1, t, wn, 5, 30.0, 5e-3)
    _write_columns(d / "lut_co2.nc", "co2", p1, t, wn, 3, 8.0, 4e-4)
    for tag in ("target", "plain"):
        (d / f"lut_{tag}.cfg").write_text(
            f"input {tag}.nc\noutput raw_{tag}.nc\ngases h2o co2\n"
            "\\begin h2o\n conc_dependence linear\n input lut_h2o.nc\n\\end h2o\n"
            "\\begin co2\n conc_dependence linear\n input lut_co2.nc\n\\end co2\n")
        _ok(run_tool("create_look_up_table", f"lut_{tag}.cfg", cwd=d))
    _same_files(d / "raw_target.nc", d / "raw_plain.nc")


@pytest.fixture(scope="module")
def sw(tmp_path_factory):
    """The shortwave files of tests/test_cli_gpu.py::test_find_g_points_sw with a tolerance per band."""
    d = tmp_path_factory.mktemp("target_sw")
    nwav, lo, hi = 16000, 250.0, 50000.0
    p = syn.pressure_grid(NLAY)
    t_hl = syn.temperature_profile(p)
    wn, dwn = syn.wavenumber_grid(nwav, lo, hi)
    ssi = syn.solar_spectral_irradiance(wn, dwn)
    w = netcdf_file(str(d / "ssi.nc"), "w", version=2)
    w.createDimension("wavenumber", nwav)
    w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = ssi
    w.close()
    for g, (seed, scale, vmr) in {"h2o": (61, 5.0, 5e-3), "o3": (67, 1.5, 1e-6)}.items():
        od = syn.optical_depth(np, p, wn, syn.SEED_BASE + seed, nlines=40, column_scale=scale, dtype="float32", lo=lo, hi=hi)
        _write_spectrum(d / f"{g}.nc", g, p, t_hl, wn, od, vmr)
        _ok(run_tool("reorder_spectrum", f"input={g}.nc", f"output=order_{g}.nc", "ssi=ssi.nc", "wavenumber1=250 10000",
                     "wavenumber2=10000 50000", cwd=d))
    cfg = ("ssi ssi.nc\naveraging_method total-transmission\nheating_rate_tolerance 0.03 0.06\nmax_iterations 40\ngases h2o o3\n"
           "\\begin h2o\n input h2o.nc\n reordering_input order_h2o.nc\n background_input o3.nc\n\\end h2o\n"
           "\\begin o3\n input o3.nc\n reordering_input order_o3.nc\n background_input h2o.nc\n max_scaling 3.0\n\\end o3\n")
    (d / "sw.cfg").write_text(cfg)
    return dict(d=d, ssi=ssi)


def test_shortwave_round_trip(ctx, sw):
    from ecckd_amd import pipeline
    d = sw["d"]
    _ok(run_tool("find_g_points", "sw.cfg", "output=other.nc", "heating_rate_tolerance=0.02 0.04", cwd=d))
    f = _nc(d / "other.nc")
    n = f.variables["band_number"].shape[0]
    f.close()
    _ok(run_tool("find_g_points", "sw.cfg", "output=target.nc", f"target_g_points={n}", cwd=d))
    tol = _tolerances(d / "target.nc")
    assert tol[1] == 2.0 * tol[0]                                     # the ratio between the bands is the configured one
    _ok(run_tool("find_g_points", "sw.cfg", "output=plain.nc", "heating_rate_tolerance=" + " ".join(repr(float(t)) for t in tol), cwd=d))
    status, ng = _check_round_trip(d / "target.nc", d / "plain.nc", n, [0.03, 0.06])
    assert status in (0, 1)
    # the mirror: the same g points, tolerances and trials (its file has no solar_irradiance, with or without a target)
    f = _nc(d / "order_h2o.nc")
    b1, b2 = f.variables["wavenumber1_band"][:].astype(np.float64), f.variables["wavenumber2_band"][:].astype(np.float64)
    f.close()
    specs = [dict(name="h2o", input=d / "h2o.nc", reordering_input=d / "order_h2o.nc", background=[dict(path=d / "o3.nc")]),
             dict(name="o3", input=d / "o3.nc", reordering_input=d / "order_o3.nc", background=[dict(path=d / "h2o.nc")], max_scaling=3.0)]
    pipeline.find_g_points(ctx, specs, b1, b2, [0.03, 0.06], output_path=d / "py_target.nc", averaging_method="total-transmission",
                           max_iterations=40, ssi=sw["ssi"], target_g_points=n)
    ft, fm = _nc(d / "target.nc"), _nc(d / "py_target.nc")
    assert set(fm.variables) == set(ft.variables) - {"solar_irradiance"}
    for k, vm in fm.variables.items():
        assert vm.typecode() == ft.variables[k].typecode() and np.array_equal(vm[...], ft.variables[k][...]), k
    ft.close(); fm.close()


def test_target_exact_leaves_no_file(lw):
    """One g point (fewer than the two bands) is out of reach: status 3; with target_exact=1 that is PROCESSING_ERROR."""
    d = lw["d"]
    r = run_tool("find_g_points", d / "find_g.cfg", f"output={d}/exact.nc", "target_g_points=1", "target_exact=1", cwd="/")
    assert r.returncode == 148 and "target_exact" in r.stderr, r.stderr + r.stdout
    assert not (d / "exact.nc").exists()
    # without target_exact the nearest answer is written
    _ok(run_tool("find_g_points", d / "find_g.cfg", f"output={d}/nearest.nc", "target_g_points=1", cwd="/"))
    f = _nc(d / "nearest.nc")
    assert int(f.variables["target_search_status"][...]) == 3 and f.variables["band_number"].shape[0] >= 2
    f.close()


def _refused(d, *args, env=None):
    """The tool under a time limit of its own: a refusal comes back at once with PARAMETER_ERROR and without an output file."""
    out = d / "refused.nc"
    r = subprocess.run(["timeout", "-k", "5", "30", os.path.join(BIN, "find_g_points"), *[str(a) for a in args], f"output={out}"],
                       cwd=d, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 147, (r.returncode, r.stderr + r.stdout)
    assert "target_g_points" in r.stderr and not out.exists()
    assert "FINDING G POINTS" not in r.stdout            # refused before any gas is read
    return r


def test_refusals(lw, sw):
    d = lw["d"]
    r = _refused(d, d / "find_g.cfg", "target_g_points=12", env=dict(WORLD_SIZE="2", RANK="0"))
    assert "WORLD_SIZE" in r.stderr
    assert not [f for f in os.listdir(d) if ".part" in f]
    r = _refused(d, d / "find_g.cfg", "target_g_points=12", "sequential_bands=1")
    assert "sequential_bands" in r.stderr
    r = _refused(d, d / "find_g.cfg", "target_g_points=12", "co2.base_wavenumber_boundary=700")
    assert "base_wavenumber_boundary" in r.stderr
    r = _refused(sw["d"], "sw.cfg", "target_g_points=12", "cloud=liquid")
    assert "cloud" in r.stderr
