"""`--scenarios-rayleigh` of bin/ckdmip_sw and the symbols of the many-scenario Rayleigh fluxes as far as they can be checked
without a GPU: _lib carries the signatures, the scenarios-per-launch rule is the documented formula, and every refusal of the
switch is decided before a device is opened or a file created (exit status 147 = PARAMETER_ERROR, the switch named in quotes)."""
import ctypes as C

import pytest

from test_lbl_scenarios_host import GOOD, run, table

BUDGET = 512 << 20                                   # RAYLEIGH_SCENARIO_BYTES of csrc/lbl_scenarios_sw_rayleigh.hip


def test_signatures():
    from ecckd_amd import _lib
    sigs = _lib.SIGNATURES
    res, args = sigs["ecckd_lbl_band_fluxes_sw_rayleigh_scenarios"]
    assert res is C.c_int and len(args) == 25
    res, args = sigs["ecckd_lbl_rayleigh_scenarios_per_launch"]
    assert res is C.c_int and args == [C.c_int, C.c_int, C.c_size_t]
    lib = _lib.load_library()
    assert hasattr(lib, "ecckd_lbl_band_fluxes_sw_rayleigh_scenarios") and hasattr(lib, "ecckd_lbl_rayleigh_scenarios_per_launch")


def _formula(budget, nlay, nsza, nchunk):
    """whole scenarios whose chunk partials [nchunk][nsza][3][nlay+1] doubles fit the budget, one at least (and what an int holds)"""
    return min(2 ** 31 - 1, max(1, budget // (nchunk * nsza * 3 * (nlay + 1) * 8)))


SHAPES = [(54, 5, 16384), (54, 5, 1), (1, 1, 3), (3, 5, 4), (8, 8, 3), (54, 8, 20000), (600, 8, 100000)]


def test_scenarios_per_launch(monkeypatch):
    from ecckd_amd import api
    monkeypatch.delenv("ECCKD_RAYLEIGH_SCENARIO_BYTES", raising=False)
    for nlay, nsza, nchunk in SHAPES:
        assert api.lbl_rayleigh_scenarios_per_launch(nlay, nsza, nchunk) == _formula(BUDGET, nlay, nsza, nchunk), (nlay, nsza, nchunk)
    # 2^22 wavenumbers in 13 bands: about 108 MB of partials per scenario, 4 scenarios in 512 MB
    assert api.lbl_rayleigh_scenarios_per_launch(54, 5, 16390) == 4
    assert api.lbl_rayleigh_scenarios_per_launch(600, 8, 100000) == 1                 # more than the budget: still one
    for budget in (1, 1000, 3 * 4 * 5 * 3 * 4 * 8, 3 * 4 * 5 * 3 * 4 * 8 - 1, 1 << 40):
        monkeypatch.setenv("ECCKD_RAYLEIGH_SCENARIO_BYTES", str(budget))
        for nlay, nsza, nchunk in SHAPES:
            assert api.lbl_rayleigh_scenarios_per_launch(nlay, nsza, nchunk) == _formula(budget, nlay, nsza, nchunk), (budget, nlay, nsza, nchunk)
    monkeypatch.setenv("ECCKD_RAYLEIGH_SCENARIO_BYTES", "1")
    assert api.lbl_rayleigh_scenarios_per_launch(54, 5, 16384) == 1
    monkeypatch.setenv("ECCKD_RAYLEIGH_SCENARIO_BYTES", str(3 * 4 * 5 * 3 * 4 * 8))
    assert api.lbl_rayleigh_scenarios_per_launch(3, 5, 4) == 3
    monkeypatch.setenv("ECCKD_RAYLEIGH_SCENARIO_BYTES", "0")                          # not a budget: the default holds
    assert api.lbl_rayleigh_scenarios_per_launch(54, 5, 16390) == 4


@pytest.mark.parametrize("tool, args, named", [
    ("ckdmip_sw", ["--scenarios-rayleigh", "ray.nc", "--output", "x.nc", "a.nc", "b.nc"], "--scenarios"),                  # no table
    ("ckdmip_lw", ["--scenarios", "scen.txt", "--scenarios-rayleigh", "ray.nc", "a.nc", "b.nc"], "longwave"),
    ("ckdmip_lw", ["--scenarios-rayleigh", "ray.nc", "--output", "x.nc", "a.nc", "b.nc"], "longwave"),
    ("ckdmip_sw", ["--scenarios", "scen.txt", "--scenarios-rayleigh", "ray.nc", "--rayleigh", "ray.nc", "a.nc", "b.nc"], "--rayleigh"),
    ("ckdmip_sw", ["--scenarios", "scen.txt", "--scenarios-rayleigh", "ray.nc", "--rayleigh-scattering", "a.nc", "b.nc"], "--rayleigh-scattering"),
    ("ckdmip_sw", ["--scenarios", "scen.txt", "--scenarios-rayleigh", "ray.nc", "--ckd", "od.nc", "a.nc", "b.nc"], "--ckd"),
    ("ckdmip_sw", ["--scenarios", "scen.txt", "--scenarios-rayleigh", "ray.nc", "--merge-only", "a.nc", "b.nc"], "--merge-only"),
])
def test_scenarios_rayleigh_refusals(tmp_path, tool, args, named):
    table(tmp_path, GOOD)
    r = run(tool, *args, cwd=tmp_path)
    assert r.returncode == 147, r.stderr
    assert "\"--scenarios-rayleigh\"" in r.stderr and named in r.stderr
    assert not list(tmp_path.glob("*.nc"))           # nothing was created


def test_scenarios_rayleigh_needs_its_file(tmp_path):
    r = run("ckdmip_sw", "--scenarios", table(tmp_path, GOOD), "a.nc", "--scenarios-rayleigh", cwd=tmp_path)
    assert r.returncode == 147 and "--scenarios-rayleigh needs" in r.stderr


@pytest.mark.parametrize("switch, args", [
    ("--rayleigh", ["--rayleigh", "ray.nc"]),
    ("--rayleigh-scattering", ["--rayleigh-scattering"]),
])
def test_the_older_spelling_stays_refused(tmp_path, switch, args):
    """`--rayleigh FILE --scenarios TABLE` is refused as before the new switch existed, with the message it always had."""
    r = run("ckdmip_sw", *args, "--scenarios", table(tmp_path, GOOD), "a.nc", "b.nc", cwd=tmp_path)
    assert r.returncode == 147, r.stderr
    assert f"\"{switch}\" cannot be combined with --scenarios" in r.stderr
    assert not list(tmp_path.glob("*.nc"))
