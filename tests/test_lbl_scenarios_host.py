"""`--scenarios` of bin/ckdmip_lw and bin/ckdmip_sw and the scenario flux symbols as far as they can be checked without a GPU: every
refusal of the option is decided before a device is opened (exit status 147 = PARAMETER_ERROR and a message naming the cause), _lib
carries the signatures, and the slots-per-launch rule is the documented formula."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ("ckdmip_lw", "ckdmip_sw")


def run(tool, *args, cwd=None):
    exe = os.path.join(ROOT, "bin", tool)
    assert os.path.exists(exe) and os.access(exe, os.X_OK), f"{exe} not built (python -c 'import __graft_entry__ as g; g.build()')"
    return subprocess.run([exe, *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=60)


def table(tmp_path, text):
    (tmp_path / "scen.txt").write_text(text)
    return "scen.txt"


GOOD = "# name output h2o co2\npresent out_present.nc asis asis\n\nco2-2x out_co2.nc asis scale=2  # doubled\n"


@pytest.mark.parametrize("tool", TOOLS)
@pytest.mark.parametrize("extra, named", [
    (["--merge-only"], "--merge-only"),
    (["--ckd", "od.nc"], "--ckd"),
    (["--output", "x.nc"], "--output"),
    (["--scenario", "present"], "--scenario"),
])
def test_scenarios_refuses_the_single_scenario_options(tmp_path, tool, extra, named):
    r = run(tool, "--scenarios", table(tmp_path, GOOD), *extra, "a.nc", "b.nc", cwd=tmp_path)
    assert r.returncode == 147, r.stderr
    assert "--scenarios" in r.stderr and named in r.stderr


@pytest.mark.parametrize("tool", TOOLS)
@pytest.mark.parametrize("flag", ["--scale", "--conc", "--const"])
def test_scenarios_refuses_a_per_file_scaling(tmp_path, tool, flag):
    r = run(tool, "--scenarios", table(tmp_path, GOOD), "a.nc", flag, "2", "b.nc", cwd=tmp_path)
    assert r.returncode == 147, r.stderr
    assert "--scenarios" in r.stderr and "per-file" in r.stderr and flag in r.stderr


@pytest.mark.parametrize("tool", TOOLS)
@pytest.mark.parametrize("text, words", [
    ("present out.nc asis\n", ["scen.txt:1", "1 scaling spec(s) for 2 spectrum file(s)"]),                # too few
    ("present out.nc asis asis scale=2\n", ["scen.txt:1", "3 scaling spec(s) for 2 spectrum file(s)"]),   # too many
    ("present\n", ["scen.txt:1", "0 scaling spec(s)"]),                                                   # not even an output
    ("present out.nc asis times=2\n", ["scen.txt:1", "unknown scaling spec", "times=2"]),
    ("present out.nc asis double\n", ["unknown scaling spec", "double"]),
    ("present out.nc scale= asis\n", ["unknown scaling spec", "scale="]),
    ("present out.nc scale=2x asis\n", ["unknown scaling spec", "scale=2x"]),
    ("a out.nc asis asis\n# the same file again\nb out.nc asis scale=2\n", ["scen.txt:3", "duplicate output", "out.nc"]),
    ("", ["scen.txt", "empty"]),
    ("# only a comment\n\n   \n", ["scen.txt", "empty"]),
])
def test_scenarios_refuses_a_bad_table(tmp_path, tool, text, words):
    r = run(tool, "--scenarios", table(tmp_path, text), "a.nc", "b.nc", cwd=tmp_path)
    assert r.returncode == 147, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert not list(tmp_path.glob("*.nc"))           # nothing was created


@pytest.mark.parametrize("tool", TOOLS)
def test_scenarios_needs_its_table_and_spectrum_files(tmp_path, tool):
    r = run(tool, "--scenarios", "missing.txt", "a.nc", cwd=tmp_path)
    assert r.returncode == 147 and "missing.txt" in r.stderr
    r = run(tool, "--scenarios", table(tmp_path, GOOD), cwd=tmp_path)
    assert r.returncode == 147 and "No spectrum files" in r.stderr
    r = run(tool, "a.nc", "--scenarios", cwd=tmp_path)
    assert r.returncode == 147 and "--scenarios needs" in r.stderr


def test_signatures_and_slots_per_launch():
    import ctypes as C
    from ecckd_amd import _lib, api
    sigs = _lib.SIGNATURES
    assert len(sigs["ecckd_lbl_band_fluxes_lw_scenarios"][1]) == 20 and len(sigs["ecckd_lbl_band_fluxes_sw_scenarios"][1]) == 20
    assert sigs["ecckd_lbl_band_fluxes_lw_scenarios"][0] is C.c_int and sigs["ecckd_lbl_band_fluxes_sw_scenarios"][0] is C.c_int
    # 4 waves x T slots x 2 (nlay+1) doubles within 42 KB (longwave) / 58 KB (shortwave), T at most 8 / 16
    for nlay in (1, 3, 54, 83, 84, 114, 200, 671, 672, 927, 928):
        assert api.lbl_scenarios_slots(False, nlay) == min(8, 43008 // (64 * (nlay + 1))), nlay
        assert api.lbl_scenarios_slots(True, nlay) == min(16, 59392 // (64 * (nlay + 1))), nlay
    assert api.lbl_scenarios_slots(False, 54) == 8 and api.lbl_scenarios_slots(True, 54) == 16
    assert api.lbl_scenarios_slots(False, 671) == 1 and api.lbl_scenarios_slots(False, 672) == 0
    assert api.lbl_scenarios_slots(True, 927) == 1 and api.lbl_scenarios_slots(True, 928) == 0
