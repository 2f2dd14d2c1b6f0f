"""bin/sw_spectra and the two shortwave g-point flux symbols as far as they can be checked without a GPU: the tool is built, it
refuses a call without `output` before it opens a device, and _lib carries the signatures (tests/test_abi.py checks that every
declared symbol is exported)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "sw_spectra")


def test_tool_is_built():
    assert os.path.exists(EXE) and os.access(EXE, os.X_OK), f"{EXE} not built (python -c 'import __graft_entry__ as g; g.build()')"


def test_no_arguments_is_a_parameter_error():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 147 and "output" in r.stderr + r.stdout


def test_missing_ssi_and_bad_angle_are_parameter_errors(tmp_path):
    out = f"output={tmp_path / 'x.nc'}"
    assert subprocess.run([EXE, out], capture_output=True, timeout=60).returncode == 147
    assert subprocess.run([EXE, out, "ssi=ssi.nc", "cos_solar_zenith_angle=1.5"], capture_output=True, timeout=60).returncode == 147
    assert subprocess.run([EXE, out, "ssi=ssi.nc", "cos_solar_zenith_angle=.1 .2 .3 .4 .5 .6 .7 .8 .9"], capture_output=True,
                          timeout=60).returncode == 147


def test_signatures():
    from ecckd_amd import _lib
    import ctypes as C
    sigs = _lib.SIGNATURES
    assert len(sigs["ecckd_lbl_gpoint_fluxes_sw"][1]) == 13 and len(sigs["ecckd_lbl_spectral_fluxes_sw"][1]) == 15
    assert sigs["ecckd_lbl_gpoint_fluxes_sw"][0] is C.c_int and sigs["ecckd_lbl_spectral_fluxes_sw"][0] is C.c_int
