"""The key nangle of bin/lw_spectra and the two quadrature symbols as far as they can be checked without a GPU: the tools read
and range-check the key before they open a device, bin/sw_spectra refuses it, and _lib carries the signatures - the two-stream
argument lists with `int nangle` after the handle (tests/test_abi.py checks that every declared symbol is exported).  The C
entry points refuse a bad nangle before they look at any other argument, so that is checked here with NULL pointers."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


@pytest.mark.parametrize("tool,extra", [("lw_spectra", ["nangle=17"]), ("lw_spectra", ["nangle=-1"]),
                                        ("sw_spectra", ["ssi=ssi.nc", "nangle=4"]), ("sw_spectra", ["ssi=ssi.nc", "nangle=0"])])
def test_the_key_is_checked_before_a_device_is_opened(tmp_path, tool, extra):
    out = tmp_path / "x.nc"
    r = subprocess.run([os.path.join(BIN, tool), f"output={out}", "input=absent.nc", *extra], capture_output=True, text=True, timeout=60)
    assert r.returncode == 147 and "nangle" in r.stderr, (r.returncode, r.stderr)
    assert not out.exists()


def test_signatures():
    from ecckd_amd import _lib
    sigs = _lib.SIGNATURES
    for name in ("ecckd_lbl_gpoint_fluxes_lw", "ecckd_lbl_spectral_fluxes_lw"):
        rt, args = sigs[name]
        rt_a, args_a = sigs[name + "_angles"]
        assert rt_a is rt is C.c_int
        assert args_a == args[:1] + [C.c_int] + args[1:]


@pytest.mark.parametrize("nangle", [-1, 17, 1 << 20])
def test_entry_points_refuse_nangle_first(nangle):
    from ecckd_amd import _lib
    lib = _lib.load_library()
    rc = lib.ecckd_lbl_gpoint_fluxes_lw_angles(None, nangle, 0, None, None, 0, 0, None, None, None, None)
    assert rc == 147 and b"nangle" in lib.ecckd_last_error()
    rc = lib.ecckd_lbl_spectral_fluxes_lw_angles(None, nangle, 0, 0, None, None, None, None, 0, 0, None, None, 0, None, None)
    assert rc == 147 and b"nangle" in lib.ecckd_last_error()
    # a valid nangle goes on to the other arguments: the handle is missing
    rc = lib.ecckd_lbl_gpoint_fluxes_lw_angles(None, 16, 0, None, None, 0, 0, None, None, None, None)
    assert rc == 147 and b"bad argument" in lib.ecckd_last_error()
