"""The Rayleigh entries of sw_spectra as far as they can be checked without a GPU: _lib and the header carry the two
signatures, lw_spectra refuses the `rayleigh` key before it opens a device, and the premise of the exact GPU tests
(test_lbl_gpoint_fluxes_sw_rayleigh_gpu.py) holds in numpy: with a Rayleigh optical depth of 0 the restated two-stream transfer
leaves no diffuse flux, and its direct and upwelling fluxes on the layout inputs sum to sw_reference exactly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpoint_layouts as L
import rayleigh_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signatures():
    """The spectral entry takes the 20 arguments of its declaration: 13 up to the Rayleigh stride, three FLOAT rows and their
    stride, three broadband rows."""
    from ecckd_amd import _lib
    sigs = _lib.SIGNATURES
    assert len(sigs["ecckd_lbl_gpoint_fluxes_sw_rayleigh"][1]) == 18 and len(sigs["ecckd_lbl_spectral_fluxes_sw_rayleigh"][1]) == 20
    assert sigs["ecckd_lbl_gpoint_fluxes_sw_rayleigh"][0] is C.c_int and sigs["ecckd_lbl_spectral_fluxes_sw_rayleigh"][0] is C.c_int


def test_the_header_declares_them():
    with open(os.path.join(ROOT, "include", "ecckd_hip.h")) as f:
        text = f.read()
    for name, nargs in (("ecckd_lbl_gpoint_fluxes_sw_rayleigh", 18), ("ecckd_lbl_spectral_fluxes_sw_rayleigh", 20)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name


def test_lw_spectra_refuses_the_key(tmp_path):
    exe = os.path.join(ROOT, "bin", "lw_spectra")
    r = subprocess.run([exe, f"output={tmp_path / 'x.nc'}", "rayleigh=rayleigh.nc"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 147 and "rayleigh" in r.stderr + r.stdout


def _case_named(name):
    return next(c for c in L.SW_CASES if c.name == name)


@pytest.mark.parametrize("name", ["layouts-1-alb-float64", "A8-nlay3-alb", "nwav257"])
def test_without_rayleigh_the_restatement_is_exactly_the_layout_reference(name):
    case = _case_named(name)
    inp, ref = L.sw_inputs(case), L.sw_reference(case)
    col = np.where(inp.g < 0, inp.ng, inp.g)
    for s, mu in enumerate(inp.cos_sza):
        d, diffuse, up = rr.two_stream_closed(inp.od.astype(np.float64), np.zeros(inp.od.shape), mu,
                                              inp.albedo if inp.albedo is not None else 0.0, inp.ssi)
        assert np.all(diffuse == 0.0)
        for lev in range(case.nlay + 1):
            gd = np.bincount(col, weights=d[lev], minlength=inp.ng + 1)
            gu = np.bincount(col, weights=up[lev], minlength=inp.ng + 1)
            assert np.array_equal(gd[:inp.ng], ref.dn[s, lev]) and np.array_equal(gu[:inp.ng], ref.up[s, lev])
            assert gd.sum() == ref.bb_dn[s, lev] and gu.sum() == ref.bb_up[s, lev]
