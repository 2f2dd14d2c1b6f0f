"""The C ABI of the resident fluxes under clouds (ecckd_flux_sky, ecckd_gas_optics_fluxes_{lw,sw}_sky_dev): the ctypes mirror
against the C compiler's layout of the header's struct, the two entry points exported and bound, and the refusals of the sky
argument through the stand-alone harness tools/check_gas_optics_fluxes_sky.cpp (host code only).  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ecckd_gas_optics_fluxes_lw_sky_dev", "ecckd_gas_optics_fluxes_sw_sky_dev")


def test_flux_sky_mirror_matches_the_header():
    from ecckd_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [name for name, _ in _lib.FluxSky._fields_]
    assert fields == ["cloud_od", "cloud_ssa", "cloud_asymmetry", "surface_emissivity", "skin_temperature", "delta_eddington"]
    lines = [' printf("%zu", sizeof(ecckd_flux_sky));\n'] + [f' printf(" %zu", offsetof(ecckd_flux_sky, {n}));\n' for n in fields]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ecckd_hip.h"\nint main(void) {\n' + "".join(lines) + ' printf("\\n");\n return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "layout.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.c"), "-o", os.path.join(d, "layout")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "layout")]).decode().split()]
    assert out[0] == C.sizeof(_lib.FluxSky)
    assert out[1:] == [getattr(_lib.FluxSky, n).offset for n in fields]
    assert all(t is C.c_void_p for _, t in _lib.FluxSky._fields_[:5]) and _lib.FluxSky._fields_[5][1] is C.c_int


def test_the_sky_entries_are_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from ecckd_amd import _lib
    lib = C.CDLL(_lib.library_path())
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    # the clear calls' arguments and one more pointer; the shortwave one without `scattering`
    lw, sw = (_lib.SIGNATURES[n] for n in ENTRIES)
    assert lw[1] == _lib.SIGNATURES["ecckd_gas_optics_fluxes_lw_dev"][1] + [C.c_void_p]
    clear_sw = _lib.SIGNATURES["ecckd_gas_optics_fluxes_sw_dev"][1]
    assert sw[1] == clear_sw[:1] + clear_sw[2:] + [C.c_void_p]
    assert lw[0] is C.c_int and sw[0] is C.c_int


def test_the_refusals_of_the_sky_argument(tmp_path):
    """check_fluxes_sky on its own: every refusal by its message and entry name, what a sound argument reports"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path / "check_gas_optics_fluxes_sky"
    csrc = os.path.join(ROOT, "ecckd_amd", "csrc")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-I" + csrc, os.path.join(ROOT, "tools", "check_gas_optics_fluxes_sky.cpp"),
                            os.path.join(csrc, "gas_optics_tables.cpp"), os.path.join(csrc, "opt_tables.cpp"), "-o", str(exe)],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.splitlines()[-1].endswith("all hold")
