"""The host step of the gas-optics handle (ecckd_amd/csrc/gas_optics_tables.cpp) without a GPU: the stand-alone harness
tools/check_gas_optics_tables.cpp, built under ASan and UBSan with the line of its header comment."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the runtimes linked statically: the program then also starts where the environment preloads a library of its own)
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-static-libasan", "-static-libubsan"]


def test_host_step_under_sanitizers(tmp_path):
    """Models of 1 / 33 / 64 / 65 g points with every concentration dependence flattened and compared element by element, the
    refusals of the model, of a call and of the launch plan by their messages, the plan at the tile's edges and past 2^32."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx, *FLAGS, str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")], capture_output=True, text=True, timeout=300)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + probe.stderr.strip()[-300:])
    exe = tmp_path / "check_gas_optics_tables"
    csrc = os.path.join(ROOT, "ecckd_amd", "csrc")
    build = subprocess.run([cxx, *FLAGS, "-I" + csrc, os.path.join(ROOT, "tools", "check_gas_optics_tables.cpp"),
                            os.path.join(csrc, "gas_optics_tables.cpp"), os.path.join(csrc, "opt_tables.cpp"), "-o", str(exe)],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.splitlines()[-1].endswith("all hold")
