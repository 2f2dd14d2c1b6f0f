"""The line-blocked layout of the longwave sweep's operands (ecckd_amd/csrc/sweep_layout.hpp) without a GPU: the stand-alone
harness tools/check_sweep_layout.cpp, built under ASan and UBSan with the line of its header comment."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the runtimes linked statically: the program then also starts where the environment preloads a library of its own)
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-static-libasan", "-static-libubsan"]


def test_blocked_layout_under_sanitizers(tmp_path):
    """The map is a bijection onto the matrix, a row is a constant away from a point's base, a tile from a line is four
    contiguous blocks, and the 32-bit condition holds and fails where it should."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx, *FLAGS, str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")], capture_output=True, text=True, timeout=300)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + probe.stderr.strip()[-300:])
    exe = tmp_path / "check_sweep_layout"
    build = subprocess.run([cxx, *FLAGS, "-I" + os.path.join(ROOT, "ecckd_amd", "csrc"), os.path.join(ROOT, "tools", "check_sweep_layout.cpp"),
                            "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.splitlines()[-1].startswith("check_sweep_layout: ok")
