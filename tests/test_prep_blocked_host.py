"""The host side of the blocked-store gas preparation (ecckd_amd/csrc/sweep_layout.hpp: the decision in front of the
preparation kernel, and the addresses the kernel's lanes store to) without a GPU: the stand-alone harness
tools/check_prep_blocked.cpp, built under ASan and UBSan with the line of its header comment."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the runtimes linked statically: the program then also starts where the environment preloads a library of its own)
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-static-libasan", "-static-libubsan"]


def test_blocked_preparation_host_side_under_sanitizers(tmp_path):
    """The decision holds and fails where it should; every blocked store of a preparation of 16, 1 168 and 4 112 points
    lands inside its matrix, on the element the layout gives it, and every element is written."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx, *FLAGS, str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")], capture_output=True, text=True, timeout=300)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + probe.stderr.strip()[-300:])
    exe = tmp_path / "check_prep_blocked"
    build = subprocess.run([cxx, *FLAGS, "-I" + os.path.join(ROOT, "ecckd_amd", "csrc"), os.path.join(ROOT, "tools", "check_prep_blocked.cpp"),
                            "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.splitlines()[-1].startswith("check_prep_blocked: ok")
