"""The part files of a several-process bin/find_g_points (ecckd_amd/cli/find_g_parts.hpp) without a GPU: the stand-alone
harness tools/check_find_g_parts.cpp, built under ASan and UBSan with the line of its header comment."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the runtimes linked statically: the program then also starts where the environment preloads a library of its own)
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-static-libasan", "-static-libubsan"]


def test_part_file_protocol_under_sanitizers(tmp_path):
    """Written, read back, cut short at every byte, spoilt headers, failure markers, the time-out: every refusal by its message,
    and no read past what a file holds."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx, *FLAGS, str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")], capture_output=True, text=True, timeout=300)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + probe.stderr.strip()[-300:])
    exe = tmp_path / "check_find_g_parts"
    build = subprocess.run([cxx, *FLAGS, os.path.join(ROOT, "tools", "check_find_g_parts.cpp"), "-o", str(exe)], capture_output=True, text=True,
                           timeout=300)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.splitlines()[-1] == "check_find_g_parts: ok"
