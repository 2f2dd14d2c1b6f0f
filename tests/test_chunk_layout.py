"""The chunk layout of the error sweep (csrc/chunk_layout.hpp) through tools/check_chunk_layout.cpp: a stand-alone program
that includes the header as it is and holds it to the cover, alignment and chunk-count properties listed at its top.  Built
twice - plainly, and with the address and undefined-behaviour sanitizers linked into the program itself - and run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "check_chunk_layout.cpp")
INC = "-I" + os.path.join(ROOT, "ecckd_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _build(exe, flags):
    return subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", *flags, INC, SRC, "-o", exe],
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("kind", ["plain", "sanitized"])
def test_check_chunk_layout(tmp_path, kind):
    exe = str(tmp_path / ("check_chunk_layout_" + kind))
    if kind == "plain":
        r = _build(exe, ["-O2"])
    else:
        # the sanitizers' runtimes inside the program: nothing has to come first among the libraries the loader brings
        r = _build(exe, SAN + ["-static-libasan", "-static-libubsan"])
        if r.returncode != 0:
            r = _build(exe, SAN)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("check_chunk_layout: ok"), r.stdout
