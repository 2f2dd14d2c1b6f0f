"""The launch plan of the fused fluxes (fluxes_plan of ecckd_amd/csrc/gas_optics_tables.cpp) without a GPU: through ctypes on
the host-only entry point ecckd_gas_optics_fluxes_plan, and the stand-alone harness tools/check_gas_optics_fluxes_plan.cpp built
under ASan and UBSan with the line of its header comment."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-static-libasan", "-static-libubsan"]
NENT = 24                       # the five-gas synthetic model: four gases of 4 entries and a look-up-table gas of 8
BROADBAND, BANDS, SPECTRAL, HEATING, DIRECT = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def plan():
    import __graft_entry__ as g
    g.build()
    from ecckd_amd import api
    return api.gas_optics_fluxes_plan


# ng -> (columns per block, layers per tile, passes over g, levels per reduction)
FIELDS = {1: (256, 1, 1, 8), 16: (16, 4, 1, 8), 33: (7, 9, 1, 8), 64: (4, 16, 1, 8), 65: (3, 21, 1, 8), 257: (1, 64, 2, 7)}


@pytest.mark.parametrize("nlay", [1, 54, 137])
@pytest.mark.parametrize("ng", sorted(FIELDS))
def test_plan_fields(plan, ng, nlay):
    cpb, tile, passes, levels = FIELDS[ng]
    for mode, rows in ((0, 4), (1, 3), (2, 5)):
        p = plan(100000, nlay, ng, NENT, nband=3, mode=mode, wants=BROADBAND | HEATING)
        assert (p["columns_per_block"], p["layer_tile"], p["g_passes"], p["reduce_levels"], p["threads"]) == (cpb, tile, passes, levels, 256)
        assert p["state_rows"] == rows
        assert p["ngroup"] == -(-100000 // cpb) and p["grid"] == min(p["ngroup"], 3 * 256)
        cells, width = cpb * tile, max(256, ng)
        assert cells <= 256 and p["lds_bytes"] == cells * (NENT * 12 + 8) + levels * width * 8 <= 160 * 1024
        # per block: the state rows of every pass, then the broadband doubles of its columns, in whole 256-byte lines
        doubles = passes * rows * (nlay + 1) * 256 + 2 * cpb * (nlay + 1)
        assert p["scratch_bytes"] == p["grid"] * (-(-doubles // 32) * 32) * 8


@pytest.mark.parametrize("ng", [16, 64, 257])
def test_scratch_stops_growing_with_ncol(plan, ng):
    a, b = plan(100000, 54, ng, NENT), plan(1000000, 54, ng, NENT)
    assert a["grid"] == b["grid"] == 768 and a["scratch_bytes"] == b["scratch_bytes"]
    assert plan(2 ** 31 - 1, 54, ng, NENT)["scratch_bytes"] == a["scratch_bytes"]
    # 3 blocks per compute unit at 54 layers, ng 64: four rows of 55 x 256 doubles each
    if ng == 64:
        assert a["scratch_bytes"] == 768 * (4 * 55 * 256 + 2 * 4 * 55 + 8) * 8


def test_forced_grid(plan):
    assert plan(29, 7, 33, NENT)["grid"] == 5                          # five groups of seven columns
    for forced, grid in ((1, 1), (2, 2), (5, 5), (100, 5)):
        p = plan(29, 7, 33, NENT, grid_override=forced)
        assert p["grid"] == grid and p["ngroup"] == 5
        assert p["scratch_bytes"] * 5 == plan(29, 7, 33, NENT)["scratch_bytes"] * grid
    assert plan(100000, 54, 64, NENT, cu_count=304)["grid"] == 912


def test_refusals(plan):
    from ecckd_amd import api
    messages = []

    def refused(*words, **kw):
        args = dict(ncol=4, nlay=7, ng=16, nent=NENT, nband=3)
        args.update(kw)
        with pytest.raises(api.EcckdError) as e:
            plan(**args)
        assert e.value.code == 147
        for w in words:
            assert w in e.value.message, e.value.message
        messages.append(e.value.message)

    refused("positive", "ncol=0", ncol=0)
    refused("positive", "nlay=-1", nlay=-1)
    refused("more than one call", ncol=2 ** 31)
    refused("bad plan dimensions", ng=0)
    refused("mode 3", mode=3)
    refused("nangle = 17", nangle=17)
    refused("no output", wants=0)
    refused("iband_per_g", nband=0, wants=BANDS)
    refused("direct outputs", mode=1, wants=DIRECT)
    refused("bytes of LDS", "163840", ng=1, nent=64)
    assert len(set(messages)) == len(messages)
    assert plan(4, 7, 16, NENT, mode=2, wants=31)["state_rows"] == 5


def test_plan_under_sanitizers(tmp_path):
    """ng 1..1024, nlay 1..200, ncol up to 2^31 - 1: every index of the kernel against the plan's sizes"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx, *FLAGS, str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")], capture_output=True, text=True, timeout=300)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + probe.stderr.strip()[-300:])
    exe = tmp_path / "check_gas_optics_fluxes_plan"
    csrc = os.path.join(ROOT, "ecckd_amd", "csrc")
    build = subprocess.run([cxx, *FLAGS, "-I" + csrc, os.path.join(ROOT, "tools", "check_gas_optics_fluxes_plan.cpp"),
                            os.path.join(csrc, "gas_optics_tables.cpp"), os.path.join(csrc, "opt_tables.cpp"), "-o", str(exe)],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.splitlines()[-1].endswith("all hold")
