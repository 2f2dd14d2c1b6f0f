"""CPU checks of the inputs of test_gpoint_bin_edges_gpu.py (gpoint_layouts.py): that the designed tile layouts reach every
branch of the tile binner of csrc/gpoint_bin.hpp, that the numbers they are designed for are still those of the sources, and
that the exact shortwave inputs are exact: every sum the device forms is representable whatever the order of its additions."""
import os
import re

import numpy as np
import pytest

import gpoint_layouts as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ecckd_amd", "csrc")

# the segment combinations (cont_in, brk == 0, collects, tail is GB_NONE), written out: 11 of the 16
SEGMENTS = {
    (False, False, False, False),   # begins a column, breaks, its last column ends with it
    (False, False, True, False),    # begins a column, breaks, its last column goes on in the next segment: collector with a break
    (False, False, False, True),    # begins a column, breaks, ends in GB_NONE
    (False, True, False, False),    # one column that begins and ends with the segment
    (False, True, True, False),     # one column that begins with the segment and goes on: collector without a break
    (False, True, False, True),     # GB_NONE begins with the segment
    (True, False, False, False),    # continues a column (parked piece), breaks, its last column ends with it
    (True, False, True, False),     # continues a column, breaks, its last column goes on: parks one piece and collects another
    (True, False, False, True),     # continues a column, breaks, ends in GB_NONE
    (True, True, False, False),     # the middle of a chain: parks its only piece and never collects
    (True, True, False, True),      # GB_NONE throughout
}
# the chains (parked pieces the collector adds, the chain ends inside a segment, it reaches segment 31): 14 of the 16
CHAINS = {(cls, inside, reaches) for cls in ("1", "2", "3..30") for inside in (False, True) for reaches in (False, True)}
CHAINS |= {("31", False, True), ("31", True, True)}
# a launch of ONE column: the column, then GB_NONE.  No segment has a break and a column at its end.
ONE_COLUMN_SEGMENTS = {s for s in SEGMENTS if s[1] or s[3]}


def test_the_listed_combinations_are_the_ones_that_can_occur():
    assert SEGMENTS == L.SEGMENT_COMBINATIONS and len(SEGMENTS) == 11
    assert CHAINS == L.CHAIN_COMBINATIONS and len(CHAINS) == 14


def test_layouts_are_what_they_say():
    """every tile of the layout spectrum ranks to its layout, with the lanes permuted and in order; the named layouts exist"""
    sp = L.spectrum(300, 255)
    names = {name.split("/")[0] for name, _ in sp.tiles}
    for want in ["one_chain", "32x8", "3_250_3", "8_240_8", "5_123_128", "256x1", "cycle_1_9", "none_1", "none_8", "none_9",
                 "none_100", "none_only", "last_255"] + ["break_at_%d" % r for r in range(1, 8)]:
        assert want in names, want
    keys = L.launch_keys(sp.g, 0, 300, True)
    scrambled = 0
    for t, (name, runs) in enumerate(sp.tiles):
        want = np.concatenate([np.full(n, 300 if c < 0 else c) for c, n in runs] + [np.full(L.TILE - sum(n for _, n in runs), L.NONE)])
        assert np.array_equal(keys[t], want), name
        tile = sp.g[t * L.TILE:(t + 1) * L.TILE]
        scrambled += bool(np.any(np.diff(np.where(tile < 0, 300, tile)) < 0))
        if name.endswith("/id"):
            assert np.all(np.diff(np.where(tile < 0, 300, tile)) >= 0), name
    assert scrambled >= len(sp.tiles) // 2 - 3          # (a one-column tile cannot be out of order)
    assert sp.nwav == (len(sp.tiles) - 1) * L.TILE + 255
    assert np.count_nonzero(sp.g == sp.empty_g) == 0
    assert np.flatnonzero(sp.g == sp.lone_g).tolist() and np.all(np.flatnonzero(sp.g == sp.lone_g) >= sp.nwav - 255)
    assert np.count_nonzero(sp.g == sp.lone_g) == 1
    # the -1 runs of 0, 1, 8, 9 and 100 points; a tile of -1 only
    none_runs = {([n for c, n in runs if c < 0] or [0])[0] for _, runs in sp.tiles}
    assert {0, 1, 8, 9, 100, 256} <= none_runs


def test_a_single_launch_reaches_every_branch():
    """ng = 300 in one launch, over the five last tiles (1, 7, 8, 9 and 255 live lanes: GB_NONE occurs in dead lanes only)"""
    segs, chs = set(), set()
    for live in (1, 7, 8, 9, 255):
        sp = L.spectrum(300, live)
        assert sp.nwav % L.TILE == live
        s, c, _ = L.reached(sp.g, [(0, 300, True)])
        segs |= s
        chs |= c
    assert segs == SEGMENTS, sorted(SEGMENTS - segs)
    assert chs == CHAINS, sorted(CHAINS - chs)
    # 256 different columns in one tile
    keys = L.launch_keys(L.spectrum(300, 255).g, 0, 300, True)
    assert any(np.unique(k).size == L.TILE for k in keys)


@pytest.mark.parametrize("case", L.RANGE_CASES + L.LW_RANGE_CASES, ids=lambda c: c.name)
def test_every_column_range_reaches_every_branch(case):
    """The launches of the multi-launch cases, one by one.  A launch of three or more columns reaches every chain and every
    segment combination (where it is the only launch GB_NONE stands in the dead lanes of the last tile alone, at offset 5 of
    a segment: the two combinations in which GB_NONE begins a segment need another launch's columns); a launch of one
    column reaches what one column can; every launch of several has a tile that is GB_NONE only."""
    sp = L.case_spectrum(case)
    if isinstance(case, L.SwCase):
        angles, launches = L.sw_split(case.nlay, case.nsza, case.ng)
        assert angles == [1, 1] and [n for _, n, _ in launches] == L.RANGE_SPLITS[case.ng]
        assert L.sw_cap(case.nlay) == 67
    else:
        launches = L.lw_ranges(case.nlay, case.ng)
        assert [n for _, n, _ in launches] == L.LW_RANGE_SPLITS[case.ng]
        assert L.lw_max_cols(case.nlay) == 48
    assert launches[0][2] and not any(w for _, _, w in launches[1:]) and sum(n for _, n, _ in launches) == case.ng
    # the last launch is exactly full (with the column of "none" where it is the first too) or has one column
    assert launches[-1][1] + (1 if len(launches) == 1 else 0) in (1, L.sw_cap(54) if isinstance(case, L.SwCase) else 48)
    for launch in launches:
        segs, chs, none_tiles = L.reached(sp.g, [launch])
        if launch[1] >= 3:
            want = SEGMENTS if len(launches) > 1 else SEGMENTS - {(False, False, False, True), (False, True, False, True)}
            assert segs == want, (launch, sorted(want - segs))
            assert chs == CHAINS, (launch, sorted(CHAINS - chs))
        else:
            assert launch[1] == 1 and segs <= ONE_COLUMN_SEGMENTS and segs >= ONE_COLUMN_SEGMENTS - {(False, True, False, False)}
            assert chs >= {("3..30", False, False), ("3..30", True, False), ("31", False, True), ("31", True, True)}
        assert none_tiles == (1 if len(launches) > 1 else 0)


def test_small_maps_keep_the_chains():
    """the layouts fitted to 5 usable columns (ng = 7) still reach every chain: the angle cases bin what the sweep bins"""
    for case in L.ANGLE_CASES[:1] + L.DEPTH_CASES + [L.BIG_CASE]:
        # (the large case repeats the full tiles of its layout spectrum: one period says what it reaches)
        g = L.spectrum(case.ng, L.TILE).g if case.kind == "cyclic" else L.case_spectrum(case).g
        segs, chs, _ = L.reached(g, [(0, case.ng, True)])
        assert chs == CHAINS, (case.name, sorted(CHAINS - chs))
        assert segs >= {s for s in SEGMENTS if not s[3]}, case.name


def test_the_constants_are_those_of_the_sources():
    """256 / 8 / 32 / 2048 and the accumulator budgets, read out of gpoint_bin.hpp and gmap_layout.hpp (the chunks of
    create_lut.hip)"""
    with open(os.path.join(CSRC, "gpoint_bin.hpp")) as f:
        hpp = f.read()
    with open(os.path.join(CSRC, "gmap_layout.hpp")) as f:
        lut = f.read()

    def const(text, name):
        m = re.search(r"constexpr\s+(?:int|size_t)\s+%s\s*=\s*([^;]+);" % name, text)
        assert m, name
        return m.group(1).strip()

    assert const(hpp, "GB_THREADS") == "256" and L.TILE == 256
    assert const(hpp, "GB_LB") == "8" and L.SEGLEN == 8
    assert const(hpp, "GB_SEG") == "GB_THREADS / GB_LB" and L.NSEG == 256 // 8
    assert const(hpp, "GB_SEGLEN") == "GB_THREADS / GB_SEG"
    assert const(hpp, "GB_ROW") == "GB_THREADS + GB_SEG"
    assert const(hpp, "GB_TARGET_BLOCKS") == "2048" and L.TARGET_BLOCKS == 2048
    assert const(hpp, "GB_NONE") == "0x7fffff" and L.NONE == 0x7FFFFF
    assert const(hpp, "GB_FIXED_LDS") == "(size_t)GB_LB * GB_ROW * 8 + (size_t)GB_LB * GB_SEG * 8 + 2 * GB_THREADS * 4"
    fixed = 8 * (256 + 32) * 8 + 8 * 32 * 8 + 2 * 256 * 4
    assert const(hpp, "GF_ACC_BYTES") == "65536 - GB_FIXED_LDS" and L.GF_ACC_BYTES == 65536 - fixed == 43008
    assert const(hpp, "SF_BLOCK_LDS") == "80 * 1024"
    assert const(hpp, "SF_ACC_BYTES") == "SF_BLOCK_LDS - GB_FIXED_LDS" and L.SF_ACC_BYTES == 80 * 1024 - fixed == 59392
    assert const(lut, "GA_THREADS") == "256" and const(lut, "GA_PPT") == "8"
    assert const(lut, "GA_CHUNK") == "GA_THREADS * GA_PPT" and L.GA_CHUNK == 2048
    with open(os.path.join(CSRC, "lbl_rt.hpp")) as f:
        assert const(f.read(), "LBL_MAX_SZA") == "8" and L.MAX_SZA == 8


def test_the_grid_of_the_large_case():
    """1 049 421 points: 4100 tiles, 3 per block, 1367 blocks; the last block has 2 tiles, the second with 77 live lanes"""
    assert L.tile_grid(L.BIG_NWAV) == (3, 1367)
    assert -(-L.BIG_NWAV // L.TILE) == 4100 and 4100 - 1366 * 3 == 2 and L.BIG_NWAV % L.TILE == 77
    assert L.tile_grid(13567) == (1, 53)


def test_the_splits_of_the_production_depth():
    assert L.sw_cap(54) == 67 and L.sw_cap(3) == 928 and L.lw_max_cols(54) == 48
    for (ng, nsza), want in L.DEPTH_SPLITS.items():
        angles, ranges = L.sw_split(54, nsza, ng)
        assert angles == want and ranges == [(0, ng, True)]
    for a in range(1, 9):
        for nlay in (3, 4):
            assert L.sw_split(nlay, a, 7) == ([a], [(0, 7, True)])
    assert L.sw_split(3, 1, 300) == ([1], [(0, 300, True)]) and L.sw_split(3, 2, 16)[0] == [2]
    for nlay in (1, 2, 3, 4):
        assert L.lw_ranges(nlay, 300) == [(0, 300, True)]
    # the longwave tail batches of 3, 5, 7 and 1 rows, and a shortwave sweep without a tail
    assert [(2 * nlay + 1) % 8 for nlay in (1, 2, 3, 4)] == [3, 5, 7, 1]
    assert all((2 * 4) % (8 // a) == 0 for a in range(1, 9))
    assert [n for n in (10, 5) for lpb in (8, 4, 2) if n % lpb] == [10, 10, 5, 5, 5]


@pytest.mark.parametrize("case", L.SW_CASES, ids=lambda c: c.name)
def test_the_exact_inputs_are_exact(case):
    """Every addend is a multiple of 2^-9 below 2^20 and every sum stays below 2^41: integers below 2^50 in units of 2^-9,
    far below 2^53, so every partial sum in every order is exact.  Every spectral value has at most 24 significant bits."""
    inp = L.sw_inputs(case)
    assert np.all(inp.ssi == np.rint(inp.ssi)) and inp.ssi.min() >= 1 and inp.ssi.max() < 2 ** 20
    assert set(np.log2(inp.cos_sza).tolist()) <= {-float(e) for e in range(8)} and np.unique(inp.cos_sza).size == case.nsza
    if case.albedo:
        assert set(np.unique(inp.albedo).tolist()) <= {1.0, 0.5, 0.25}
    assert set(np.unique(inp.od).tolist()) <= {0.0, 1.0e6} and np.float32(1.0e6) == 1.0e6
    assert np.all(np.count_nonzero(inp.od, axis=0) == (inp.cut < case.nlay))
    assert np.all(np.diff(inp.wn) > 0)
    dn, up = L.sw_spectral(case)
    for f in (dn, up):
        units = f / L.UNIT
        assert np.all(units == np.rint(units)) and f.max() < 2 ** 20 and f.min() >= 0
        assert np.array_equal(f.astype(np.float32).astype(np.float64), f)
        m, _ = np.frexp(f)
        assert np.all(m * 2 ** 24 == np.rint(m * 2 ** 24))
    ref = L.sw_reference(case)
    assert max(ref.bb_dn.max(), ref.bb_up.max(), ref.dn.max(), ref.up.max()) < 2 ** 41
    # the integer sums against a plain sum of the exact spectral values (exact in any order, so numpy's is as good)
    col = np.where(inp.g < 0, inp.ng, inp.g)
    for f, per_g, bb in ((dn, ref.dn, ref.bb_dn), (up, ref.up, ref.bb_up)):
        assert np.array_equal(f.sum(2), bb)
        for c in np.unique(col[col < inp.ng])[:40]:
            assert np.array_equal(f[:, :, col == c].sum(2), per_g[:, :, c])
    if inp.ng >= 4 and case.kind != "cyclic":
        sp = L.case_spectrum(case)
        assert np.all(ref.dn[:, :, sp.empty_g] == 0) and np.count_nonzero(inp.g == sp.lone_g) == 1
