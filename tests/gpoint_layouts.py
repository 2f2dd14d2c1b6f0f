"""g-point maps built from TILE LAYOUTS, exact shortwave inputs and smooth longwave inputs for the tests of the tile binner of
csrc/gpoint_bin.hpp (test_gpoint_bin_layouts.py on the CPU, test_gpoint_bin_edges_gpu.py on the device).  numpy only.

The binner ranks the 256 points of a tile by (column, lane) and adds every row of fluxes in segments of 8 ranks.  What it
does is decided by the ranked keys of the tile alone, so a test that wants a certain branch designs the RANKED tile: a
layout is the list of (column, count) runs of one tile in rank order - columns ascending, then the points without a g point
(column -1), counts summing to the tile's live lanes.  tile_g() hands the lanes of the tile to those runs: through a seeded
permutation (the natural order is scrambled on purpose; the order inside a column is lane order, so every assignment ranks to
the same layout) or through the identity.  A spectrum is the concatenation of tiles.

The numbers of the kernels that the layouts are written for are repeated here (test_gpoint_bin_layouts.py reads them out of the
sources and fails when they differ)."""
import functools
from collections import namedtuple

import numpy as np

TILE = 256                 # GB_THREADS: points of a tile
SEGLEN = 8                 # GB_SEGLEN: ranks of a segment (= GB_LB, rows of a batch)
NSEG = 32                  # GB_SEG: segments of a tile
TARGET_BLOCKS = 2048       # GB_TARGET_BLOCKS
GF_ACC_BYTES = 43008       # the longwave kernel's accumulator budget
SF_ACC_BYTES = 59392       # the shortwave kernel's
GA_CHUNK = 2048            # sorted positions per block of ecckd_gmap_sum_rows
MAX_SZA = 8                # LBL_MAX_SZA
NONE = 0x7FFFFF            # GB_NONE


# ------------------------------------------------------------------------------------------------ what the host code decides
def tile_grid(nwav):
    """(tiles per block, blocks) of a spectrum: tile_grid() of gpoint_bin.hpp"""
    ntiles = -(-nwav // TILE)
    tpb = max(1, -(-ntiles // TARGET_BLOCKS))
    return tpb, -(-ntiles // tpb)


def column_ranges(ng, max_cols):
    """[(g0, gcount, with_none)] of bin_column_ranges(): the first pass also bins the points without a g point"""
    out, g0, npass = [], 0, 0
    while npass == 0 or g0 < ng:
        with_none = npass == 0
        gcount = min(ng - g0, max_cols - (1 if with_none else 0))
        out.append((g0, gcount, with_none))
        g0 += gcount
        npass += 1
    return out


def lw_max_cols(nlay):
    return GF_ACC_BYTES // (16 * (nlay + 1))


def sw_cap(nlay):
    return SF_ACC_BYTES // (16 * (nlay + 1))


def sw_split(nlay, nsza, ng):
    """(angles of every launch group, column ranges of each) by the formula in the header of lbl_gpoint_fluxes_sw.hip"""
    cap, out_cols = sw_cap(nlay), ng + 1
    if cap >= out_cols:
        amax = min(nsza, MAX_SZA, cap // out_cols)
        nl = -(-nsza // amax)
        per, cols = -(-nsza // nl), out_cols
    else:
        per, cols = 1, cap
    angles, a0 = [], 0
    while a0 < nsza:
        angles.append(min(per, nsza - a0))
        a0 += angles[-1]
    return angles, column_ranges(ng, cols)


def lw_ranges(nlay, ng):
    return column_ranges(ng, lw_max_cols(nlay))


# ------------------------------------------------------------------------------------------------------------- tile layouts
def cycle_counts(total, longest=9):
    """run lengths cycling 1..longest that sum to `total`"""
    out, k = [], 0
    while sum(out) < total:
        out.append(min(k % longest + 1, total - sum(out)))
        k += 1
    return out


def full_tile_layouts(with_256=True):
    """[(name, counts of the columns in rank order, points without a g point)] of a tile with 256 live lanes"""
    out = [("one_chain", [256], 0),
           ("32x8", [8] * 32, 0)]
    out += [("break_at_%d" % r, [r] + [8] * 31 + [8 - r], 0) for r in range(1, 8)]
    out += [("3_250_3", [3, 250, 3], 0),
            ("8_240_8", [8, 240, 8], 0),
            ("5_123_128", [5, 123, 128], 0),
            ("3_5_248", [3, 5, 248], 0),          # a column that ends on its segment's last rank without a chain
            ("cycle_1_9", cycle_counts(256), 0),
            # chains of 1, 2, 3 and 25 parked pieces, each begun at offset 4 of a segment and ended at offset 3 of another
            # (the last one inside segment 31)
            ("chains_end_inside", [4, 8, 16, 24, 200, 4], 0),
            # chains of 1, 2, 3 and 22 parked pieces that end on a segment's last rank (the last one on the tile's); all but
            # the first begin on a segment's first rank: their collector has no break
            ("chains_end_on_last_rank", [4, 12, 24, 32, 184], 0),
            # chains of 2 and of 1 parked pieces that reach segment 31: to its last rank, and to its offset 3
            ("tail_236_20", [236, 20], 0),
            ("tail_244_12", [244, 12], 0),
            ("tail_236_16_4", [236, 16, 4], 0),
            ("tail_244_8_4", [244, 8, 4], 0),
            ("none_1", [8] * 31 + [7], 1),
            ("none_8", [3, 245], 8),
            ("none_9", [5] + [8] * 30 + [2], 9),
            ("none_100", [156], 100),
            ("none_100_cycle", cycle_counts(156), 100),
            ("none_only", [], 256)]
    if with_256:
        out.append(("256x1", [1] * 256, 0))
    for name, counts, none in out:
        assert sum(counts) + none == TILE and all(c > 0 for c in counts), name
    return out


def fit(counts, ncols):
    """a layout for a map with fewer columns than it has runs: the first ncols - 1 runs, then one run of the rest"""
    if len(counts) <= ncols:
        return list(counts)
    return list(counts[:ncols - 1]) + [sum(counts[ncols - 1:])]


def tile_g(runs, perm=None):
    """The g_point values of one tile in natural (lane) order.  runs: (column, count) in rank order; perm: which lanes each
    run gets (a permutation of the live lanes, consumed run by run), None for the identity."""
    cols = [c for c, _ in runs if c >= 0]
    assert cols == sorted(set(cols)), "columns ascend in rank order"
    assert all(c >= 0 for c, _ in runs[:-1]), "the points without a g point rank last"
    live = sum(n for _, n in runs)
    assert 0 < live <= TILE
    g = np.empty(live, dtype=np.int32)
    lanes = np.arange(live) if perm is None else np.asarray(perm)
    assert sorted(lanes.tolist()) == list(range(live))
    at = 0
    for c, n in runs:
        g[lanes[at:at + n]] = c
        at += n
    return g


Spectrum = namedtuple("Spectrum", "g ng nwav tiles empty_g lone_g")


@functools.lru_cache(maxsize=None)
def spectrum(ng, last_live=77, ranges=None, seed=0):
    """The layout spectrum of a map with ng g points: every layout of full_tile_layouts() (fit() to the columns there are)
    twice - lanes permuted, lanes in order - with columns drawn from all g points; with `ranges` ((g0, gcount), ...) once more
    per range with columns of that range only (such a tile is wholly GB_NONE in the other launches); then a last tile of
    `last_live` lanes.  From 4 g points on, g point 1 owns no wavenumber and g point ng - 2 owns one, in the last tile.
    -> Spectrum; .tiles is the list of (name, runs) in order."""
    rng = np.random.default_rng(20250 + 7 * ng + last_live + seed)
    empty_g, lone_g = (1, ng - 2) if ng >= 4 else (None, None)
    pools = [[c for c in range(ng) if c not in (empty_g, lone_g)]]
    for g0, gcount in (ranges or ()):
        pool = [c for c in range(g0, g0 + gcount) if c not in (empty_g, lone_g)]
        if pool:
            pools.append(pool)
    tiles, parts = [], []

    def add(name, runs, permute):
        live = sum(n for _, n in runs)
        parts.append(tile_g(runs, rng.permutation(live) if permute else None))
        tiles.append((name, runs))

    for ip, pool in enumerate(pools):
        for name, counts, none in full_tile_layouts(with_256=len(pool) >= 256):
            for permute in (True, False):
                c = fit(counts, len(pool))
                cols = sorted(rng.choice(pool, size=len(c), replace=False).tolist())
                runs = list(zip(cols, c)) + ([(-1, none)] if none else [])
                add("%s/pool%d/%s" % (name, ip, "perm" if permute else "id"), runs, permute)
    # the last tile: a few columns, one point without a g point where there is room, and the lone g point's only wavenumber
    rest = last_live - (1 if lone_g is not None else 0)
    none = 1 if rest >= 8 else 0
    below = [x for x in pools[0] if lone_g is None or x < lone_g]
    c = fit(cycle_counts(rest - none), len(below)) if rest - none > 0 else []
    cols = sorted(rng.choice(below, size=len(c), replace=False).tolist())
    runs = list(zip(cols, c)) + ([(lone_g, 1)] if lone_g is not None else []) + ([(-1, none)] if none else [])
    add("last_%d" % last_live, runs, True)
    g = np.concatenate(parts)
    return Spectrum(g, ng, g.size, tiles, empty_g, lone_g)


def cyclic_spectrum(ng, nwav):
    """the full tiles of spectrum(ng) repeated cyclically up to nwav points"""
    base = spectrum(ng, last_live=TILE)
    return Spectrum(np.resize(base.g, nwav), ng, nwav, None, base.empty_g, None)


def tiny_spectrum(nwav):
    """nwav = 1, 255, 256, 257 with two g points: shorter than a tile, one lane short, exactly a tile, one lane over"""
    rng = np.random.default_rng(nwav)
    g = rng.integers(-1, 2, size=nwav).astype(np.int32)
    g[0] = 1
    return Spectrum(g, 2, nwav, None, None, None)


# ---------------------------------------------------------------------------------- the binner's decisions, restated in numpy
def launch_keys(g, g0, gcount, with_none):
    """the ranked keys [ntiles][256] of one launch: tile_key() and the order of tile_rank() (dead lanes: GB_NONE)"""
    ntiles = -(-g.size // TILE)
    key = np.full(ntiles * TILE, NONE, dtype=np.int64)
    inside = (g >= g0) & (g < g0 + gcount)
    k = np.where(inside, g - g0, NONE)
    if with_none:
        k = np.where(g < 0, gcount, k)
    key[:g.size] = k
    return np.sort(key.reshape(ntiles, TILE), axis=1, kind="stable")


def segment_branches(keys):
    """per (tile, segment): cont_in, brk == 0, collects, tail is GB_NONE - what tile_pieces() hands reduce_batch()"""
    k = keys.reshape(keys.shape[0], NSEG, SEGLEN)
    brk0 = np.all(k[:, :, 1:] == k[:, :, :-1], axis=2)
    cont_in = np.zeros(k.shape[:2], dtype=bool)
    cont_in[:, 1:] = k[:, 1:, 0] == k[:, :-1, -1]
    tail = k[:, :, -1]
    nxt = np.zeros(k.shape[:2], dtype=bool)
    nxt[:, :-1] = k[:, 1:, 0] == tail[:, :-1]
    collects = nxt & (tail != NONE) & ~(brk0 & cont_in)
    return cont_in, brk0, collects, tail == NONE


def length_class(n):
    return "1" if n == 1 else "2" if n == 2 else "31" if n == 31 else "3..30"


def chains(keys):
    """per collector: (class of the number of parked pieces it adds, the chain ends inside a segment, it reaches segment 31) -
    the collector loop of reduce_batch(), which stops at a first key that differs, after a last key that differs, or at the
    tile's end"""
    k = keys.reshape(keys.shape[0], NSEG, SEGLEN)
    _, _, collects, _ = segment_branches(keys)
    out = []
    for t, seg in zip(*np.nonzero(collects)):
        tail, n, inside, s2 = k[t, seg, -1], 0, False, seg + 1
        while s2 < NSEG and k[t, s2, 0] == tail:
            n += 1
            if k[t, s2, -1] != tail:
                inside = True
                break
            s2 += 1
        out.append((length_class(n), inside, seg + n == NSEG - 1))
    return out


# the combinations that can occur.  A segment: collects needs a tail that is a column and not (no break and continued) - such
# a segment is the middle of somebody else's chain.
SEGMENT_COMBINATIONS = {(cont_in, brk0, collects, tail_none)
                        for cont_in in (False, True) for brk0 in (False, True) for collects in (False, True)
                        for tail_none in (False, True)
                        if not (collects and (tail_none or (brk0 and cont_in)))}
# A chain: 31 parked pieces start in segment 0 and so reach segment 31.
CHAIN_COMBINATIONS = {(cls, inside, reaches) for cls in ("1", "2", "3..30", "31") for inside in (False, True)
                      for reaches in (False, True) if not (cls == "31" and not reaches)}


def reached(g, launches):
    """(segment combinations, chain combinations, launches with a tile that is GB_NONE only) of a map over `launches`"""
    segs, chs, none_tiles = set(), set(), 0
    for g0, gcount, with_none in launches:
        keys = launch_keys(g, g0, gcount, with_none)
        a = segment_branches(keys)
        segs |= set(zip(*(x.ravel().tolist() for x in a)))
        chs |= set(chains(keys))
        none_tiles += bool(np.any(np.all(keys == NONE, axis=1)))
    return segs, chs, none_tiles


# ------------------------------------------------------------------------------------------ exact shortwave inputs and sums
COS_EXP = (0, 3, 6, 1, 4, 7, 2, 5)           # cos_sza[s] = 2^-COS_EXP[s]: all different, so a swap of angles shows
UNIT = 2.0 ** -9                              # every flux is a multiple of it: 2^-7 (angle) x 2^-2 (albedo) x an integer

SwCase = namedtuple("SwCase", "name kind nlay ng nsza albedo dtype last_live nwav")


def sw_case(name, kind, nlay, ng, nsza, albedo=True, dtype="float32", last_live=77, nwav=0):
    return SwCase(name, kind, nlay, ng, nsza, albedo, dtype, last_live, nwav)


def case_spectrum(case):
    if case.kind == "layouts":
        return spectrum(case.ng, case.last_live)
    if case.kind == "ranges":
        return spectrum(case.ng, case.last_live, tuple((g0, n) for g0, n, _ in sw_split(case.nlay, case.nsza, case.ng)[1]))
    if case.kind == "lw_ranges":
        return spectrum(case.ng, case.last_live, tuple((g0, n) for g0, n, _ in lw_ranges(case.nlay, case.ng)))
    if case.kind == "cyclic":
        return cyclic_spectrum(case.ng, case.nwav)
    assert case.kind == "tiny"
    return tiny_spectrum(case.nwav)


BIG_NWAV = 1049421          # 4100 tiles, 3 per block, 1367 blocks; the last block has 2 tiles, the second with 77 live lanes

LAYOUT_CASES = [sw_case("layouts-%d-%s-%s" % (live, "alb" if alb else "noalb", dt), "layouts", 3, 300, 1, alb, dt, live)
                for live in (1, 7, 8, 9, 255) for alb in (False, True) for dt in ("float32", "float64")]
ANGLE_CASES = [sw_case("A%d-nlay%d-%s" % (a, nlay, "alb" if alb else "noalb"), "layouts", nlay, 7, a, alb)
               for nlay in (3, 4) for alb in (True, False) for a in range(1, 9)]
# (ng, nsza) -> the angles of its launches at 54 layers
DEPTH_SPLITS = {(7, 8): [8], (8, 7): [7], (10, 6): [6], (12, 5): [5], (15, 7): [4, 3], (32, 5): [2, 2, 1]}
DEPTH_CASES = [sw_case("nlay54-ng%d-nsza%d" % k, "layouts", 54, k[0], k[1]) for k in DEPTH_SPLITS]
# ng -> the g points of its launches at 54 layers (67 column-angles per launch; the first launch keeps one for "none")
RANGE_SPLITS = {66: [66], 67: [66, 1], 133: [66, 67], 134: [66, 67, 1]}
RANGE_CASES = [sw_case("nlay54-ng%d" % ng, "ranges", 54, ng, 2) for ng in RANGE_SPLITS]
BIG_CASE = sw_case("several-tiles-per-block", "cyclic", 3, 16, 2, nwav=BIG_NWAV)
TINY_CASES = [sw_case("nwav%d" % n, "tiny", 3, 2, 2, nwav=n) for n in (1, 255, 256, 257)]
SW_CASES = LAYOUT_CASES + ANGLE_CASES + DEPTH_CASES + RANGE_CASES + [BIG_CASE] + TINY_CASES

SwInputs = namedtuple("SwInputs", "g ng nwav wn dwn cos_sza ssi albedo od cut")


@functools.lru_cache(maxsize=4)
def sw_inputs(case):
    """Exact inputs: ssi an integer in [1, 2^20), cos_sza a power of two, albedo 1, 1/2 or 1/4, optical depth 0 but for one
    layer cut[j] per wavenumber (nlay: none) that holds 1e6.  Then every flux is cos_sza x albedo x ssi or exactly 0."""
    sp = case_spectrum(case)
    rng = np.random.default_rng(1000003 * case.nlay + 1009 * case.ng + 31 * case.nsza + sp.nwav)
    ssi = rng.integers(1, 2 ** 20, size=sp.nwav).astype(np.float64)
    albedo = (0.5 ** rng.integers(0, 3, size=sp.nwav)) if case.albedo else None
    cut = rng.integers(0, case.nlay + 1, size=sp.nwav)
    od = np.zeros((case.nlay, sp.nwav), dtype=case.dtype)
    at = np.nonzero(cut < case.nlay)[0]
    od[cut[at], at] = 1.0e6
    cos_sza = np.array([2.0 ** -e for e in COS_EXP[:case.nsza]])
    wn = np.linspace(2000.0, 20000.0, sp.nwav) if sp.nwav > 1 else np.array([2000.0])
    dwn = np.full(sp.nwav, 18000.0 / max(sp.nwav - 1, 1))
    return SwInputs(sp.g, sp.ng, sp.nwav, wn, dwn, cos_sza, ssi, albedo, od, cut)


def sw_integer_sums(inp, nlay):
    """Per level and column (g points, then the points without one) in integers: dn = the sum of ssi over the points whose
    opaque layer is not above the level; up = the sum of 4 x albedo x ssi over the transparent points, at every level."""
    col = np.where(inp.g < 0, inp.ng, inp.g).astype(np.int64)
    w = inp.ssi.astype(np.int64)
    assert np.array_equal(w.astype(np.float64), inp.ssi)
    dn = np.zeros((nlay + 1, inp.ng + 1), dtype=np.int64)
    up4 = np.zeros((nlay + 1, inp.ng + 1), dtype=np.int64)
    order = np.argsort(col, kind="stable")
    edges = np.searchsorted(col[order], np.arange(inp.ng + 2))

    def per_column(values):                       # int64 per point -> int64 per column
        v = np.concatenate([[0], values[order].cumsum()])
        return v[edges[1:]] - v[edges[:-1]]

    for lev in range(nlay + 1):
        dn[lev] = per_column(np.where(inp.cut >= lev, w, 0))
    if inp.albedo is not None:
        a4 = np.rint(inp.albedo * 4.0).astype(np.int64)
        assert np.array_equal(a4 / 4.0, inp.albedo)
        up4[:] = per_column(np.where(inp.cut == nlay, a4 * w, 0))
    return dn, up4


SwReference = namedtuple("SwReference", "dn up bb_dn bb_up")


@functools.lru_cache(maxsize=4)
def sw_reference(case):
    """(dn, up) [nsza][nlay + 1][ng] and (bb_dn, bb_up) [nsza][nlay + 1]: integer sums times powers of two, exact in double"""
    inp = sw_inputs(case)
    dn, up4 = sw_integer_sums(inp, case.nlay)
    assert int(dn.sum(1).max()) < 2 ** 41 and int(up4.sum(1).max()) < 2 ** 43  # sums below 2^41: below 2^50 units of 2^-9
    mu = inp.cos_sza[:, None, None]
    fdn, fup = mu * dn.astype(np.float64), mu * (up4.astype(np.float64) * 0.25)
    bdn = inp.cos_sza[:, None] * dn.sum(1).astype(np.float64)
    bup = inp.cos_sza[:, None] * (up4.sum(1).astype(np.float64) * 0.25)
    return SwReference(fdn[:, :, :inp.ng], fup[:, :, :inp.ng], bdn, bup)


def sw_spectral(case):
    """the exact spectral fluxes (dn, up) [nsza][nlay + 1][nwav] in double; every value has at most 20 significant bits"""
    inp = sw_inputs(case)
    lev = np.arange(case.nlay + 1)[:, None]
    dn = inp.cos_sza[:, None, None] * np.where(inp.cut[None, :] >= lev, inp.ssi[None, :], 0.0)[None]
    if inp.albedo is None:
        return dn, np.zeros_like(dn)
    up1 = np.where(inp.cut == case.nlay, inp.albedo * inp.ssi, 0.0)
    up = inp.cos_sza[:, None, None] * np.broadcast_to(up1, (case.nlay + 1, inp.nwav))[None]
    return dn, np.ascontiguousarray(up)


# ------------------------------------------------------------------------------------------------- smooth longwave inputs
LwCase = namedtuple("LwCase", "name kind nlay ng dtype last_live nwav")
LW_SMALL_CASES = [LwCase("nlay%d-%s" % (nlay, dt), "layouts", nlay, 300, dt, 77, 0)
                  for nlay, dt in ((1, "float32"), (2, "float64"), (3, "float32"), (4, "float64"))]
# ng -> the g points of its launches at 54 layers (48 columns per launch; the first launch keeps one for "none")
LW_RANGE_SPLITS = {47: [47], 48: [47, 1], 95: [47, 48], 96: [47, 48, 1]}
LW_RANGE_CASES = [LwCase("nlay54-ng%d" % ng, "lw_ranges", 54, ng, "float32" if ng % 2 else "float64", 77, 0) for ng in LW_RANGE_SPLITS]
LW_BIG_CASE = LwCase("several-tiles-per-block", "cyclic", 3, 16, "float32", 77, BIG_NWAV)
LW_CASES = LW_SMALL_CASES + LW_RANGE_CASES + [LW_BIG_CASE]

LwInputs = namedtuple("LwInputs", "g ng nwav wn dwn t_hl od")


@functools.lru_cache(maxsize=2)
def lw_inputs(case):
    """600-700 cm-1, optical depths of 0.1 to 1 per layer that vary slowly with the wavenumber: every point's flux is within
    a small factor of its neighbours', so one point lost or misplaced among the N of a column moves its sum by about 1 / N."""
    sp = case_spectrum(case)
    wn = np.linspace(600.0, 700.0, sp.nwav)
    dwn = np.full(sp.nwav, 100.0 / (sp.nwav - 1))
    lay = np.arange(case.nlay)[:, None]
    od = (0.55 + 0.45 * np.sin(0.07 * wn[None, :] + 0.9 * lay)).astype(case.dtype)
    t_hl = np.linspace(215.0, 292.0, case.nlay + 1)
    return LwInputs(sp.g, sp.ng, sp.nwav, wn, dwn, t_hl, od)
