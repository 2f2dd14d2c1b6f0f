"""CPU checks of the inputs and references of test_cloud_edges_gpu.py (cloud_cases.py): the geometry comes from the library
(ecckd_cloud_geometry, a host-only entry), every case is classified from its inputs and its reference alone - interp path, tiles
per band, items of the last live thread, chunks per g point, blocks of boundary searches, grid passes - and no class the device
tests rely on is empty.  The sums of the exact cases are shown to be exact, their reference to agree with the restatement
test_cloud_gpu.py uses, and the general cases to keep that test's margin."""
import math

import numpy as np
import pytest

import cloud_cases as K


@pytest.fixture(scope="module")
def geo():
    import __graft_entry__ as g
    g.build()
    from ecckd_amd import api
    return api.cloud_geometry()          # without a context: grid_points of an MI355X


@pytest.fixture(scope="module")
def exact(geo):
    cases = K.exact_cases(geo)
    return [(c, K.partition_exact(c.ssi, c.rank, c.sv, c.begin, c.end, c.max_range)) for c in cases]


def test_geometry_is_the_librarys(geo):
    assert set(geo) == {"lds_knots", "scan_items", "scan_tile", "stats_chunk", "bounds_block", "grid_points"}
    assert geo["scan_tile"] == 256 * geo["scan_items"]            # a block of 256 threads
    assert geo["grid_points"] % 256 == 0 and geo["grid_points"] > 20000 + 7
    assert (geo["lds_knots"], geo["scan_items"], geo["stats_chunk"], geo["bounds_block"]) == (2048, 8, 8192, 64)
    assert geo["grid_points"] == 16 * 256 * 256                   # 256 compute units
    assert 2 * geo["lds_knots"] * 8 <= 64 * 1024                  # both staged arrays fit the LDS of a block


def test_exact_cases_are_exact_and_leave_no_g_point_empty(exact):
    for c, ref in exact:
        n = c.ssi.size
        assert c.rank.dtype == np.int32 and c.rank.size == n and c.sv.size == n
        u, v = c.ssi * K.SSI_UNIT, c.sv * K.SV_UNIT
        assert np.array_equal(u, np.rint(u)) and u.min() >= 0 and u.max() <= K.SSI_UNIT            # multiples of 2^-10 in [0, 1]
        assert np.array_equal(v, np.rint(v)) and v.min() >= 0 and v.max() < K.SV_UNIT              # of 2^-20 in [0, 1)
        assert n * K.SSI_UNIT < 2 ** 53 and n * K.SV_UNIT < 2 ** 53                                # any subset's sum is exact
        assert (c.ssi == 0).any() or c.ssi.size < 2000                                             # zeros included
        inside = K.band_index(n, c.begin, c.end) >= 0
        assert np.array_equal(c.rank[~inside], np.flatnonzero(~inside))
        for ib, ie in zip(c.begin, c.end):
            order = K.rank_order(c.rank, ib, ie)
            assert np.array_equal(np.sort(c.rank[ib:ie + 1]), np.arange(ib, ie + 1))
            for a in (c.ssi[order], c.sv[order]):
                assert np.cumsum(a)[-1] == np.cumsum(a[::-1])[-1] == math.fsum(a), c.name
            assert np.array_equal(np.cumsum(c.ssi[order]) * K.SSI_UNIT, np.cumsum(u[order].astype(np.int64)))
            assert c.ssi[ib:ie + 1].any()                                                          # a non-zero point per band
        assert min(ref["count"]) > 0, c.name
        assert sum(ref["count"]) == sum(e - b + 1 for b, e in zip(c.begin, c.end))                 # every band point in a g point
        assert sum(ref["n_g_points"]) <= c.capacity


def test_exact_reference_is_the_restatement(exact):
    """partition_exact against partition_numpy (the reference's loop as test_cloud_gpu.py restates it), bit for bit: on exact
    sums np.mean is fsum / count"""
    for c, ref in exact:
        if c.ssi.size > 100000:
            continue                     # (the restatement scans the whole array per g point)
        iband = K.band_index(c.ssi.size, c.begin, c.end)
        want, _ = K.partition_numpy(c.ssi, c.rank, c.sv, iband, len(c.begin), c.max_range)
        for k in ("n_g_points", "band_number", "rank1", "rank2"):
            assert list(ref[k]) == list(want[k]), (c.name, k)
        for k in ("error", "median"):
            assert np.array_equal(np.array(ref[k]).view(np.uint64), np.array(want[k]).view(np.uint64)), (c.name, k)


def test_exact_cases_hold_every_class(geo, exact):
    T, I, C, B = geo["scan_tile"], geo["scan_items"], geo["stats_chunk"], geo["bounds_block"]
    seen = set()
    per_case = {}
    for c, ref in exact:
        per_case[c.name] = K.partition_classes(c, ref, geo)
        seen |= per_case[c.name]
    classes = ["band of %d" % n for n in K.band_lengths(geo)]
    classes += ["tiles 1", "tiles 2", "tiles 3", "tiles 4", "last tile of %d" % (T - 1), "last tile of %d" % T, "last tile of 1",
                "last tile of 5"]
    # the last live thread of a tile: thread 0 with 1, I - 1 and I items, thread 1 with one, the last thread full and ragged
    classes += ["last thread 0 holds 1", "last thread 0 holds %d" % (I - 1), "last thread 0 holds %d" % I, "last thread 1 holds 1",
                "last thread 255 holds %d" % I, "last thread 255 holds %d" % (I - 1), "last thread 31 holds %d" % (I - 1),
                "last thread 31 holds %d" % I, "last thread 32 holds 1"]
    classes += ["adjacent bands", "gap between bands", "points before the first band", "points after the last band", "nband 1",
                "nband 13", "g point of 1", "g point of %d" % (C - 1), "g point of %d" % C, "g point of %d" % (C + 1), "chunks 1",
                "chunks 2", "chunks 3", "last chunk of 1", "queries %d" % (B - 1), "queries %d" % B, "queries %d" % (B + 1),
                "query blocks 1", "query blocks 2", "query blocks 3", "ng == capacity", "constant band of 2 tiles", "perm stable",
                "perm identity", "perm reversed", "grid passes 1", "grid passes 2", "band astride the first grid pass",
                "band in the second grid pass", "g points per band 1", "g points per band 2", "g points per band 3",
                "zero irradiance first in rank order"]
    assert all(k in seen for k in classes), [k for k in classes if k not in seen]
    # the named cases are what they are named for
    assert {"chunks 3", "last chunk of 1", "g points per band 1"} <= per_case["long/1-g-point"]
    assert {"g points per band 2", "nband 1", "band of %d" % (2 * C + 1)} <= per_case["long/2-g-point"]
    assert {"g point of %d" % (C - 1), "g point of %d" % C, "g point of %d" % (C + 1)} <= per_case["chunk-edges"]
    for nq in (B - 1, B, B + 1):
        assert "queries %d" % nq in per_case["bounds/%d" % nq]
    assert "query blocks 1" in per_case["bounds/%d" % B] and "query blocks 2" in per_case["bounds/%d" % (B + 1)]
    assert "ng == capacity" in per_case["capacity"]
    for perm in ("identity", "reversed"):
        assert {"grid passes 2", "band astride the first grid pass", "band in the second grid pass"} <= per_case["grid/" + perm]
        assert [c for c, _ in exact if c.name == "grid/" + perm][0].ssi.size == geo["grid_points"] + 257
    for perm in K.PERMS:
        for mr in K.EXACT_RANGES:
            assert "nband 13" in per_case["thirteen/%s/%g" % (perm, mr)] and "nband 1" in per_case["one-band/%s/%g" % (perm, mr)]
    # bands of fewer than 256 points: one g point at every range
    for c, ref in exact:
        if c.name.startswith("thirteen"):
            assert [ng for ng, b, e in zip(ref["n_g_points"], c.begin, c.end) if e - b + 1 < 256] == [1] * 5
            assert min(ng for ng, b, e in zip(ref["n_g_points"], c.begin, c.end) if e - b + 1 >= 256) >= 3
    # a permutation is what its name says
    by_name = {c.name: c for c, _ in exact}
    c = by_name["thirteen/identity/0.05"]
    assert np.array_equal(c.rank, np.arange(c.rank.size))
    c = by_name["thirteen/reversed/0.05"]
    assert all(np.array_equal(c.rank[b:e + 1], np.arange(e, b - 1, -1)) for b, e in zip(c.begin, c.end))
    c = by_name["thirteen/stable/0.05"]
    assert all(np.all(np.diff(c.sv[K.rank_order(c.rank, b, e)]) >= 0) for b, e in zip(c.begin, c.end))
    assert not np.array_equal(c.rank, np.arange(c.rank.size))


def test_general_cases_keep_the_margin(geo):
    cases = K.general_cases(geo)
    assert [c.end[0] - c.begin[0] + 1 for c in cases] == K.band_lengths(geo)
    several = 0
    for c in cases:
        n = c.ssi.size
        want, margin = K.partition_numpy(c.ssi, c.rank, c.sv, K.band_index(n, c.begin, c.end), 1, c.max_range)
        assert margin > K.GENERAL_MARGIN, (c.name, margin)
        assert c.begin[0] > 0 and c.end[0] < n - 1 and np.all(c.ssi >= 0)
        u = c.ssi * K.SSI_UNIT
        assert not np.array_equal(u, np.rint(u))                                   # not dyadic
        several += want["n_g_points"][0] > 1
        items = geo["scan_items"]
        if c.end[0] - c.begin[0] + 1 >= 255:
            # a whole thread of the scan adds nothing (its items, consecutive in rank order, are all zero), its neighbours do
            w = c.ssi[K.rank_order(c.rank, c.begin[0], c.end[0])]
            idle = (w[:w.size // items * items].reshape(-1, items) == 0).all(axis=1)
            assert idle.any() and not idle.all()
    assert several >= 9


def test_sorting_cases_hold_every_class(geo):
    L, G = geo["lds_knots"], geo["grid_points"]
    cases = K.sorting_cases(geo)
    assert [c.x.size for c in cases] == [2, 3, 255, 256, 257, L - 1, L, L + 1, 2 * L + 4]
    seen = set()
    for c in cases:
        n = c.x.size
        assert np.all(np.diff(c.x) > 0) and np.all(c.g > 0)
        assert (c.ssa == 1.0).any() and (c.ssa == 0.0).any() and (n < 4 or ((c.ssa > 0) & (c.ssa < 1)).any())
        ref = K.abs_inf_numpy(c.x, c.ssa, c.g, c.points)
        assert np.isfinite(ref).all()
        on_knot = K.abs_inf_numpy(c.x, c.ssa, c.g, c.x)
        assert np.all(on_knot[c.ssa == 1.0] == 0.0) and np.all(on_knot[c.ssa == 0.0] == 1.0)
        assert c.points.size == 4 * n + 1 and np.unique(c.points).size == c.points.size
        sizes = K.sorting_sizes(geo, c.points.size)
        assert set(sizes) >= {1, 255, 256, 257, G - 1, G, G + 257, c.points.size}
        per = set()
        for nwav in sizes:
            per |= K.sorting_classes(c, nwav, geo)
        assert {"every segment", "every knot", "below the first knot", "above the last knot", "grid passes 1", "grid passes 2"} <= per
        assert n == 2 or "neighbouring lanes in different segments" in per
        seen |= per
    classes = ["interp lds", "interp hbm", "clamp n - 2 == 0", "knots %d" % L, "knots %d" % (L + 1), "staging rounds 1, last of 2",
               "staging rounds 1, last of 255", "staging rounds 1, last of 256", "staging rounds 2, last of 1",
               "staging rounds %d, last of 256" % (L // 256), "points 1", "points %d" % (G - 1), "points %d" % G, "points %d" % (G + 257)]
    assert all(k in seen for k in classes), [k for k in classes if k not in seen]
    assert "interp lds" in K.sorting_classes(cases[6], 1, geo) and "interp hbm" in K.sorting_classes(cases[7], 1, geo)


def test_nan_knot_case_poisons_two_segments_only():
    c = K.nan_knot_case()
    with np.errstate(invalid="ignore"):
        ref = K.abs_inf_numpy(c.x, c.ssa, c.g, c.points)
    bad = np.isnan(ref)
    assert bad.any() and not np.isinf(ref).any()
    assert np.array_equal(bad, (c.points >= c.x[4]) & (c.points < c.x[6]))
    assert np.isfinite(ref[c.points == c.x[6]]).all() and (c.points == c.x[6]).sum() == 1
