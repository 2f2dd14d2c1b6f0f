"""CPU checks of the inputs and references of test_index_edges_gpu.py (index_cases.py): the geometry comes from the library
(ecckd_index_geometry, a host-only entry), every case is classified from its inputs and its reference alone - which branch of
the sort's host code it takes, how many rounds the row scan makes, which stage of the median kernel holds the answer - and no
class the device tests rely on is empty.  The restatement of the median loop is checked against the oracle on every case."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import index_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def geo():
    import __graft_entry__ as g
    g.build()
    from ecckd_amd import api
    return api.index_geometry()


def test_geometry_is_the_librarys(geo):
    T, W = geo["sort_keys_per_tile"], geo["sort_keys_per_wave"]
    assert T == 4 * W and W % 64 == 0                 # a block of four waves, chunks of 64 consecutive keys
    if "ECCKD_SORT_ITEMS" not in os.environ:
        assert (T, W) == (3840, 960)                  # 15 keys per thread
    assert geo["sort_scan_round_tiles"] == 2048 and geo["sort_max_one_sort_bands"] == 59
    assert geo["median_tile"] == 256 and geo["max_groups"] == 32
    # the A/B knob is honoured: the edges of the variant tests are that variant's own
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\nfrom ecckd_amd import api\n"
                          "g = api.index_geometry(); print(g['sort_keys_per_tile'], g['sort_keys_per_wave'])" % ROOT],
                         env=dict(os.environ, ECCKD_SORT_ITEMS="8"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["2048", "512"], out.stdout + out.stderr


def test_one_band_cases_reach_both_single_band_paths(geo):
    T, W, B = geo["sort_keys_per_tile"], geo["sort_keys_per_wave"], geo["sort_max_one_sort_bands"]
    lengths = K.one_band_lengths(T, W)
    assert set(lengths) >= {1, 2, 63, 64, 65, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1}
    cases = K.one_band_cases(T, W)
    paths = Counter()
    for c in cases:
        n = c.key.size
        path = K.sort_path(n, c.begin, c.end, B)
        paths[path] += 1
        m = c.end[0] - c.begin[0] + 1
        assert m in lengths
        if c.name.startswith("whole"):
            assert path == "per_band_whole" and m == n
        else:
            assert path == "per_band_identity" and c.begin[0] % 64 and c.end[0] < n - 1     # unaligned, points on both sides
        rank, ordered = K.ref_band_sort(c.key, c.begin, c.end)
        assert np.array_equal(np.sort(rank), np.arange(n)) and np.array_equal(rank[ordered], np.arange(n))
    assert paths == {"per_band_whole": len(lengths), "per_band_identity": len(lengths)}
    # tiles of the band: one ragged, exactly one, one and a point, ... three
    assert sorted({K.sort_tiles(m, T) for m in lengths}) == [1, 2, 3]


@pytest.mark.parametrize("b", range(8))
def test_byte_keys_differ_in_one_byte_only(geo, b):
    T = geo["sort_keys_per_tile"]
    key = K.byte_keys(b, T)
    bits = key.view(np.uint64)
    assert key.size > T and not np.isnan(key).any() and not np.isinf(key).any() and np.all(key != 0.0)
    others = ~(np.uint64(0xFF) << np.uint64(8 * b)) & np.uint64(0x7FFFFFFFFFFFFFFF)
    assert np.unique(bits & others).size == 1                               # every other bit (the sign apart) is fixed
    digit = ((bits >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.int64)
    sign = (bits >> np.uint64(63)).astype(np.int64)
    for s in (0, 1):
        counts = np.bincount(digit[sign == s], minlength=256)
        if b == 7:
            assert np.all(counts[128 * s:128 * s + 128] >= 8)               # (the sign is the byte's top bit)
        else:
            assert np.all(counts >= 4)
    order = K.ref_argsort(key)
    assert np.all(np.diff(key[order]) >= 0) and np.any(np.diff(order) < 0)
    ties = np.diff(key[order]) == 0
    assert ties.sum() > key.size // 2 and np.all(np.diff(order)[ties] > 0)  # stable inside every value's group


def test_special_keys_hold_every_special(geo):
    key = K.special_keys(3 * geo["sort_keys_per_tile"] + 5, 40)
    bits = key.view(np.uint64)
    for v in K.SPECIALS:
        assert np.count_nonzero(bits == np.float64(v).view(np.uint64)) >= 3, v
    nan = np.isnan(key)
    assert np.count_nonzero(nan & (bits >> np.uint64(63) == 1)) >= 3 and np.count_nonzero(nan & (bits >> np.uint64(63) == 0)) >= 3
    assert np.unique(bits[nan]).size >= 4                                   # payloads (a copy may quieten a signalling one)
    assert np.count_nonzero(key == -0.5) > key.size // 5
    order = K.ref_argsort(key)
    nn = int(nan.sum())
    assert np.array_equal(order[-nn:], np.flatnonzero(nan))                 # NaNs last, in index order
    head = key[order[:-nn]]
    assert np.all(head[1:] >= head[:-1]) and head[0] == -np.inf and head[-1] == np.inf
    zeros = order[:-nn][head == 0.0]
    assert np.all(np.diff(zeros) > 0) and np.signbit(key[zeros]).any() and not np.signbit(key[zeros]).all()


def test_band_lists_reach_the_one_sort_and_the_fall_backs(geo):
    T, B = geo["sort_keys_per_tile"], geo["sort_max_one_sort_bands"]
    n = K.band_list_length(T)
    lists = K.band_lists(T, B)
    want = {"two-gaps": (2, "one_sort"), "two-adjacent": (2, "one_sort"), "thirteen": (13, "one_sort"),
            "most-one-sort": (B, "one_sort"), "most-one-sort-flush": (B, "one_sort"), "one-too-many": (B + 1, "per_band_identity"),
            "descending": (13, "per_band_identity")}
    assert set(lists) == set(want)
    seen = Counter()
    for name, (begin, end) in lists.items():
        assert (len(begin), K.sort_path(n, begin, end, B)) == want[name], name
        live = sorted((b, e) for b, e in zip(begin, end) if e >= b)
        assert live[0][0] >= 0 and live[-1][1] <= n - 1
        assert all(live[i][0] > live[i - 1][1] for i in range(1, len(live)))        # disjoint in every list
        seen["leading gap" if live[0][0] > 0 else "no leading gap"] += 1
        seen["trailing gap" if live[-1][1] < n - 1 else "no trailing gap"] += 1
        seen["empty band in the middle"] += any(e < b for b, e in list(zip(begin, end))[1:-1])
        seen["one-point band"] += any(e == b for b, e in live)
        seen["one-point gap"] += any(live[i][0] - live[i - 1][1] == 2 for i in range(1, len(live)))
        seen["adjacent bands"] += any(live[i][0] - live[i - 1][1] == 1 for i in range(1, len(live)))
        for _, e in live:
            for d, label in ((T - 1, "end on T-1"), (0, "end on T"), (1, "end on T+1")):
                seen[label] += e % T == d
        if K.sort_path(n, begin, end, B) == "one_sort":
            segments = len(live) + sum(live[i][0] - live[i - 1][1] > 1 for i in range(1, len(live))) + (live[0][0] > 0) + (live[-1][1] < n - 1)
            seen["full segment table"] += segments == 2 * B + 1
        # the poisoned keys: NaN and huge values exactly on the points outside the bands
        key = K.poison_gaps(K.special_keys(n, 50), begin, end)
        rank, ordered = K.ref_band_sort(key, begin, end)
        outside = np.ones(n, dtype=bool)
        for b, e in live:
            outside[b:e + 1] = False
        assert outside.any() or name in ("two-adjacent", "most-one-sort-flush")
        assert np.array_equal(rank[outside], np.flatnonzero(outside)) and np.array_equal(ordered[outside], np.flatnonzero(outside))
        assert np.isnan(key[outside]).sum() >= outside.sum() // 4
    classes = ["leading gap", "no leading gap", "trailing gap", "no trailing gap", "empty band in the middle", "one-point band",
               "one-point gap", "adjacent bands", "end on T-1", "end on T", "end on T+1", "full segment table"]
    assert all(seen[c] > 0 for c in classes), seen
    b2, e2 = lists["two-gaps"]
    b3, e3 = lists["thirteen"]
    assert e2[0] == T - 1 and lists["two-adjacent"][1][0] == T and T + 1 in e3        # the first tile's own edge, all three
    assert lists["descending"][0] == b3[::-1] and lists["descending"][1] == e3[::-1]


def test_scan_round_length_reaches_the_second_round(geo):
    R, B = geo["sort_scan_round_tiles"], geo["sort_max_one_sort_bands"]
    for T in (geo["sort_keys_per_tile"], 2048):                # the process's tile, and ECCKD_SORT_ITEMS=8's
        n = K.scan_round_length(T, R)
        assert n == R * T + T + 17 and n < 2 ** 31 - 1
        assert K.scan_rounds(n, T, R) == 2 and K.sort_tiles(n, T) - R == 2 and n - (K.sort_tiles(n, T) - 1) * T == 17
        assert K.scan_rounds(R * T, T, R) == 1                 # one key fewer than a tile more: still one round
        bands = K.scan_round_bands(n)
        assert K.sort_path(n, *bands["single"], B) == "per_band_whole"
        assert K.sort_path(n, *bands["two"], B) == "one_sort"  # the one sort runs over the whole array: two rounds as well
        (b0, b1), (e0, e1) = bands["two"]
        assert b0 == 0 and e1 == n - 1 and b1 - e0 > 1
    # what the suite sorted before: BASELINE's 7.2e6 keys are one round at the default tile, 200 003 keys one at 2 048
    assert K.scan_rounds(7_200_000, 3840, R) == 1 and K.scan_rounds(200_003, 2048, R) == 1


def test_regroup_cases_hold_every_class(geo):
    from test_find_g_band_gpu import ref_regroup
    T, G = geo["sort_keys_per_tile"], geo["max_groups"]
    cases = K.regroup_cases(T, G)
    seen = Counter()
    for c in cases:
        n = c.rank.size
        nsub = c.wn_bound.size - 1
        member = (c.rank >= c.lo) & (c.rank <= c.hi)
        seen["nsub %d" % nsub] += 1
        seen["range of %d" % (c.hi - c.lo + 1)] += 1
        seen["whole range"] += (c.lo, c.hi) == (0, n - 1)
        seen["interior range"] += c.lo > 0 and c.hi < n - 1
        assert np.all(np.diff(c.wn_bound) >= 0)
        assert np.all((c.wn[member] >= c.wn_bound[0]) & (c.wn[member] < c.wn_bound[-1]))      # every point has a group
        on = np.isin(c.wn[member], c.wn_bound)
        seen["point on a lower bound"] += bool(np.any(c.wn[member] == c.wn_bound[0]))
        seen["point on an inner bound"] += bool(np.any(np.isin(c.wn[member], c.wn_bound[1:-1])))
        assert on.any()
        want, ends = ref_regroup(c.wn, c.rank, c.lo, c.hi, c.wn_bound)
        counts = np.diff(np.concatenate([[c.lo - 1], ends]))
        assert counts.sum() == c.hi - c.lo + 1 and ends[-1] == c.hi
        seen["empty group"] += bool(np.any(counts == 0))
        assert np.array_equal(want[~member], c.rank[~member]) and np.array_equal(np.sort(want), np.arange(n))
        # a point ON an inner bound belongs to the group that begins there
        for q in range(1, nsub):
            hit = np.flatnonzero(member & (c.wn == c.wn_bound[q]))
            later = [s for s in range(q, nsub) if c.wn_bound[s + 1] > c.wn_bound[q]][0]
            for j in hit:
                assert (ends[later - 1] if later else c.lo - 1) < want[j] <= ends[later]
    classes = ["nsub 1", "nsub 2", "nsub %d" % G, "range of 1", "range of %d" % (T - 1), "range of %d" % T, "range of %d" % (T + 1),
               "whole range", "interior range", "point on a lower bound", "point on an inner bound", "empty group"]
    assert all(seen[c] > 0 for c in classes), seen


@pytest.fixture(scope="module")
def median_calls(geo):
    return K.median_calls(geo["median_tile"])


def test_median_restatement_is_the_oracles_loop(oracle, geo, median_calls):
    M = geo["median_tile"]
    n = K.median_length(M)
    sv = np.arange(n, dtype=np.float64)
    for call in median_calls:
        assert call.weight.size == n and call.weight.min() >= 0 and call.weight.max() <= K.MAX_WEIGHT
        w = call.weight.astype(np.float64)
        for a, b in zip(call.ind1, call.ind2):
            assert 0 <= a <= b < n
            index, _, _ = K.ref_median(call.weight, a, b)
            assert oracle.median_sorting_variable(sv, w, a, b) == float(index), (call.name, a, b)


def test_median_cases_reach_every_stage(geo, median_calls):
    M = geo["median_tile"]
    seen = Counter()
    placed = {}
    for call in median_calls:
        seen["single interval" if len(call.ind1) == 1 else "many intervals"] += 1
        seen["about 300 intervals"] += 280 <= len(call.ind1) <= 320
        for a, b in zip(call.ind1, call.ind2):
            index, crossed, exact = K.ref_median(call.weight, a, b)
            head, ntile, tail, seg = K.median_geometry(a, b, M)
            stage = K.median_stage(a, b, index, crossed, M)
            total = int(call.weight[a:b + 1].sum())
            seen[stage[0]] += 1
            seen["seg %d" % seg] += 1
            seen["equal to half"] += exact
            if ntile == 0:
                seen["no tile: " + ("one point" if a == b else "two points" if b == a + 1 else "inside a tile" if a // M == b // M
                                    else "across an edge")] += 1
                seen["no tile: %d points" % (b - a + 1)] += 1
            else:
                seen["head %d tail %d" % (head, tail)] += 1
                seen["%d tiles" % ntile] += 1
            if stage[0] == "tile":
                _, thread, place, point = stage
                seen["tile: point %d" % point] += 1
                seen["tile: thread %d place %d of %d" % (min(thread, 1), place, seg)] += 1
                seen["tile: last of a run of %d" % seg] += place == seg - 1
            if total == 0:
                assert index == a or a == b
                seen["zero: " + ("no tile" if ntile == 0 else "head and tiles" if head else "i1 on a tile edge and tiles")] += 1
            elif call.weight[a] == 0 and a < b:
                lead = int(np.flatnonzero(call.weight[a:b + 1])[0])
                seen["leading zeros"] += lead >= M
            if call.name not in ("many", "zero"):
                gname, pname, variant = call.name.split("/")
                want = K.median_placements(a, b, M)[pname]
                assert index == want and exact == (variant == "equal") and crossed == (want != b), call.name
                placed.setdefault(pname, set()).add(variant)
                if pname == "i2":
                    assert call.weight[b] == call.weight[a:b].sum() + 1          # one short of half in front of i2
    classes = ["single interval", "many intervals", "about 300 intervals", "head", "tile", "tail", "fall-through", "seg 0", "seg 1",
               "seg 2", "seg 3", "equal to half", "no tile: one point", "no tile: two points", "no tile: inside a tile",
               "no tile: across an edge", "no tile: %d points" % (2 * M - 2), "tile: point 0", "tile: point %d" % (M - 1),
               "tile: thread 0 place 1 of 2", "tile: thread 1 place 0 of 2", "tile: thread 0 place 2 of 3", "tile: thread 1 place 0 of 3",
               "tile: last of a run of 2", "zero: no tile", "zero: head and tiles", "zero: i1 on a tile edge and tiles", "leading zeros"]
    classes += ["head %d tail %d" % (h, t) for h in (0, 1, M - 1) for t in (0, 1, M - 1)]
    classes += ["%d tiles" % k for k in (1, M - 1, M, M + 1, 2 * M, 2 * M + 1)]
    assert all(seen[c] > 0 for c in classes), [c for c in classes if not seen[c]]
    names = ["i1", "last-head-point", "first-tile-first-point", "tile-last-point", "next-tile-first-point", "thread0-last-tile",
             "thread0-last-tile-last-point", "thread1-first-tile", "thread1-first-tile-inside", "first-tail-point", "i2-1", "i2"]
    assert set(placed) == set(names)
    assert all(placed[p] == ({"above"} if p == "i2" else {"above", "equal"}) for p in names), placed
    # 257 tiles: runs of two, 129 threads busy, the last run a single tile
    seg = K.median_geometry(M, 258 * M, M)[3]
    assert seg == 2 and -(-257 // seg) == 129 and 257 - 128 * seg == 1
    # the issue's worked example is among the zero-weight intervals
    zero = [c for c in median_calls if c.name == "zero"][0]
    assert (M, 4 * M - 1) in list(zip(zero.ind1, zero.ind2)) and zero.weight[M:4 * M].sum() == 0


def test_g_point_map_cases_hold_every_class():
    seen = Counter()
    for name, rank, r1, r2 in K.g_point_cases():
        n = rank.size
        assert np.array_equal(np.sort(rank), np.arange(n))
        g = K.ref_gas_g_point(rank, r1, r2)
        seen["n %d" % n] += 1
        seen["ng 1"] += len(r1) == 1
        seen["rank in no range"] += bool(np.any(g < 0))
        seen["empty range"] += any(b < a for a, b in zip(r1, r2))
        seen["one-rank range"] += any(b == a for a, b in zip(r1, r2))
        for ig, (a, b) in enumerate(zip(r1, r2)):
            for later, (a2, b2) in list(enumerate(zip(r1, r2)))[ig + 1:]:
                both = [r for r in (a, b) if a <= b and a2 <= r <= b2]
                for r in both:                                                   # ON an edge of an earlier range and inside a later
                    assert g[np.flatnonzero(rank == r)[0]] >= later
                    seen["later range wins"] += 1
            if a <= b and not any(a2 <= a <= b2 for a2, b2 in list(zip(r1, r2))[ig + 1:]):
                assert g[np.flatnonzero(rank == a)[0]] == ig                     # a rank exactly on rank1
                seen["on rank1"] += 1
            if a <= b and not any(a2 <= b <= b2 for a2, b2 in list(zip(r1, r2))[ig + 1:]):
                assert g[np.flatnonzero(rank == b)[0]] == ig
                seen["on rank2"] += 1
    for name, gp, lo, hi in K.merge_cases():
        out, nun = K.ref_merge_g_points(gp, lo, hi)
        seen["merge n %d" % gp[0].size] += 1
        seen["merge %d gas" % len(gp)] += 1
        seen["merge ng 1"] += lo.shape[1] == 1
        seen["unassigned"] += 0 < nun < out.size
        seen["merged"] += bool(np.any(out >= 0))
    classes = ["n 255", "n 256", "n 257", "ng 1", "rank in no range", "empty range", "one-rank range", "later range wins", "on rank1",
               "on rank2", "merge n 255", "merge n 256", "merge n 257", "merge 1 gas", "merge 3 gas", "merge ng 1", "unassigned", "merged"]
    assert all(seen[c] > 0 for c in classes), seen
