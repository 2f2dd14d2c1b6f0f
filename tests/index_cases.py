"""Inputs and exact references for the index kernels: K3's stable band sort (csrc/radix_sort.hip), the wavenumber regrouping
and the weighted median of csrc/find_g_band.hip, the rank -> g-point maps of csrc/overlap.hip (test_index_cases.py on the CPU,
test_index_edges_gpu.py on the device).  numpy only.

Nothing here knows a tile size: every builder takes the geometry that ecckd_index_geometry reports - T keys per sort tile,
W keys per wave, R tile counts per round of the row scan, the largest band count of the one-sort path, the median's tile M -
and derives its edges from it.  The results of these kernels are integers, or one value picked by an integer, so every
reference is exact: numpy's stable argsort for the sort, integer cumulative sums for the median (the weights are small
integers stored as doubles: every partial sum is exact in whatever order it is formed), `where` passes for the maps.

Which path of the host code and which stage of a kernel a case reaches is restated here (sort_path, scan_rounds,
median_geometry, median_stage) from the inputs and the reference alone; test_index_cases.py asserts that every class is hit."""
from collections import namedtuple

import numpy as np

# ------------------------------------------------------------------------------------------------------------------- sort

SortCase = namedtuple("SortCase", "name key begin end")


def ref_argsort(key):
    """std::stable_sort with `<` (reorder_spectrum.cpp:262-300) on keys where -0.0 == +0.0; NaN keys last, in index order
    (numpy's stable sort treats NaN as the largest value, all NaNs equal)."""
    return np.argsort(np.where(key == 0.0, 0.0, key), kind="stable")


def ref_band_sort(key, begin, end):
    """(rank, ordered_index) of ecckd_stable_argsort_bands_dev: every band [begin, end] sorted on its own, the points outside
    every band in place; a band with end < begin is empty."""
    n = key.size
    ordered = np.arange(n, dtype=np.int64)
    rank = np.arange(n, dtype=np.int64)
    for b, e in zip(begin, end):
        if e < b:
            continue
        o = b + ref_argsort(key[b:e + 1])
        ordered[b:e + 1] = o
        rank[o] = np.arange(b, e + 1)
    return rank, ordered


def sort_path(n, begin, end, max_one_sort_bands):
    """The branch of ecckd_stable_argsort_bands_dev: "identity" (no point in a band), "one_sort" (2 .. max bands, ascending
    and disjoint: eight passes over the key and one over the segment), else band by band - "whole" when a band covers the
    whole array (no identity fill) or "identity" + the bands."""
    live = [(b, e) for b, e in zip(begin, end) if e >= b]
    if not live:
        return "identity"
    ascending = all(live[i][0] > live[i - 1][1] for i in range(1, len(live)))
    if 1 < len(begin) <= max_one_sort_bands and ascending:
        return "one_sort"
    return "per_band_whole" if any(b == 0 and e == n - 1 for b, e in live) else "per_band_identity"


def sort_tiles(n, T):
    return -(-n // T)


def scan_rounds(n, T, R):
    """rounds of k_sort_scan_rows for a sort of n keys"""
    return -(-sort_tiles(n, T) // R)


def one_band_lengths(T, W):
    return [1, 2, 63, 64, 65, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]


def mixed_keys(n, seed):
    """random keys of many magnitudes and both signs with a large tie group, some zeros of either sign"""
    rs = np.random.RandomState(seed)
    key = rs.standard_normal(n) * np.exp(rs.uniform(-30, 30, n))
    key[rs.uniform(size=n) < 0.25] = -0.5
    key[rs.uniform(size=n) < 0.03] = 0.0
    key[rs.uniform(size=n) < 0.03] = -0.0
    return key


ONE_BAND_OFFSET = 37        # no multiple of anything


def one_band_cases(T, W):
    """every length once as one band over the whole array and once at an unaligned offset inside a longer array"""
    out = []
    for k, n in enumerate(one_band_lengths(T, W)):
        out.append(SortCase("whole-%d" % n, mixed_keys(n, 100 + k), [0], [n - 1]))
        out.append(SortCase("inside-%d" % n, mixed_keys(ONE_BAND_OFFSET + n + 11, 200 + k), [ONE_BAND_OFFSET],
                            [ONE_BAND_OFFSET + n - 1]))
    return out


BYTE_BASE = 0x3F5A3C6996A5C31E     # eight different bytes; no byte-7 / byte-6 value turns it into a NaN, an inf or a zero


def byte_keys(b, T, seed=0):
    """keys that differ in byte b only (b = 0: lowest mantissa byte ... 7: sign and high exponent bits): byte b takes all 256
    values, the other bytes are those of BYTE_BASE; each value several times, under both signs, shuffled; more than one tile"""
    reps = max(4, -(-(T + 1) // 512))
    v = np.arange(256, dtype=np.uint64)
    pat = (np.uint64(BYTE_BASE) & ~(np.uint64(0xFF) << np.uint64(8 * b))) | (v << np.uint64(8 * b))
    pat = np.concatenate([pat, pat ^ np.uint64(1 << 63)])
    pat = np.tile(pat, reps)
    np.random.RandomState(seed + b).shuffle(pat)
    return pat.view(np.float64).copy()


NAN_PATTERNS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF0000000000001,
                0xFFF00000DEADBEEF]
SPECIALS = [0.0, -0.0, 5e-324, -5e-324, np.finfo(np.float64).max, -np.finfo(np.float64).max, np.inf, -np.inf]


def special_keys(n, seed):
    """mixed_keys with +-0, +-the smallest denormal, +-the largest finite, +-inf and NaNs of either sign and several payloads,
    each several times"""
    rs = np.random.RandomState(seed)
    key = mixed_keys(n, seed + 1)
    pool = np.concatenate([np.array(SPECIALS), np.array(NAN_PATTERNS, dtype=np.uint64).view(np.float64)])
    where = rs.choice(n, min(n, 12 * pool.size), replace=False)
    key[where] = np.resize(pool, where.size)
    return key


GAP_POISON = np.array([np.nan, np.finfo(np.float64).max, -np.inf, -np.finfo(np.float64).max])


def poison_gaps(key, begin, end):
    """a copy of key with NaN and huge values on every point outside the bands (they must keep their places)"""
    inside = np.zeros(key.size, dtype=bool)
    for b, e in zip(begin, end):
        if e >= b:
            inside[b:e + 1] = True
    out = key.copy()
    gaps = np.flatnonzero(~inside)
    out[gaps] = np.resize(GAP_POISON, gaps.size)
    return out


def _random_bands(n0, n1, nband, seed, lead, trail):
    """nband bands in [n0, n1] with a gap of 1..3 points between neighbours; a leading / trailing gap or none"""
    rs = np.random.RandomState(seed)
    lo = n0 + (2 if lead else 0)
    hi = n1 - (3 if trail else 0)
    # 2 nband - 1 pieces (band, gap, band, ...) from 2 nband - 2 distinct cuts
    cuts = np.sort(rs.choice(np.arange(lo + 1, hi + 1), 2 * nband - 2, replace=False))
    edges = np.concatenate([[lo], cuts, [hi + 1]])
    begin, end = [], []
    for k in range(nband):
        b, e = edges[2 * k], edges[2 * k + 1] - 1
        begin.append(int(b))
        end.append(int(e))
        # the gap [edges[2k+1], edges[2k+2]) is cut down to at most 3 points by handing the rest to the next band
        if k < nband - 1 and edges[2 * k + 2] - edges[2 * k + 1] > 3:
            edges[2 * k + 2] = edges[2 * k + 1] + 1 + rs.randint(3)
    return begin, end


def band_list_length(T):
    return 5 * T + 123


def band_lists(T, max_one_sort_bands):
    """name -> (begin, end) on an array of band_list_length(T) keys"""
    n = band_list_length(T)
    B = max_one_sort_bands
    lists = {
        # leading gap, a band that ends on T-1, a one-point gap on T, a band that begins on T+1, trailing gap
        "two-gaps": ([3, T + 1], [T - 1, n - 4]),
        # no leading and no trailing gap, two adjacent bands, the first ends on T
        "two-adjacent": ([0, T + 1], [T, n - 1]),
        # a one-point band on 0, a one-point gap, ends on T-1, T (a one-point band), T+1 (another), 2T, an empty band in the
        # middle, ends on 3T+1 and 4T-1, adjacent bands, seven short ones, trailing gap
        "thirteen": ([0, 2, T, T + 1, T + 2, 2 * T + 2, 2 * T + 1, 3 * T + 2, 4 * T + 5, 4 * T + 40, 4 * T + 50, 4 * T + 51, 5 * T],
                     [0, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 1, 4 * T - 1, 4 * T + 30, 4 * T + 48, 4 * T + 50, 5 * T - 1,
                      5 * T + 100]),
    }
    lists["most-one-sort"] = _random_bands(0, n - 1, B, 7, lead=True, trail=True)        # 2 B + 1 segments: the table is full
    lists["most-one-sort-flush"] = _random_bands(0, n - 1, B, 8, lead=False, trail=False)
    lists["one-too-many"] = _random_bands(0, n - 1, B + 1, 9, lead=True, trail=True)      # band by band
    b13, e13 = lists["thirteen"]
    lists["descending"] = (b13[::-1], e13[::-1])                                          # falls back to band by band
    return lists


def scan_round_length(T, R):
    """one full round of the row scan, then a whole tile and a ragged one in the second round"""
    return R * T + T + 17


def scan_round_keys(n, seed=5):
    rs = np.random.RandomState(seed)
    key = rs.standard_normal(n)
    tie = rs.uniform(size=n) < 0.3
    key[tie] = np.round(key[tie], 3)
    return key


def scan_round_bands(n):
    """the array as a single band, and as two bands with a gap between them (one sort over the whole array)"""
    return {"single": ([0], [n - 1]), "two": ([0, n // 2 + 3], [n // 2 - 2, n - 1])}


# ---------------------------------------------------------------------------------------------------------------- regroup

RegroupCase = namedtuple("RegroupCase", "name wn rank lo hi wn_bound")


def regroup_wavenumbers(n):
    return 100.0 + 0.25 * np.arange(n)       # exact: a bound can be put ON a wavenumber


def regroup_cases(T, max_groups):
    """nsub = 1, 2, max_groups; rank ranges of 1, T-1, T, T+1 points, [0, n-1] and interior ones; bounds that lie on
    wavenumbers of the range (a lower bound takes the point, an upper bound gives it to the next group); an empty group"""
    n = 3 * T + 100
    wn = regroup_wavenumbers(n)
    top = wn[-1] + 1.0
    rs = np.random.RandomState(11)
    out = []
    ranges = [("all", 0, n - 1), ("one", T + 5, T + 5), ("T-1", 50, 50 + T - 2), ("T", 51, 50 + T), ("T+1", T - 1, 2 * T - 1),
              ("interior", 7, n - 9)]
    for rname, lo, hi in ranges:
        for nsub in (1, 2, max_groups):
            rank = rs.permutation(n).astype(np.int64)
            member = np.flatnonzero((rank >= lo) & (rank <= hi))            # original indices of the range's points
            if nsub == 1:
                wb = [wn[member].min(), top]                                # the lowest point lies ON the lower bound
            elif nsub == 2:
                wb = [wn[0], wn[member[member.size // 2]], top]             # a point of the range ON the inner bound
            else:
                inner = np.sort(wn[rs.choice(n, nsub - 1, replace=False)])
                inner[nsub // 2] = inner[nsub // 2 - 1]                     # two equal bounds: an empty group
                inner[3] = wn[member[0]]                                    # a point of the range ON an inner bound
                wb = [wn[0]] + np.sort(inner).tolist() + [top]
            out.append(RegroupCase("%s-%d" % (rname, nsub), wn, rank, lo, hi, np.array(wb)))
    return out


# ----------------------------------------------------------------------------------------------------------------- median

MedianCall = namedtuple("MedianCall", "name weight ind1 ind2")     # weight: int64 [n]; one call of the entry
THREADS = 256                                                     # k_median_sorting: a block of 256 threads per interval
MAX_WEIGHT = 1000


def median_length(M):
    return 514 * M + 700


def ref_median(weight, i1, i2):
    """calc_median_sorting_variable (find_g_points.cpp:35-49) on integer weights -> (index, crossed, exact): the first index
    of i1 .. i2-1 at which the running sum (:43) has reached half the sum over [i1, i2] (:39, :44), else i2 (:48);
    `crossed` says the loop broke, `exact` that the running sum EQUALS half the total there."""
    c = np.cumsum(weight[i1:i2 + 1].astype(np.int64))
    hit = np.flatnonzero(2 * c[:-1] >= c[-1])
    if hit.size == 0:
        return int(i2), False, False
    return int(i1 + hit[0]), True, bool(2 * c[hit[0]] == c[-1])


def median_geometry(i1, i2, M):
    """(head points, whole tiles, tail points, tiles per thread) as k_median_sorting cuts [i1, i2]"""
    t1, t2 = -(-i1 // M), (i2 + 1) // M
    if t1 >= t2:
        return i2 - i1 + 1, 0, 0, 0
    return t1 * M - i1, t2 - t1, i2 + 1 - t2 * M, -(-(t2 - t1) // THREADS)


def median_stage(i1, i2, index, crossed, M):
    """where the reference's answer lies in the kernel's top-down search: "fall-through" (no crossing before i2), "head"
    (everything, without a whole tile), ("tile", thread, place in the thread's run of tiles, point in the tile), "tail" """
    head, ntile, tail, seg = median_geometry(i1, i2, M)
    if not crossed:
        return ("fall-through",)
    if index < i1 + head:
        return ("head",)
    if index >= i2 + 1 - tail:
        return ("tail",)
    t = (index - (i1 + head)) // M
    return ("tile", t // seg, t % seg, index % M)


def _grow(rs, a, amount):
    k = -(-amount // 900)
    idx = rs.choice(a.size, k, replace=False)
    a[idx] += 900
    a[idx[0]] -= 900 * k - amount


def _shrink(rs, a, amount):
    order = rs.permutation(a.size)
    k = int(np.searchsorted(np.cumsum(a[order]), amount)) + 1
    a[order[:k]] = 0


def _balance(rs, left, right, lo, hi):
    """change the integer weights in place until lo <= sum(right) - sum(left) <= hi, each weight staying in 0 .. 903"""
    mid = (lo + hi) // 2
    for _ in range(6):
        d = int(right.sum() - left.sum())
        if lo <= d <= hi:
            return
        if d < lo:
            if right.size * 900 >= mid - d:
                _grow(rs, right, mid - d)
            else:
                _shrink(rs, left, mid - d)
        else:
            if left.size * 900 >= d - mid:
                _grow(rs, left, d - mid)
            else:
                _shrink(rs, right, d - mid)
    raise AssertionError("weights could not be balanced")


def place_crossing(n, i1, i2, p, exact, seed):
    """integer weights [n] for which the reference's loop over [i1, i2] stops at p (i1 <= p < i2) - with the running sum above
    half the total, or EQUAL to it (exact) - or, for p == i2, never stops: the points before p (L) and after p (R) carry
    weights 0 .. 3 balanced so that 0 < R - L < 1000, and p the weight R - L (exact) or R - L + 1.  For p == i2 the heavy
    weight lies on i2 and the points before it sum to one less than it (the loop never looks at i2: its equality variant is the
    placement i2 - 1)."""
    rs = np.random.RandomState(seed)
    w = rs.randint(0, MAX_WEIGHT + 1, n).astype(np.int64)       # outside the interval: anything
    left = rs.randint(0, 4, p - i1).astype(np.int64)
    right = rs.randint(0, 4, i2 - p).astype(np.int64)
    if p == i2:
        if left.sum() > 899:
            _shrink(rs, left, int(left.sum()) - 899)
        w[i1:p] = left
        w[p] = left.sum() + 1
        return w
    _balance(rs, left, right, 1, 998)
    d = int(right.sum() - left.sum())
    w[i1:p] = left
    w[p] = d if exact else d + 1
    w[p + 1:i2 + 1] = right
    return w


def median_placement_geometries(M):
    """(name, i1, i2): head / whole tiles / tail of 255 / 3 / 100 (one tile per thread), 1 / 300 / 255 (two per thread),
    0 / 257 / 1 (two per thread, the last run a single tile, threads 129 .. 255 without one), 0 / 513 / 0 (three per thread)"""
    return [("seg1", 2 * M - 255, 5 * M + 99), ("seg2", 3 * M - 1, 303 * M + 254), ("seg2-257", M, 258 * M), ("seg3", M, 514 * M - 1)]


def median_placements(i1, i2, M):
    """name -> index of the crossing, for the interval [i1, i2]"""
    head, ntile, tail, seg = median_geometry(i1, i2, M)
    first = i1 + head                       # first point of the first whole tile
    out = {"i1": i1, "first-tile-first-point": first, "i2-1": i2 - 1, "i2": i2}
    if head:
        out["last-head-point"] = first - 1
    mid = first + (ntile // 2) * M
    out["tile-last-point"] = mid + M - 1
    if ntile // 2 + 1 < ntile:
        out["next-tile-first-point"] = mid + M
    if seg >= 2:
        out["thread0-last-tile"] = first + (seg - 1) * M + 77          # the last tile of thread 0's run
        out["thread0-last-tile-last-point"] = first + seg * M - 1
        out["thread1-first-tile"] = first + seg * M                    # the first tile of thread 1's run, its first point
        out["thread1-first-tile-inside"] = first + seg * M + 200
    if tail > 1:                            # (a tail of one point is i2 itself)
        out["first-tail-point"] = i2 + 1 - tail
    return out


def median_placement_calls(M):
    """one call of one interval per geometry, placement and variant (running sum above half / equal to half)"""
    n = median_length(M)
    out = []
    seed = 0
    for gname, i1, i2 in median_placement_geometries(M):
        for pname, p in sorted(median_placements(i1, i2, M).items()):
            for exact in (False, True):
                if exact and p == i2:
                    continue
                seed += 1
                out.append(MedianCall("%s/%s/%s" % (gname, pname, "equal" if exact else "above"),
                                      place_crossing(n, i1, i2, p, exact, seed), [i1], [i2]))
    return out


def median_many_call(M, seed=21):
    """one call of about 300 intervals over random weights 0 .. 1000: every interval without a whole tile, every head of 0, 1,
    M-1 points crossed with every tail of 0, 1, M-1 points around 1, M-1, M, M+1, 2M and 2M+1 whole tiles, random ones"""
    n = median_length(M)
    rs = np.random.RandomState(seed)
    w = rs.randint(0, MAX_WEIGHT + 1, n).astype(np.int64)
    iv = [(0, 0), (n - 1, n - 1), (5, 6), (M - 1, M), (3 * M + 2, 4 * M - 3), (3 * M, 4 * M - 2), (3 * M + 1, 4 * M - 1),
          (7 * M + 1, 9 * M - 2), (7 * M + 100, 8 * M + 100)]
    for ntile in (1, M - 1, M, M + 1, 2 * M, 2 * M + 1):
        for head in (0, 1, M - 1):
            for tail in (0, 1, M - 1):
                for a in {1, 1 + (514 - 1 - ntile) // 2, 514 - ntile}:
                    iv.append((a * M - head, (a + ntile) * M - 1 + tail))
    while len(iv) < 300:
        a, b = sorted(rs.randint(0, n, 2).tolist())
        iv.append((a, b))
    return MedianCall("many", w, [a for a, _ in iv], [b for _, b in iv])


def median_zero_call(M, seed=22):
    """intervals without any weight - without a whole tile, with a head in front of whole tiles, with i1 ON a tile edge in
    front of whole tiles (the reference stops at i1: 0 >= 0) - and intervals that begin with a run of zero weights"""
    n = median_length(M)
    rs = np.random.RandomState(seed)
    w = rs.randint(0, MAX_WEIGHT + 1, n).astype(np.int64)
    w[:30 * M] = 0
    iv = [(10 * M + 3, 10 * M + 200), (10 * M + 3, 10 * M + 3), (10 * M - 100, 14 * M + 5), (M, 4 * M - 1), (10 * M, 14 * M - 1),
          (10 * M, 13 * M + 7), (2 * M, 3 * M - 1), (0, 29 * M + 17), (M, 29 * M)]
    # leading zeros, then weight: i1 on a tile edge and off it, the zeros end inside a tile and on a tile edge
    iv += [(27 * M, 40 * M + 17), (27 * M + 9, 40 * M + 17), (29 * M + 250, 30 * M + 100), (28 * M, 31 * M - 1)]
    w[40 * M:43 * M + 5] = 0
    iv += [(40 * M, 50 * M + 3), (40 * M - 3, 300 * M)]
    return MedianCall("zero", w, [a for a, _ in iv], [b for _, b in iv])


def median_calls(M):
    return median_placement_calls(M) + [median_many_call(M), median_zero_call(M)]


# ------------------------------------------------------------------------------------------------------------ g-point maps

def ref_gas_g_point(rank, rank1, rank2):
    """SingleGasData::store_g_points (single_gas_data.h:56-62): g point ig for the ranks in [rank1[ig], rank2[ig]], later ones
    overwrite; -1 where no range holds the rank"""
    out = np.full(rank.size, -1, dtype=np.int32)
    for ig, (a, b) in enumerate(zip(rank1, rank2)):
        out[(rank >= a) & (rank <= b)] = ig
    return out


def ref_merge_g_points(gas_g_point, g_min, g_max):
    """find_g_points.cpp:1459-1475 -> (merged g point, number of points without one)"""
    n = gas_g_point[0].size
    out = np.full(n, -1, dtype=np.int32)
    for ig in range(g_min.shape[1]):
        found = np.ones(n, dtype=bool)
        for i, g in enumerate(gas_g_point):
            found &= (g >= g_min[i, ig]) & (g <= g_max[i, ig])
        out[found] = ig
    return out, int(np.count_nonzero(out < 0))


def g_point_cases():
    """(name, rank, rank1, rank2): 255, 256, 257 points (a block of the kernel is 256); one range; ranges that overlap (the
    later one wins), leave ranks out (-1), hold a single rank, and an empty one"""
    out = []
    for n in (255, 256, 257):
        rank = np.random.RandomState(n).permutation(n).astype(np.int32)
        out.append(("%d-one" % n, rank, [0], [n - 1]))
        out.append(("%d-one-short" % n, rank, [1], [n - 2]))
        out.append(("%d-overlap" % n, rank, [0, 40, 100, 90, 200, 250], [60, 99, 150, 120, 200, 249]))
    return out


def merge_cases():
    """(name, gas g points [ngas][n], g_min, g_max [ngas][ng]): one gas and three, 255 / 256 / 257 points, points that no merged
    g point takes, merged g points that overlap (the later one wins)"""
    out = []
    for n in (255, 256, 257):
        for ngas in (1, 3):
            rs = np.random.RandomState(10 * n + ngas)
            gp = [rs.randint(-1, 5, n).astype(np.int32) for _ in range(ngas)]
            ng = 6
            lo = rs.randint(0, 4, (ngas, ng)).astype(np.int32)
            hi = (lo + rs.randint(0, 3, (ngas, ng))).astype(np.int32)
            out.append(("%d-%dgas" % (n, ngas), gp, lo, hi))
        gp = [np.random.RandomState(n).randint(-1, 3, n).astype(np.int32)]
        out.append(("%d-ng1" % n, gp, np.array([[1]], dtype=np.int32), np.array([[2]], dtype=np.int32)))
    return out
