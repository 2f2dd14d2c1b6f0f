"""The index kernels at the edges of their own tiling: K3's stable band sort (radix_sort.hip), the wavenumber regrouping and the
weighted median (find_g_band.hip), the rank -> g-point maps (overlap.hip).  Their results are integers, or one value picked by
an integer: every comparison here is array_equal against the exact references of index_cases.py, there is no tolerance.  The
edges - tile, wave, scan round, band count of the one-sort path, median tile, group count - come from ecckd_index_geometry, so
they follow the kernels; test_index_cases.py shows on the CPU which path every case reaches.

Seconds on one MI355X, host references included: one band at wave and tile edges 0.04, every digit 0.01, special values
< 0.005, band lists 0.05, second round of the row scan 1.97 (7 868 177 keys: two host argsorts), regroup 0.13, median 0.11
(78 calls), g-point maps 0.01."""
import ctypes as C

import numpy as np
import pytest
import torch

import index_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo():
    from ecckd_amd import api
    return api.index_geometry()


def _dev(ctx, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)


def _sort_matches(ctx, key, begin, end, name):
    from ecckd_amd import api
    want_rank, want_ordered = K.ref_band_sort(key, begin, end)
    d_key = _dev(ctx, key)
    rank, ordered = api.stable_argsort_bands(ctx, d_key, begin, end)
    assert np.array_equal(rank.cpu().numpy(), want_rank), name
    assert np.array_equal(ordered.cpu().numpy(), want_ordered), name
    rank2, none = api.stable_argsort_bands(ctx, d_key, begin, end, want_ordered=False)
    assert none is None and np.array_equal(rank2.cpu().numpy(), want_rank), name


def test_one_band_at_wave_and_tile_edges(ctx, geo):
    for c in K.one_band_cases(geo["sort_keys_per_tile"], geo["sort_keys_per_wave"]):
        _sort_matches(ctx, c.key, c.begin, c.end, c.name)


def test_every_digit_of_the_key_on_its_own(ctx, geo):
    for b in range(8):
        key = K.byte_keys(b, geo["sort_keys_per_tile"])
        _sort_matches(ctx, key, [0], [key.size - 1], "byte %d" % b)


def test_special_values_among_random_keys(ctx, geo):
    T = geo["sort_keys_per_tile"]
    for n in (T - 1, 3 * T + 5):
        key = K.special_keys(n, 40 + n % 7)
        _sort_matches(ctx, key, [0], [n - 1], "specials, one band of %d" % n)
        _sort_matches(ctx, key, [0, n // 2 + 1], [n // 2 - 1, n - 1], "specials, two bands of %d" % n)


def test_band_lists_up_to_and_past_the_one_sort(ctx, geo):
    T, B = geo["sort_keys_per_tile"], geo["sort_max_one_sort_bands"]
    n = K.band_list_length(T)
    key = K.special_keys(n, 50)
    for name, (begin, end) in K.band_lists(T, B).items():
        _sort_matches(ctx, key, begin, end, name)
        _sort_matches(ctx, K.poison_gaps(key, begin, end), begin, end, name + ", NaN and huge keys in the gaps")


def test_second_round_of_the_row_scan(ctx, geo):
    """More tiles than one round of k_sort_scan_rows takes: the carry into the second round, as one band (band by band, the
    histogram of the first pass taken by the prepare kernel) and as two bands with a gap (the one nine-pass sort)."""
    from ecckd_amd import api
    T, R = geo["sort_keys_per_tile"], geo["sort_scan_round_tiles"]
    n = K.scan_round_length(T, R)
    assert K.scan_rounds(n, T, R) == 2
    key = K.scan_round_keys(n)
    d_key = _dev(ctx, key)
    for name, (begin, end) in K.scan_round_bands(n).items():
        want_rank, want_ordered = K.ref_band_sort(key, begin, end)
        rank, ordered = api.stable_argsort_bands(ctx, d_key, begin, end)
        assert np.array_equal(rank.cpu().numpy(), want_rank), name
        assert np.array_equal(ordered.cpu().numpy(), want_ordered), name


def test_regroup_on_bounds_and_at_tile_edges(ctx, geo):
    from ecckd_amd import api
    from test_find_g_band_gpu import ref_regroup
    for c in K.regroup_cases(geo["sort_keys_per_tile"], geo["max_groups"]):
        want, ends = ref_regroup(c.wn, c.rank, c.lo, c.hi, c.wn_bound)
        d_rank = _dev(ctx, c.rank.astype(np.int32))
        count = api.regroup_rank_by_wavenumber(ctx, _dev(ctx, c.wn), d_rank, c.lo, c.hi, c.wn_bound)
        got = d_rank.cpu().numpy()
        assert np.array_equal(got, want), c.name
        assert np.array_equal(np.cumsum(count) + c.lo - 1, ends), c.name
        outside = (c.rank < c.lo) | (c.rank > c.hi)
        assert np.array_equal(got[outside], c.rank[outside]), c.name
        # the two index helpers on the new ranks: the inverse permutation and the gather through it
        inv = api.invert_permutation(ctx, d_rank)
        want_inv = np.empty_like(want)
        want_inv[want] = np.arange(want.size)
        assert np.array_equal(inv.cpu().numpy(), want_inv), c.name
        assert np.array_equal(api.gather_f64(ctx, _dev(ctx, c.wn), inv).cpu().numpy(), c.wn[want_inv]), c.name


def test_median_picks_the_references_point_at_every_placement(ctx, geo):
    """Integer weights: every partial sum is exact however it is formed, so the kernel must pick the very point the reference's
    sequential loop picks - in the head, at the first and last tile of a thread's run, on a tile's first and last point, in the
    tail, at i2, with the running sum above half the total and EQUAL to it - and i1 for an interval without weight, also where
    i1 is the first point of a whole tile (find_g_points.cpp:39-48: 0 >= 0 at the first point)."""
    from ecckd_amd import api
    M = geo["median_tile"]
    n = K.median_length(M)
    d_sv = _dev(ctx, np.arange(n, dtype=np.float64))
    wrong = []
    for call in K.median_calls(M):
        want = np.array([K.ref_median(call.weight, a, b)[0] for a, b in zip(call.ind1, call.ind2)], dtype=np.float64)
        got = api.median_sorting_variable(ctx, _dev(ctx, call.weight.astype(np.float64)), d_sv, call.ind1, call.ind2)
        for k in np.flatnonzero(got != want):
            wrong.append((call.name, call.ind1[k], call.ind2[k], int(want[k]), int(got[k])))
    assert not wrong, wrong


def test_g_point_maps_at_block_edges(ctx):
    from ecckd_amd import api
    for name, rank, r1, r2 in K.g_point_cases():
        g = api.gas_g_point(ctx, _dev(ctx, rank), r1, r2)
        assert np.array_equal(g.cpu().numpy(), K.ref_gas_g_point(rank, r1, r2)), name
    for name, gp, lo, hi in K.merge_cases():
        want, want_unassigned = K.ref_merge_g_points(gp, lo, hi)
        d_gp = [_dev(ctx, g) for g in gp]
        out, unassigned = api.merge_g_points(ctx, d_gp, lo, hi)
        assert np.array_equal(out.cpu().numpy(), want) and unassigned == want_unassigned, name
        # rows of g_min / g_max longer than ng (ecckd_overlap_g_points hands out rows of `capacity`): the library called directly
        ngas, ng = lo.shape
        stride = ng + 3
        wide_lo = np.full((ngas, stride), -7, dtype=np.int32)
        wide_hi = np.full((ngas, stride), 99, dtype=np.int32)
        wide_lo[:, :ng], wide_hi[:, :ng] = lo, hi
        ptrs = (C.c_void_p * ngas)(*[t.data_ptr() for t in d_gp])
        out2 = torch.empty(gp[0].size, dtype=torch.int32, device=ctx.device)
        cnt = C.c_int64()
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        ctx.fence_from_torch()
        api.check(ctx.lib.ecckd_merge_g_points_dev(ctx.handle, gp[0].size, ngas, ptrs, ng, stride, ip(wide_lo), ip(wide_hi),
                                                   C.c_void_p(out2.data_ptr()), C.byref(cnt)))
        assert np.array_equal(out2.cpu().numpy(), want) and cnt.value == want_unassigned, name + ", stride > ng"
