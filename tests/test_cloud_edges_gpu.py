"""The cloud pseudo-gas kernels (csrc/cloud.hip) at the edges of their own tiling: the knot search in LDS and in HBM, the scan
tiles, the chunks of the g-point statistics, the blocks of boundary searches, the second pass of the grid-stride kernels, the
flag latches and the refusals of the host code.  The cases and their references are cloud_cases.py's; the edges come from
ecckd_cloud_geometry, so they follow the kernels; test_cloud_cases.py shows on the CPU which edge every case reaches.

The exact cases (dyadic irradiance and sorting variable: every sum exact in any order) are compared bit for bit, every output,
without a margin.  The general cases keep the two numbers of test_cloud_gpu.py: the reference's margin above 1e-10 (asserted on
the CPU), the median to rtol 1e-12.  The sorting variable is compared through its uint64 view.

Seconds on one MI355X, host references included: every test below 0.1 (the nine knot counts 0.01 - 0.09 each, the tile edges
0.04 per permutation, the latches of the second grid pass 0.04); the file 2.8."""
import numpy as np
import pytest
import torch

import cloud_cases as K

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_g_points", "band_number", "rank1", "rank2")


@pytest.fixture(scope="module")
def geo(ctx):
    from ecckd_amd import api
    return api.cloud_geometry(ctx)


def _dev(ctx, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)


def _partition(ctx, c, **change):
    from ecckd_amd import api
    c = c._replace(**change)
    return api.cloud_partition(ctx, _dev(ctx, c.ssi), _dev(ctx, c.rank), _dev(ctx, c.sv), c.begin, c.end, c.max_range, c.capacity)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, want, name):
    for k in INT_KEYS:
        assert np.array_equal(got[k], np.asarray(want[k])), (name, k)
    for k in ("error", "median"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (name, k)


def _exact_matches(ctx, c):
    want = K.partition_exact(c.ssi, c.rank, c.sv, c.begin, c.end, c.max_range)
    assert min(want["count"]) > 0
    _same_bits(_partition(ctx, c), want, c.name)


def test_geometry_follows_the_device(ctx, geo):
    from ecckd_amd import api
    props = torch.cuda.get_device_properties(ctx.device)
    assert geo["grid_points"] == 16 * props.multi_processor_count * 256
    assert {k: v for k, v in geo.items() if k != "grid_points"} == {k: v for k, v in api.cloud_geometry().items() if k != "grid_points"}


# --------------------------------------------------------------------------------------------------------- sorting variable

@pytest.mark.parametrize("k", range(9))
def test_sorting_variable_at_knot_and_grid_edges(ctx, geo, k):
    """2 .. 2 lds_knots + 4 knots (the search in LDS and in HBM), points on, next to and between the knots and beyond both ends,
    1 .. grid_points + 257 of them"""
    from ecckd_amd import api
    c = K.sorting_case(K.knot_counts(geo)[k])
    base = K.abs_inf_numpy(c.x, c.ssa, c.g, c.points)             # elementwise: the tiled points have the tiled reference
    assert np.isfinite(base).all()
    for nwav in K.sorting_sizes(geo, c.points.size):
        xi, want = np.resize(c.points, nwav), np.resize(base, nwav)
        got = api.cloud_sorting_variable(ctx, c.x, c.ssa, c.g, _dev(ctx, xi)).cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(_bits(got), _bits(want)), (c.name, nwav, int(np.count_nonzero(_bits(got) != _bits(want))))


def test_sorting_variable_next_to_a_nan_knot(ctx):
    from ecckd_amd import api
    c = K.nan_knot_case()
    with np.errstate(invalid="ignore"):
        want = K.abs_inf_numpy(c.x, c.ssa, c.g, c.points)
    got = api.cloud_sorting_variable(ctx, c.x, c.ssa, c.g, _dev(ctx, c.points)).cpu().numpy()
    bad = np.isnan(want)
    assert bad.any() and np.array_equal(np.isnan(got), bad)
    assert np.array_equal(_bits(got[~bad]), _bits(want[~bad]))


# ---------------------------------------------------------------------------------------------------------------- partition

@pytest.mark.parametrize("perm", K.PERMS)
def test_partition_at_tile_edges_exactly(ctx, geo, perm):
    """bands of 1 .. 3 T + 5 points as thirteen bands of one call, 20 000 points as one band, at four ranges"""
    cases = [c for c in K.tile_edge_cases(geo) if c.perm == perm]
    assert len(cases) == 2 * len(K.EXACT_RANGES)
    for c in cases:
        _exact_matches(ctx, c)


def test_partition_g_points_at_chunk_and_single_point_edges_exactly(ctx, geo):
    cases = [K.single_point_case(p) for p in ("stable", "reversed")] + K.long_g_point_cases(geo) + [K.chunk_edge_case(geo)]
    for c in cases + [K.constant_band_case(geo)]:
        _exact_matches(ctx, c)


def test_partition_bounds_query_blocks_and_exact_capacity(ctx, geo):
    for c in K.bounds_query_cases(geo):
        _exact_matches(ctx, c)
    c = K.capacity_case()
    want = K.partition_exact(c.ssi, c.rank, c.sv, c.begin, c.end, c.max_range)
    assert sum(want["n_g_points"]) == c.capacity == 5
    _exact_matches(ctx, c)


@pytest.fixture(scope="module")
def grid_cases(geo):
    cases = K.grid_pass_cases(geo)
    return [(c, K.partition_exact(c.ssi, c.rank, c.sv, c.begin, c.end, c.max_range)) for c in cases]


def test_partition_in_the_second_grid_pass_exactly(ctx, geo, grid_cases):
    for c, want in grid_cases:
        assert c.ssi.size == geo["grid_points"] + 257 and c.begin[1] > geo["grid_points"] > c.begin[0]
        _same_bits(_partition(ctx, c), want, c.name)


def test_partition_general_at_tile_edges(ctx, geo):
    for c in K.general_cases(geo):
        want, margin = K.partition_numpy(c.ssi, c.rank, c.sv, K.band_index(c.ssi.size, c.begin, c.end), 1, c.max_range)
        assert margin > K.GENERAL_MARGIN
        got = _partition(ctx, c)
        for k in INT_KEYS:
            assert np.array_equal(got[k], np.asarray(want[k])), (c.name, k)
        assert np.array_equal(got["error"], np.asarray(want["error"])), c.name
        assert np.allclose(got["median"], want["median"], rtol=K.GENERAL_RTOL, atol=0.0), c.name


# ------------------------------------------------------------------------------------------------------ latches and refusals

def _refused(ctx, c, code, fragment, **change):
    from ecckd_amd import api
    with pytest.raises(api.EcckdError) as e:
        _partition(ctx, c, **change)
    assert e.value.code == code and fragment in e.value.message, (e.value.code, e.value.message)


def _with(a, index, value):
    out = a.copy()
    out[index] = value
    return out


@pytest.fixture(scope="module")
def base(geo):
    """thirteen bands with points before, between and after them"""
    c = [c for c in K.tile_edge_cases(geo) if c.name == "thirteen/stable/0.05"][0]
    return c, K.partition_exact(c.ssi, c.rank, c.sv, c.begin, c.end, c.max_range)


NEGATIVE, PERMUTE, NAN_SV = "negative (or NaN)", "does not permute", "sorting variable is NaN"


def test_flag_latches_of_the_scatter(ctx, base):
    c, want = base
    n = c.ssi.size
    last, gap = n - 1, c.end[5] + 2                        # outside every band: after the last one, between two
    assert c.end[-1] < last and c.end[5] < gap < gap + 1 < c.begin[6]
    inside = c.begin[6] + 11
    past_end = int(np.flatnonzero(c.rank == c.end[6])[0])  # the point ranked last in its band

    def good():
        _same_bits(_partition(ctx, c), want, "after a refusal")

    good()
    _refused(ctx, c, 147, NEGATIVE, ssi=_with(c.ssi, last, np.nan))                 # the very last index, the last block
    good()
    _refused(ctx, c, 147, NEGATIVE, ssi=_with(c.ssi, inside, -2.0 ** -10))
    good()
    _same_bits(_partition(ctx, c, ssi=_with(_with(c.ssi, last, -0.0), inside, -0.0)),
               K.partition_exact(_with(c.ssi, inside, 0.0), c.rank, c.sv, c.begin, c.end, c.max_range), "-0.0")
    _refused(ctx, c, 147, PERMUTE, rank=_with(c.rank, past_end, c.end[6] + 1))      # one past its band's end
    good()
    _refused(ctx, c, 147, PERMUTE, rank=_with(c.rank, int(np.flatnonzero(c.rank == c.begin[6])[0]), c.begin[6] - 1))
    good()
    _refused(ctx, c, 147, PERMUTE, rank=_with(c.rank, gap, gap + 1))                # outside every band, not its own index
    good()
    _refused(ctx, c, 147, PERMUTE, rank=_with(c.rank, last, 0))
    good()
    _refused(ctx, c, 147, NEGATIVE, ssi=_with(c.ssi, last, np.nan), rank=_with(c.rank, gap, gap + 1))     # both: the irradiance
    good()
    _refused(ctx, c, 147, NAN_SV, sv=_with(c.sv, inside, np.nan))
    good()
    _refused(ctx, c, 147, NAN_SV, sv=_with(c.sv, c.end[-1], np.nan))
    good()
    _refused(ctx, c, 147, PERMUTE, sv=_with(c.sv, inside, np.nan), rank=_with(c.rank, gap, gap + 1))
    good()
    # a NaN sorting variable outside every band is nobody's
    _same_bits(_partition(ctx, c, sv=_with(_with(c.sv, last, np.nan), gap, np.nan)), want, "NaN outside every band")


def test_flag_latches_in_the_second_grid_pass(ctx, geo, grid_cases):
    c, want = grid_cases[0]
    G = geo["grid_points"]
    last, gap, inside = c.ssi.size - 1, c.end[0] + 5, c.begin[1] + 17
    assert gap > G and c.end[0] < gap < c.begin[1] and c.end[1] < last

    def good():
        _same_bits(_partition(ctx, c), want, "after a refusal")

    _refused(ctx, c, 147, NEGATIVE, ssi=_with(c.ssi, last, np.nan))
    good()
    _refused(ctx, c, 147, PERMUTE, rank=_with(c.rank, gap, gap - 1))
    good()
    _refused(ctx, c, 147, PERMUTE, rank=_with(c.rank, inside, c.end[1] + 1))
    good()
    _refused(ctx, c, 147, NAN_SV, sv=_with(c.sv, inside, np.nan))
    good()


def test_band_list_and_range_refusals(ctx, base):
    c, want = base
    n = c.ssi.size
    swapped_b, swapped_e = list(c.begin), list(c.end)
    swapped_b[5], swapped_e[5] = c.end[5], c.begin[5]
    _refused(ctx, c, 147, "contains no wavenumbers", begin=swapped_b, end=swapped_e)                # begin > end
    overlap = list(c.begin)
    overlap[5] = c.end[4]
    _refused(ctx, c, 147, "overlap", begin=overlap)
    _refused(ctx, c, 147, "contains no wavenumbers", end=list(c.end[:-1]) + [n])                    # end >= nwav
    _refused(ctx, c, 147, "contains no wavenumbers", begin=[-1] + list(c.begin[1:]))
    for mr in (0.0, -0.26, np.nan):
        _refused(ctx, c, 147, "max_reflectance_range must be positive", max_range=mr)
    _same_bits(_partition(ctx, c), want, "after the refusals")
    # the last band may end on the last point
    cut = c._replace(ssi=c.ssi[:c.end[-1] + 1], rank=c.rank[:c.end[-1] + 1], sv=c.sv[:c.end[-1] + 1])
    _same_bits(_partition(ctx, cut), want, "no point after the last band")


def test_capacity_refusals(ctx, base):
    c = K.capacity_case()
    want = K.partition_exact(c.ssi, c.rank, c.sv, c.begin, c.end, c.max_range)
    assert want["n_g_points"] == [2, 3]
    _refused(ctx, c, 148, "More than 4 cloud g points", capacity=4)                  # the bands' total
    _refused(ctx, c, 148, "more g points than the 2 allowed", capacity=2)            # nd >= capacity in band 1
    _refused(ctx, c, 148, "More than 3 cloud g points", capacity=3)
    _same_bits(_partition(ctx, c), want, "ng == capacity")
    b, want_b = base
    inside = b.begin[8] + 3
    _refused(ctx, b, 148, "more g points than", sv=_with(b.sv, inside, np.inf))
    _refused(ctx, b, 148, "more g points than", sv=_with(_with(b.sv, inside, np.inf), inside + 1, -np.inf))
    _same_bits(_partition(ctx, b), want_b, "after the refusals")


def test_band_without_irradiance_is_refused(ctx, base):
    """today's behaviour: every boundary of the band is 0, its first g point ends before it begins"""
    c, want = base
    for b in (0, 7):
        ssi = c.ssi.copy()
        ssi[c.begin[b]:c.end[b] + 1] = 0.0
        _refused(ctx, c, 148, "Band %d, g point 0 holds no wavenumber" % b, ssi=ssi)
    _same_bits(_partition(ctx, c), want, "after the refusals")
