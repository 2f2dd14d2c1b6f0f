"""The tile binner of csrc/gpoint_bin.hpp (tile_key, tile_rank, tile_pieces, reduce_batch, k_gpoint_combine, tile_grid,
bin_column_ranges) pinned at its edges, through both kernels that share it and through the launch splits around them.

Shortwave, exactly: with the inputs of gpoint_layouts.sw_inputs() every flux is cos_sza x albedo x ssi - an integer times a
power of two - or exactly 0, so every per-column and broadband sum is a representable number WHATEVER the order of the
additions, and the device's sums are compared with integer sums by ==.  A point that is lost, added twice or added to the wrong
column or row changes an integer.  (The upwelling rows of this scheme are equal at all levels: a swap among them is not seen
here but in test_lbl_gpoint_fluxes_sw_gpu.py, against the oracle.)  This rests on the device's exp() giving exactly 1 at -0.0
and exactly 0 at -1e6 and below.

Longwave: at optical depth 0 the flux that comes down is exactly 0 and every upwelling row holds the same addends in the same
order, so all rows have the same bits; with smooth optical depths on 600-700 cm-1 the sums are compared with the oracle's
fluxes added per column by math.fsum.

The maps are the designed tile layouts of gpoint_layouts.py; test_gpoint_bin_layouts.py shows on the CPU which branches of
the binner they reach."""
import functools
import math

import numpy as np
import pytest
import torch

import gpoint_layouts as L

pytestmark = pytest.mark.gpu


def _dev(ctx, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)


def _gmap(ctx, inp):
    from ecckd_amd import api
    return api.GPointMap(ctx, _dev(ctx, inp.g), inp.ng, _dev(ctx, inp.wn), _dev(ctx, inp.dwn))


def _fused(ctx, case, angles=None):
    """the fused call on the case's inputs -> (dn, up, bb_dn, bb_up)"""
    inp = L.sw_inputs(case)
    gm = _gmap(ctx, inp)
    mu = inp.cos_sza if angles is None else inp.cos_sza[angles]
    out = gm.lbl_fluxes_sw(mu, _dev(ctx, inp.ssi), _dev(ctx, inp.od), _dev(ctx, inp.albedo) if case.albedo else None)
    gm.close()
    return out


def _assert_exact(case, got, angles=None):
    ref = L.sw_reference(case)
    pick = slice(None) if angles is None else angles
    for name, a, b in zip(("dn", "up", "bb_dn", "bb_up"), got, ref):
        b = b[pick]
        assert a.shape == b.shape, (case.name, name)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError("%s %s: %d of %d differ, first at %s: %r instead of %r" %
                                 (case.name, name, len(bad), a.size, bad[0].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


def _assert_other_entry_points(ctx, case, got):
    """The same inputs through ecckd_lbl_spectral_fluxes_sw and ecckd_gmap_sum_rows: the FLOAT rows are the exact spectral
    values, its broadband sums and the per-g sums of its rows are the fused ones, bit for bit."""
    from ecckd_amd import api
    inp = L.sw_inputs(case)
    sdn, sup, sbdn, sbup = api.lbl_spectral_fluxes_sw(ctx, inp.cos_sza, _dev(ctx, inp.ssi), _dev(ctx, inp.od),
                                                      _dev(ctx, inp.albedo) if case.albedo else None)
    xdn, xup = L.sw_spectral(case)
    assert sdn.dtype == torch.float32 and torch.equal(sdn.cpu(), torch.from_numpy(xdn.astype(np.float32)))
    assert torch.equal(sup.cpu(), torch.from_numpy(xup.astype(np.float32)))
    assert np.array_equal(sbdn, got[2]) and np.array_equal(sbup, got[3])
    gm = _gmap(ctx, inp)
    for s in range(case.nsza):
        assert np.array_equal(gm.sum_rows(sdn[s]), got[0][s]) and np.array_equal(gm.sum_rows(sup[s]), got[1][s])
    gm.close()


@pytest.mark.parametrize("case", L.LAYOUT_CASES, ids=lambda c: c.name)
def test_layouts_sweep(ctx, case):
    """Every designed layout (the tile of 256 columns included) in one launch of 301 columns, 3 layers, one angle; with and
    without albedo, FLOAT and DOUBLE optical depths; last tiles of 1, 7, 8, 9 and 255 live lanes."""
    assert L.sw_split(case.nlay, case.nsza, case.ng) == ([1], [(0, 300, True)])
    got = _fused(ctx, case)
    _assert_exact(case, got)
    _assert_other_entry_points(ctx, case, got)


@pytest.mark.parametrize("case", L.ANGLE_CASES, ids=lambda c: c.name)
def test_every_number_of_angles_per_launch(ctx, case):
    """A = 1..8 angles in one launch: 8 / A = 8, 4, 2, 2, 1, 1, 1, 1 levels per batch.  3 layers with albedo are 8 steps: no
    tail batch at any A; 4 layers are 10 or 5 steps: tails for 8, 4 and 2 levels per batch."""
    assert L.sw_split(case.nlay, case.nsza, case.ng) == ([case.nsza], [(0, 7, True)])
    got = _fused(ctx, case)
    _assert_exact(case, got)
    if case.albedo and case.nlay == 4:
        _assert_other_entry_points(ctx, case, got)


@pytest.mark.parametrize("case", L.DEPTH_CASES, ids=lambda c: c.name)
def test_production_depth_angle_splits(ctx, case):
    """54 layers: launches of 8, 7, 6, 5, 4 + 3 and 2 + 2 + 1 angles (the split by the formula of the kernel's header, so a
    change of the budget is noticed); every angle alone gives the bits it has in the call of all."""
    assert L.sw_cap(54) == 67
    assert L.sw_split(54, case.nsza, case.ng) == (L.DEPTH_SPLITS[(case.ng, case.nsza)], [(0, case.ng, True)])
    got = _fused(ctx, case)
    _assert_exact(case, got)
    _assert_other_entry_points(ctx, case, got)
    for s in range(case.nsza):
        one = _fused(ctx, case, angles=[s])
        _assert_exact(case, one, angles=[s])
        for a, b in zip(got, one):
            assert np.array_equal(a[s], b[0])


@pytest.mark.parametrize("case", L.RANGE_CASES, ids=lambda c: c.name)
def test_column_ranges(ctx, case):
    """54 layers, 67 column-angles per launch: ng = 66 is one launch, exactly full; 67 = 66 + 1; 133 = 66 + 67, the last pass
    exactly full; 134 = 66 + 67 + 1; two angles, so every range is used once per angle."""
    angles, ranges = L.sw_split(54, case.nsza, case.ng)
    assert angles == [1, 1] and [n for _, n, _ in ranges] == L.RANGE_SPLITS[case.ng]
    got = _fused(ctx, case)
    _assert_exact(case, got)
    _assert_other_entry_points(ctx, case, got)
    one = _fused(ctx, case, angles=[1])
    for a, b in zip(got, one):
        assert np.array_equal(a[1], b[0])


def test_several_tiles_per_block(ctx):
    """1 049 421 points: 4100 tiles, 3 per block, 1367 blocks; the last block has 2 tiles (the loop's break is taken), the
    second with 77 live lanes."""
    case = L.BIG_CASE
    assert L.tile_grid(L.sw_inputs(case).nwav) == (3, 1367)
    got = _fused(ctx, case)
    _assert_exact(case, got)
    _assert_other_entry_points(ctx, case, got)


@pytest.mark.parametrize("case", L.TINY_CASES, ids=lambda c: c.name)
def test_tiny_spectra(ctx, case):
    """1, 255, 256 and 257 wavenumbers"""
    got = _fused(ctx, case)
    _assert_exact(case, got)
    _assert_other_entry_points(ctx, case, got)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_sum_rows_at_its_chunk_edges(ctx, dtype):
    """ecckd_gmap_sum_rows adds a g point in chunks of 2048 sorted positions: g points of 0, 1, 2047, 2048, 2049, 4096 and
    4097 wavenumbers, interleaved in natural order among 500 points without a g point; integer rows below 2^24 (exact as FLOAT;
    a sum stays below 2^37) with a row stride larger than nwav, against integer sums."""
    counts = [0, 1, L.GA_CHUNK - 1, L.GA_CHUNK, L.GA_CHUNK + 1, 2 * L.GA_CHUNK, 2 * L.GA_CHUNK + 1]
    rng = np.random.default_rng(77)
    g = rng.permutation(np.concatenate([np.full(n, ig) for ig, n in enumerate(counts)] + [np.full(500, -1)])).astype(np.int32)
    nwav, ng, nrows = g.size, len(counts), 3
    rows = rng.integers(0, 2 ** 24, size=(nrows, nwav))
    want = np.stack([[int(r[g == ig].sum()) for ig in range(ng)] for r in rows])
    wn = np.linspace(600.0, 700.0, nwav)
    inp = L.SwInputs(g, ng, nwav, wn, np.full(nwav, 100.0 / (nwav - 1)), None, None, None, None, None)
    gm = _gmap(ctx, inp)
    assert gm.counts().tolist() == counts
    wide = torch.zeros((nrows, nwav + 37), dtype=getattr(torch, dtype), device=ctx.device)
    wide[:, nwav:] = 1.0e6                                   # (what lies past the row must not be added)
    wide[:, :nwav] = _dev(ctx, rows.astype(dtype))
    for d_rows in (wide[:, :nwav], wide[:, :nwav].contiguous()):
        assert d_rows.stride(0) in (nwav, nwav + 37)
        got = gm.sum_rows(d_rows)
        assert np.array_equal(got, want.astype(np.float64))
    gm.close()


# ------------------------------------------------------------------------------------------------------------- longwave
def _lw(ctx, inp, od):
    gm = _gmap(ctx, inp)
    out = gm.lbl_fluxes_lw(inp.t_hl, _dev(ctx, od))
    gm.close()
    return out


@pytest.mark.parametrize("case", L.LW_SMALL_CASES, ids=lambda c: c.name)
def test_longwave_rows_are_equal_at_zero_optical_depth(ctx, case):
    """1, 2, 3 and 4 layers: 3, 5, 7 and 1 rows in the tail batch.  Nothing absorbs and nothing emits: the flux down is exactly
    0, and the surface emission arrives at every level unchanged - every upwelling row is the sum of the same addends in the
    same order, per column and broadband, so a row that the tail drops or takes from the wrong slot differs from the others."""
    inp = L.lw_inputs(case)
    dn, up, bdn, bup = _lw(ctx, inp, np.zeros_like(inp.od))
    assert dn.shape == up.shape == (case.nlay + 1, inp.ng)
    assert not dn.any() and not bdn.any()
    for lev in range(case.nlay + 1):
        assert np.array_equal(up[lev], up[case.nlay]) and bup[lev] == bup[case.nlay], lev
    owned = np.bincount(inp.g[inp.g >= 0], minlength=inp.ng) > 0
    assert np.all(up[:, owned] > 0.0) and not up[:, ~owned].any() and not owned[L.case_spectrum(case).empty_g]


@functools.lru_cache(maxsize=None)
def _lw_oracle_sums(case):
    """per column (g points, then the points without one) and row, math.fsum of the oracle's spectral fluxes"""
    import pyoracle as oracle
    inp = L.lw_inputs(case)
    planck = oracle.planck_function(inp.t_hl, inp.wn, inp.dwn)
    fdn, fup = oracle.radiative_transfer_lw(planck, inp.od.astype(np.float64), np.ones(inp.nwav), planck[-1])
    col = np.where(inp.g < 0, inp.ng, inp.g)
    order = np.argsort(col, kind="stable")
    edges = np.searchsorted(col[order], np.arange(inp.ng + 2))
    out = []
    for f in (fdn, fup):
        rows = f[:, order].tolist()
        per = np.array([[math.fsum(r[edges[c]:edges[c + 1]]) for c in range(inp.ng + 1)] for r in rows])
        out += [per[:, :inp.ng], np.array([math.fsum(r) for r in rows])]
    return out[0], out[2], out[1], out[3]


@pytest.mark.parametrize("case", L.LW_CASES, ids=lambda c: c.name)
def test_longwave_against_the_oracle(ctx, oracle, case):
    """The same maps through k_lbl_gpoint_fluxes_lw (its own row_of and tail): 1..4 layers in one launch of 301 columns; 54
    layers with 47, 48, 95 and 96 g points (48 columns per launch: one full launch, 47 + 1, 47 + 48, 47 + 48 + 1); three tiles
    per block.  rtol 1e-10 is that of test_lbl_gpoint_fluxes_gpu.py::test_against_the_oracle for the same arithmetic against
    the same oracle functions; one point lost or misplaced among the N <= 70 000 of a column moves its sum by about 1 / N."""
    inp = L.lw_inputs(case)
    if case.kind == "lw_ranges":
        assert [n for _, n, _ in L.lw_ranges(case.nlay, case.ng)] == L.LW_RANGE_SPLITS[case.ng]
    got = _lw(ctx, inp, inp.od)
    ref = _lw_oracle_sums(case)
    worst = 0.0
    for name, a, b in zip(("dn", "up", "bb_dn", "bb_up"), got, ref):
        worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))
    print(case.name, "nwav", inp.nwav, "largest relative difference", worst)
    for a, b in zip(got, ref):
        assert np.allclose(a, b, rtol=1e-10, atol=1e-300)
    assert not got[0][0].any() and got[2][0] == 0.0           # nothing comes down at the top
