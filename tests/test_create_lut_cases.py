"""CPU checks of the inputs and of the extended-precision reference of test_create_lut_edges_gpu.py (create_lut_cases.py):
the numbers the layouts are designed for are still those of csrc/create_lut.hip, the layouts give the chunk counts they are
meant to give, the designed inputs are what they say, and the reference - written from the formulas - agrees with the
double-precision oracle (oracle_lut.c) on the EDGE inputs under every method, both precisions and every designed branch,
within the bound the device is held to: 64 eps max(1, condition) (create_lut_cases.fit_bound)."""
import math
import os
import re

import numpy as np
import pytest

import create_lut_cases as K

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ecckd_amd", "csrc")


def test_the_constants_are_those_of_the_source():
    src = ""
    for name in ("create_lut.hip", "gmap_layout.hpp"):          # the kernels; the chunk constants and the chunking
        with open(os.path.join(CSRC, name)) as f:
            src += f.read()

    def const(name):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % name, src)
        assert m, name
        return m.group(1).strip()

    assert const("GA_THREADS") == "256" and K.GA_THREADS == 256
    assert const("GA_PPT") == "8" and K.GA_PPT == 8
    assert const("GA_CHUNK") == "GA_THREADS * GA_PPT" and K.GA_CHUNK == 2048
    # the one lane-strided loop that combines chunk partials (combine_chunks), and nowhere another stride
    strides = re.findall(r"for \(int c = [^;]+; c < [^;]+; c \+= (\w+)\)", src)
    assert strides == [str(K.FINAL_LANES)], strides
    assert "for (int t = tid; t < nlay * 6; t += GA_THREADS)" in src
    assert "for (; i + 192 < hi; i += 256)" in src and "for (; i < hi; i += 64)" in src
    import test_create_lut_gpu
    assert K.METHODS == test_create_lut_gpu.METHODS


@pytest.mark.parametrize("name", sorted(K.LAYOUTS))
def test_layouts_give_the_intended_chunks(name):
    counts, none = K.LAYOUTS[name]
    g = K.layout_g(name)
    assert g.size == sum(counts) + none and g.dtype == np.int32
    assert np.bincount(g[g >= 0], minlength=len(counts)).tolist() == counts and np.count_nonzero(g < 0) == none
    assert K.chunks_of(counts) == K.CHUNKS[name]
    if name == "NONE_ONLY":
        assert sum(K.chunks_of(counts)) == 0
        return
    # whole runs of varying length are interleaved: the natural order is not the sorted order
    edges = np.flatnonzero(np.diff(g)) + 1
    runs = np.diff(np.concatenate([[0], edges, [g.size]]))
    assert np.unique(runs).size > 20 and runs.max() >= max(counts) // 80 and np.any(np.diff(g) < 0)
    first = [int(np.flatnonzero(g == ig)[0]) for ig, n in enumerate(counts) if n]
    assert first != sorted(first)
    wn, dwn = K.grid(g.size)
    assert np.all(np.diff(wn) > 0) and np.all((wn - 600.0) * 64 == np.arange(g.size))
    assert set(np.unique(dwn).tolist()) == set(range(1, 9))


def test_the_stride_layout_reaches_the_second_trip():
    """chunks c0 + lane, c0 + lane + 64: 64 chunks are one trip of every lane, 65 and 66 a second trip of lanes 0 and 0, 1"""
    assert K.CHUNKS["STRIDE"] == [64, 64, 65, 66, 1]
    counts = K.LAYOUTS["STRIDE"][0]
    assert [n % K.GA_CHUNK for n in counts] == [K.GA_CHUNK - 1, 0, 1, 1, 3]
    assert [max(0, c - K.FINAL_LANES) for c in K.CHUNKS["STRIDE"]] == [0, 0, 1, 2, 0]
    # the second trip of the LDS combine of k_gavg_partial needs nlay * 6 > GA_THREADS
    assert [n * 6 > K.GA_THREADS for n in (3, 42, 43, 54)] == [False, False, True, True]


@pytest.mark.parametrize("nlay", [3, 42, 43, 54])
def test_pressure_grid_has_a_layer_at_exactly_100_hpa(nlay):
    p = K.pressure_grid(nlay)
    assert p.size == nlay + 1 and np.all(np.diff(p) > 0)
    at = K.layer_at_100hpa(p)
    pfl = 0.5 * (p[1:] + p[:-1])
    assert pfl[at] == 10000.0 and pfl[at - 1] < 10000.0 < pfl[at + 1]
    m = K.layer_methods("hybrid-logarithmic-transmission-3", p)
    assert m[at] == "transmission-3" and m[at - 1] == "transmission-3" and m[at + 1] == "logarithmic"


def test_isolated_map_keeps_the_segment_and_moves_it():
    g = K.layout_g("EDGE")
    wn = K.grid(g.size)[0]
    for ig in (K.G_SINGLE, K.G_PARTLY_ZERO, K.G_SATURATED, K.G_SMOOTH):
        pos, g2 = K.isolated(g, ig)
        assert np.array_equal(pos[g2 == ig], np.flatnonzero(g == ig)) and set(np.unique(g2).tolist()) == {-1, ig}
        assert np.all(np.diff(wn[pos]) > 0) and pos.size < g.size
        # other natural positions, and another begin of the segment in the sorted order
        assert not np.array_equal(np.flatnonzero(g2 == ig), np.flatnonzero(g == ig))
        assert np.count_nonzero((g >= 0) & (g < ig)) > 0 or ig == K.G_SINGLE          # (only an empty g point precedes it)


def test_designed_optical_depths_are_what_they_say():
    g = K.layout_g("EDGE")
    for dtype in ("float32", "float64"):
        od = K.optical_depth("EDGE", 54, "designed-fltmax", dtype)
        assert od.dtype == np.dtype(dtype) and np.all(np.isfinite(od)) and od.min() == 0.0
        part = od[:, g == K.G_PARTLY_ZERO]
        zero_cols = np.all(part == 0, axis=0)
        assert np.all(zero_cols[::4]) and 0.25 <= zero_cols.mean() < 0.35
        assert np.array_equal(part == 0, np.broadcast_to(zero_cols, part.shape))
        assert not od[:, g == K.G_ALL_ZERO].any()
        const = od[:, g == K.G_CONSTANT]
        assert np.all(const == const[:, :1]) and np.all(const > 0)
        sat = od[:, g == K.G_SATURATED]
        assert sat.min() >= 1.0e3 and np.all((sat == K.FLT_MAX).sum(1) == 1)
        assert K.optical_depth("EDGE", 54, "designed", dtype)[:, g == K.G_SATURATED].max() <= 1.0e4
        assert np.all(od[:, g == K.G_SINGLE] > 0)
        # exp(-1e3 * 1.66) is 0 in double: every transmission term of the saturated g point is exactly 1
        assert math.exp(-1.0e3 * K.LW_DIFFUSIVITY) == 0.0


def test_width_intervals_cut_the_designed_runs():
    for name, ig in (("EDGE", K.G_SMOOTH), ("STRIDE", 0)):
        g = K.layout_g(name)
        wn, dwn = K.grid(g.size)
        w1, w2, want = K.width_intervals(g, wn, ig)
        s = wn[g == ig]
        got = [int(np.count_nonzero((s > a) & (s <= b))) for a, b in zip(w1, w2)]
        assert got == want and want[1:1 + len(K.RUNS)] == list(K.RUNS) and len(w1) == 15
        assert np.all(np.isin(w1[1:-1], s)) and np.all(np.isin(w2[:-2], s))       # the bounds lie ON wavenumbers
        assert w1[1] == w2[1]                                                      # (w, w] is empty
        frac, width, total = K.fraction_reference(g, K.layout_ng(name), wn, dwn, w1, w2)
        assert np.array_equal(width[:, -1], total) and total.sum() == dwn[g >= 0].sum()
        assert np.array_equal(width[:, :-1].sum(1), total)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", ["EDGE", "NONE_ONLY"])
def test_fraction_reference_is_the_oracles(oracle, name):
    g = K.layout_g(name)
    ng = K.layout_ng(name)
    wn, dwn = K.grid(g.size)
    if name == "EDGE":
        w1, w2, _ = K.width_intervals(g, wn, K.G_SMOOTH)
    else:
        w1, w2 = np.array([599.0, 601.0]), np.array([601.0, 700.0])
    frac = K.fraction_reference(g, ng, wn, dwn, w1, w2)[0]
    assert _same(frac, oracle.gpoint_fraction(ng, g, wn, dwn, w1, w2))
    empty = np.array(K.LAYOUTS[name][0]) == 0
    assert np.all(np.isnan(frac[empty])) and np.all(np.isfinite(frac[~empty]))
    if name == "EDGE":
        assert np.all(frac[~empty, -1] == 1.0)


def _weights(kind, p, nwav):
    """(the reference's weights in extended precision, the oracle's (nlay, nwav) in double)"""
    wn, dwn = K.grid(nwav)
    if kind == "lw":
        import pyoracle
        t_fl = K.temperature_fl(p)
        return K.planck_terms(t_fl, wn, dwn), pyoracle.planck_function(t_fl, wn, dwn)
    ssi = K.ssi_weights(nwav)
    return ssi.astype(K.X), np.tile(ssi, (p.size - 1, 1))


@pytest.mark.parametrize("weights", ["lw", "ssi"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("variant,nlay", [("smooth", 43), ("designed", 54), ("designed-fltmax", 54)])
def test_average_reference_against_the_oracle(oracle, variant, nlay, dtype, weights):
    """Every method on the EDGE inputs.  Every cell of the reference is finite; the oracle's fit is within the bound of it,
    its min and max are equal to it; with reference_surface_vmr > 0 all three within a few eps more."""
    g, ng = K.layout_g("EDGE"), K.layout_ng("EDGE")
    p = K.pressure_grid(nlay)
    od = K.optical_depth("EDGE", nlay, variant, dtype)
    wx, wd = _weights(weights, p, g.size)
    assert np.all(wd > 0)
    for method in K.METHODS:
        ref = K.average_reference(g, ng, p, od, method, wx)
        for a in ref:
            assert np.all(np.isfinite(a.astype(np.float64))), method
        oma, omn, omx, ne = oracle.average_optical_depth_to_g_point(ng, -1.0, p, g, od.astype(np.float64), wd, method)
        assert ne == 2
        if variant == "designed-fltmax" and method == "square-root":
            # One term of the saturated g point is sqrt(FLT_MAX) w = 1.8e19 w, the other 4095 are below 100 w: less than half
            # an ulp of the sum, so the oracle's index-order additions drop every one of them and miss the bound - that is
            # its own summation.  Its TERMS added with math.fsum are held to the bound instead.
            idx = g == K.G_SATURATED
            for l in range(nlay):
                w = wd[l, idx]
                v = math.fsum((np.sqrt(od[l, idx].astype(np.float64)) * w).tolist()) / math.fsum(w.tolist())
                oma[l, K.G_SATURATED] = v * v
        assert np.array_equal(omn, ref.mn) and np.array_equal(omx, ref.mx), method
        err = K.relative_error(oma, ref.fit)
        bound = K.fit_bound(ref)
        print("%-34s %s %s %s nlay %d: largest error / (eps max(1, cond)) %.2f, / bound %.3f" %
              (method, variant, dtype, weights, nlay, np.max(err / (K.EPS * ref.cond)), np.max(err / bound)))
        assert np.all(err <= bound), (method, np.argwhere(err > bound)[:5].tolist())
        # as molar absorption
        sma, smn, smx, _ = oracle.average_optical_depth_to_g_point(ng, 4.0e-4, p, g, od.astype(np.float64), wd, method)
        scale = K.molar_scale(p, 4.0e-4)[:, None]
        if not (variant == "designed-fltmax" and method == "square-root"):
            assert np.all(K.relative_error(sma, ref.fit * scale) <= bound + 4 * K.EPS)
        assert np.all(K.relative_error(smn, ref.mn.astype(K.X) * scale) <= 4 * K.EPS)
        assert np.all(K.relative_error(smx, ref.mx.astype(K.X) * scale) <= 4 * K.EPS)
        if variant != "smooth":
            K.assert_branches(method, p, od, g, ref.fit.astype(np.float64), ref.mn, ref.mx)


@pytest.mark.parametrize("nlut", [1, 4, 231])
def test_planck_lut_reference_against_the_oracle(oracle, nlut):
    g, ng = K.layout_g("EDGE"), K.layout_ng("EDGE")
    wn, dwn = K.grid(g.size)
    t = np.arange(120.0, 351.0)[:nlut] if nlut > 1 else np.array([287.5])
    ref = K.planck_lut_reference(g, ng, t, wn, dwn)
    got = oracle.planck_lut(ng, t, g, wn, dwn)
    assert np.all(np.isfinite(ref.astype(np.float64))) and not ref[:, [0, 7]].any() and not got[:, [0, 7]].any()
    err = K.relative_error(got, ref)
    print("planck_lut nlut %d: largest error / eps %.2f" % (nlut, err.max() / K.EPS))
    assert np.all(err <= 64 * K.EPS)


def test_erythemal_reference_against_double_terms():
    """there is no oracle function: the formula in double, added with math.fsum"""
    g, ng = K.layout_g("EDGE"), K.layout_ng("EDGE")
    wn, dwn = K.erythemal_grid(g.size)
    ref = K.erythemal_reference(g, ng, wn, dwn)
    wl = 1.0e7 / wn
    ery = np.zeros(wn.size)
    ery[(wl > 250.0) & (wl <= 298.0)] = 1.0
    m = (wl > 298.0) & (wl <= 328.0)
    ery[m] = 10.0 ** (0.094 * (298.0 - wl[m]))
    m = (wl > 328.0) & (wl <= 400.0)
    ery[m] = 10.0 ** (0.015 * (140.0 - wl[m]))
    assert ery.min() == 0.0 and ery.max() == 1.0 and np.count_nonzero((ery > 0) & (ery < 1)) > 1000
    import pyoracle
    pl = pyoracle.planck_function([5777.0], wn, dwn)[0]
    for ig in range(ng):
        idx = g == ig
        if not idx.any():
            assert np.isnan(ref[ig])
            continue
        want = math.fsum((np.sqrt(ery[idx]) * pl[idx]).tolist()) / math.fsum(pl[idx].tolist())
        assert 0.0 < ref[ig] <= 1.0 and K.relative_error(want, ref[ig]) <= 64 * K.EPS


def test_stride_reference_against_fsum_of_the_oracles_terms(oracle):
    """STRIDE: the oracle adds 130 000 terms in index order in double, which costs it more than the bound; its TERMS (the
    Planck function of oracle_rt.c, times the optical depth) added with math.fsum are held to it.  One temperature, the
    linear average of one layer, every g point."""
    g, ng = K.layout_g("STRIDE"), K.layout_ng("STRIDE")
    wn, dwn = K.grid(g.size)
    p = K.pressure_grid(3)
    od = K.optical_depth("STRIDE", 3, "smooth", "float32")
    t_fl = K.temperature_fl(p)
    pl = oracle.planck_function(t_fl[1:2], wn, dwn)[0]
    lut = K.planck_lut_reference(g, ng, t_fl[1:2], wn, dwn)[0]
    ref = K.average_reference(g, ng, p[1:3], od[1:2], "linear", K.planck_terms(t_fl[1:2], wn, dwn))
    for ig in range(ng):
        idx = g == ig
        den = math.fsum(pl[idx].tolist())
        num = math.fsum((od[1, idx].astype(np.float64) * pl[idx]).tolist())
        assert K.relative_error(den, lut[ig]) <= 64 * K.EPS
        assert K.relative_error(num / den, ref.fit[0, ig]) <= 64 * K.EPS


def test_the_regrowth_calls_grow_the_work_buffer():
    """gmap_work() regrows when a call needs more than every call before it: the sequence of the regrowth test does so twice
    after the first allocation, and ends with calls that fit"""
    nchunk, ng = sum(K.CHUNKS["EDGE"]), K.layout_ng("EDGE")
    need = [K.work_bytes(call, nchunk, ng, n) for call, n in K.REGROWTH_CALLS]
    grows = [b > max(need[:i], default=0) for i, b in enumerate(need)]
    assert grows == [True, False, True, True, False, False], need
