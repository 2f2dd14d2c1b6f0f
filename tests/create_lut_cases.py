"""Inputs and an extended-precision reference for the segmented reductions of csrc/create_lut.hip (K6/K7): the g-point
averages under every averaging method, the Planck look-up table, the g-point fractions and the erythemal weights
(test_create_lut_cases.py on the CPU, test_create_lut_edges_gpu.py on the device).  numpy only.

Every kernel of that file reduces a g point - a contiguous segment of the g-sorted order - in three levels: a block of
GA_THREADS threads takes a chunk of GA_CHUNK sorted positions, GA_PPT per thread (chunk_positions); its four waves meet in
LDS (block_sum_256 of rt_device.hpp; in k_gavg_partial after the last layer); a second kernel - k_gavg_final for the averages,
k_combine_chunks for everything else - adds the chunk partials of a g point, lane j taking the chunks j, j + 64, ...
(combine_chunks).  What a segment goes through is decided by its
number of points alone, so a LAYOUT is the list of the g points' counts.  layout_g() hands out natural positions run by run
(runs of varying length, g points and points without one interleaved by a seeded permutation): the wavenumbers ascend in
natural order, so they ascend inside every g point, as ecckd_gmap_create demands.

The numbers of the kernels that the layouts are written for are repeated here (test_create_lut_cases.py reads them out of
the source - create_lut.hip and gmap_layout.hpp, which holds the chunk constants, the chunking and the sizes of the work
buffer - and fails when they differ; tools/check_gmap_layout.cpp holds gmap_layout.hpp to CHUNKS and to work_bytes()).

The reference restates the formulas of average_optical_depth_to_g_point, planck_function, the g-point fraction and the
erythemal weight - not the oracle's code -: every term is computed in np.longdouble (64-bit mantissa; np.expm1 / np.log1p
where a 1 is added or taken away) and added in np.longdouble.  Where the platform's long double is no wider than double,
the terms are doubles and are added with math.fsum.  The inputs (wavenumbers, temperatures, pressures, optical depths as
stored) and the constants of the formulas as doubles are taken as exact."""
import functools
import math
from collections import namedtuple

import numpy as np

GA_THREADS = 256
GA_PPT = 8
GA_CHUNK = GA_THREADS * GA_PPT      # 2048 sorted positions per block
FINAL_LANES = 64                    # combine_chunks (k_gavg_final, k_combine_chunks): lane j adds the chunks j, j + 64, ...

METHODS = ["linear", "transmission", "transmission-2", "transmission-3", "transmission-10", "square-root",
           "logarithmic", "hybrid-logarithmic-transmission-3"]
TRANSMISSION_K = {"transmission": 1.0, "transmission-2": 2.0, "transmission-3": 3.0, "transmission-10": 10.0}

LW_DIFFUSIVITY = 1.66
ACCEL_GRAVITY = 9.80665
MOLAR_MASS_DRY_AIR = 28.970
PLANCK_H = 6.62606896e-34
LIGHT_C = 2.99792458e8
BOLTZMANN_K = 1.3806504e-23
PI = 3.14159265358979323846
CLAMP = 0.9999999999999999           # the largest "1 - transmission" the transmission methods invert
FLT_MAX = float(np.finfo(np.float32).max)

EPS = float(np.finfo(np.float64).eps)
EXTENDED = bool(np.finfo(np.longdouble).eps < 1e-18)
X = np.longdouble if EXTENDED else np.float64


def xsum(a):
    """the sum of a 1-d array of terms: in long double, or by math.fsum where long double is double"""
    if EXTENDED:
        return np.sum(a, dtype=np.longdouble)
    return np.float64(math.fsum(a.tolist()))


# ---------------------------------------------------------------------------------------------------------------- layouts
# name -> (points of every g point, points without a g point)
LAYOUTS = {
    # a leading and a trailing empty g point; one point; one short of a chunk, a chunk, one over; two chunks, one over
    "EDGE": ([0, 1, GA_CHUNK - 1, GA_CHUNK, GA_CHUNK + 1, 2 * GA_CHUNK, 2 * GA_CHUNK + 1, 0], 300),
    # 64 chunks with a short last one; exactly 64: one trip of the lane-strided loops with every lane busy; 65 with a
    # one-point tail: lane 0 makes a second trip; 66 with a one-point tail: lanes 0 and 1 do; three points
    "STRIDE": ([FINAL_LANES * GA_CHUNK - 1, FINAL_LANES * GA_CHUNK, FINAL_LANES * GA_CHUNK + 1,
                (FINAL_LANES + 1) * GA_CHUNK + 1, 3], 500),
    # no point has a g point: no chunk at all
    "NONE_ONLY": ([0, 0, 0], 300),
}
CHUNKS = {"EDGE": [0, 1, 1, 1, 2, 2, 3, 0], "STRIDE": [64, 64, 65, 66, 1], "NONE_ONLY": [0, 0, 0]}


def chunks_of(counts):
    return [-(-n // GA_CHUNK) for n in counts]


def split_runs(n, rng, longest):
    out = []
    while n > 0:
        out.append(int(min(n, rng.integers(1, longest + 1))))
        n -= out[-1]
    return out


def interleave(counts, none, seed):
    """g_point in natural order: every g point's points in runs of 1..max(9, count / 40) points, the points without a g point in
    runs of 1..9, the runs shuffled"""
    rng = np.random.default_rng(seed)
    runs = []
    for ig, n in enumerate(counts):
        runs += [(ig, r) for r in split_runs(n, rng, max(9, n // 40))]
    runs += [(-1, r) for r in split_runs(none, rng, 9)]
    return np.concatenate([np.full(runs[k][1], runs[k][0], dtype=np.int32) for k in rng.permutation(len(runs))])


@functools.lru_cache(maxsize=None)
def layout_g(name):
    counts, none = LAYOUTS[name]
    g = interleave(counts, none, 4242 + len(counts))
    g.setflags(write=False)
    return g


def layout_ng(name):
    return len(LAYOUTS[name][0])


def isolated(g, ig, keep_every=3):
    """The natural positions of a second map that holds g point `ig` alone: all its points, and every keep_every-th of the
    others, which lose their g point.  -> (positions into the first map's arrays, g_point of the second map)"""
    other = np.flatnonzero(g != ig)[::keep_every]
    pos = np.sort(np.concatenate([np.flatnonzero(g == ig), other]))
    return pos, np.where(g[pos] == ig, ig, -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def grid(nwav, lo=600.0):
    """wavenumbers lo + j / 64 and widths that are integers in [1, 8]: every sum of widths is exact in any order.  (From 600
    cm-1 on and below 350 K, h nu / k T >= 2.4: no cancellation in exp(x) - 1.)"""
    wn = lo + np.arange(nwav) / 64.0
    dwn = np.random.default_rng(nwav).integers(1, 9, size=nwav).astype(np.float64)
    for a in (wn, dwn):
        a.setflags(write=False)
    return wn, dwn


@functools.lru_cache(maxsize=None)
def erythemal_grid(nwav):
    """500 nm .. 222 nm: the three branches of the action spectrum and the zeros on both sides of it"""
    wn = 20000.0 + np.arange(nwav) * (25000.0 / nwav)
    return wn, grid(nwav)[1]


def pressure_grid(nlay):
    """Half levels with 9000 and 11000 Pa next to each other: that layer's full-level pressure is exactly 10000 Pa, the layer
    above it has 8000 and the layer below it 12000."""
    if nlay == 3:
        return np.array([7000.0, 9000.0, 11000.0, 13000.0])
    assert nlay >= 12
    low = [9000.0, 11000.0, 13000.0, 20000.0, 35000.0, 50000.0, 70000.0, 85000.0, 101325.0]
    return np.concatenate([np.geomspace(1.0, 7000.0, nlay + 1 - len(low)), low])


def layer_at_100hpa(p_hl):
    pfl = 0.5 * (p_hl[1:] + p_hl[:-1])
    at = np.flatnonzero(pfl == 100.0e2)
    assert at.size == 1
    return int(at[0])


def temperature_fl(p_hl):
    from ecckd_amd import synthetic as syn
    t_hl = syn.temperature_profile(p_hl)
    return 0.5 * (t_hl[:-1] * p_hl[:-1] + t_hl[1:] * p_hl[1:]) / (0.5 * (p_hl[:-1] + p_hl[1:]))


def ssi_weights(nwav):
    from ecckd_amd import synthetic as syn
    wn, dwn = grid(nwav)
    return syn.solar_spectral_irradiance(wn, dwn)


# the designed g points of EDGE
G_SINGLE, G_PARTLY_ZERO, G_ALL_ZERO, G_CONSTANT, G_SATURATED, G_SMOOTH = 1, 2, 3, 4, 5, 6
VARIANTS = ("smooth", "designed", "designed-fltmax")


@functools.lru_cache(maxsize=6)
def optical_depth(name, nlay, variant="smooth", dtype="float32"):
    """(nlay, nwav) as stored (FLOAT or DOUBLE).  "smooth": the synthetic column of conftest.make_lw_case, its ~5 % all-zero
    wavenumbers included; the single point of EDGE is positive.  "designed" (EDGE): on top of it
      g point 2   every fourth of its points is exactly 0 in every layer          logarithmic: exp(num / den_nz) * (cnt / ntot)
      g point 3   all zeros                                                       every method gives 0
      g point 4   one value per layer                                             min >= max: min * 0.99, max * 1.01
      g point 5   1e3 .. 1e4: every transmission is 0                             num == den: the clamp, then fit = min
    "designed-fltmax": one point per layer of g point 5 holds the largest finite FLOAT."""
    from conftest import make_lw_case
    g = layout_g(name)
    nwav = g.size
    od = make_lw_case(nwav, nlay=nlay, seed=61, dtype="float64", lo=600.0, hi=600.0 + nwav / 64.0)[3]
    lay = np.arange(nlay)
    if name == "EDGE":
        od[:, g == G_SINGLE] = (0.3 + 0.01 * lay)[:, None]
    if variant != "smooth":
        assert name == "EDGE" and variant in VARIANTS
        od[:, np.flatnonzero(g == G_PARTLY_ZERO)[::4]] = 0.0
        od[:, g == G_ALL_ZERO] = 0.0
        od[:, g == G_CONSTANT] = (0.125 * (lay + 1))[:, None]
        idx = np.flatnonzero(g == G_SATURATED)
        od[:, idx] = 1.0e3 * (1.0 + 9.0 * np.random.default_rng(5).uniform(size=(nlay, idx.size)))
        if variant == "designed-fltmax":
            od[lay, idx[(7 * lay + 3) % idx.size]] = FLT_MAX
    od = od.astype(dtype)
    od.setflags(write=False)
    return od


# --------------------------------------------------------------------------------------------------------------- reference
def planck_terms(temperature, wn, dwn):
    """planck_function: (nt, n) terms  d_wavenumber 2 h (100 c) pi / c^2  nu^3 / (exp(h nu / k T) - 1),  nu = 100 c wavenumber"""
    inv_cm_2_hz = X(100.0) * X(LIGHT_C)
    freq = wn.astype(X) * inv_cm_2_hz
    pref = dwn.astype(X) * X(2.0) * X(PLANCK_H) * inv_cm_2_hz * X(PI) / (X(LIGHT_C) * X(LIGHT_C)) * (freq * freq * freq)
    x = (X(PLANCK_H) / X(BOLTZMANN_K)) * freq[None, :] / np.asarray(temperature, dtype=np.float64).astype(X)[:, None]
    return pref[None, :] / np.expm1(x)


def planck_lut_reference(g, ng, temperature_lut, wn, dwn):
    """(nlut, ng) in extended precision; an empty g point has 0"""
    out = np.zeros((len(temperature_lut), ng), dtype=X)
    for ig in range(ng):
        idx = np.flatnonzero(g == ig)
        if idx.size:
            terms = planck_terms(temperature_lut, wn[idx], dwn[idx])
            out[:, ig] = [xsum(row) for row in terms]
    return out


def fraction_reference(g, ng, wn, dwn, w1, w2):
    """(ng, nint): the widths are integers, so the sums are exact and the fraction is the correctly rounded quotient; an
    empty g point has 0 / 0"""
    assert np.array_equal(dwn, np.rint(dwn)) and dwn.sum() < 2.0 ** 53
    have = g >= 0
    total = np.bincount(g[have], weights=dwn[have], minlength=ng)
    width = np.empty((ng, len(w1)))
    for i, (a, b) in enumerate(zip(w1, w2)):
        m = have & (wn > a) & (wn <= b)
        width[:, i] = np.bincount(g[m], weights=dwn[m], minlength=ng)
    with np.errstate(invalid="ignore", divide="ignore"):
        return width / total[:, None], width, total


def erythemal_reference(g, ng, wn, dwn):
    """sqrt of the erythemal action spectrum, weighted by the 5777 K Planck function; (ng,) extended, 0 / 0 where empty"""
    wl = X(1.0e7) / wn.astype(X)
    ery = np.zeros(wn.size, dtype=X)
    ery[(wl > 250.0) & (wl <= 298.0)] = 1.0
    m = (wl > 298.0) & (wl <= 328.0)
    ery[m] = np.power(X(10.0), X(0.094) * (X(298.0) - wl[m]))
    m = (wl > 328.0) & (wl <= 400.0)
    ery[m] = np.power(X(10.0), X(0.015) * (X(140.0) - wl[m]))
    ery = np.sqrt(ery)
    pl = planck_terms([5777.0], wn, dwn)[0]
    out = np.full(ng, np.nan, dtype=X)
    for ig in range(ng):
        idx = np.flatnonzero(g == ig)
        if idx.size:
            out[ig] = xsum(ery[idx] * pl[idx]) / xsum(pl[idx])
    return out


AvgRef = namedtuple("AvgRef", "fit mn mx cond cancel")


def layer_methods(method, p_hl):
    if method != "hybrid-logarithmic-transmission-3":
        return [method] * (len(p_hl) - 1)
    pfl = 0.5 * (p_hl[1:] + p_hl[:-1])
    return ["logarithmic" if p > 100.0e2 else "transmission-3" for p in pfl]


def average_reference(g, ng, p_hl, od, method, weight):
    """average_optical_depth_to_g_point as plain optical depth (reference_surface_vmr <= 0).  weight: (nlay, nwav) or (nwav,)
    in extended precision.  -> AvgRef of (nlay, ng) arrays: fit (extended); mn, mx (double: copies of inputs, or their double
    products with 0.99 and 1.01); cond, the condition number of the fit with respect to a relative error of its sums; cancel,
    for the transmission methods 1 / v (v = num / den): the terms 1 - exp(-x) are formed in double with an absolute error of
    up to eps / 2 (1 + term), which is a relative error of the sum num of up to eps / 2 (1 + 1 / v)."""
    nlay = od.shape[0]
    methods = layer_methods(method, np.asarray(p_hl, dtype=np.float64))
    fit = np.zeros((nlay, ng), dtype=X)
    mn, mx = np.zeros((nlay, ng)), np.zeros((nlay, ng))
    cond, cancel = np.ones((nlay, ng)), np.zeros((nlay, ng))
    for ig in range(ng):
        idx = np.flatnonzero(g == ig)
        if idx.size == 0:
            continue                                   # "no wavenumbers with this g point": zeros
        for l in range(nlay):
            od_l = od[l, idx]
            o = od_l.astype(X)
            w = weight[l, idx] if weight.ndim == 2 else weight[idx]
            den = xsum(w)
            lm = methods[l]
            if lm == "linear":
                f = xsum(o * w) / den
            elif lm in TRANSMISSION_K:
                c = X(np.float64(LW_DIFFUSIVITY) * TRANSMISSION_K[lm])       # the formula's constant, a double
                v = xsum(-np.expm1(-o * c) * w) / den
                vc = min(v, X(CLAMP))
                f = abs(-np.log1p(-vc) / c)
                if v > 0:
                    cond[l, ig] = max(1.0, float(vc / ((1 - vc) * abs(np.log1p(-vc)))))
                    cancel[l, ig] = float(1 / v)
            elif lm == "square-root":
                v = xsum(np.sqrt(o) * w) / den
                f = v * v
                cond[l, ig] = 2.0
            else:
                assert lm == "logarithmic"
                nz = od_l > 0
                cnt = int(np.count_nonzero(nz))
                if cnt == 0:
                    f = X(0.0)
                else:
                    logo = np.log(o[nz])
                    den_nz = den if cnt == idx.size else xsum(w[nz])
                    f = np.exp(xsum(logo * w[nz]) / den_nz)
                    if cnt != idx.size:
                        f = f * (X(cnt) / X(idx.size))
                    cond[l, ig] = max(1.0, float(xsum(np.abs(logo) * w[nz]) / den_nz))
            lo, hi = float(od_l.min()), float(od_l.max())
            f = max(X(lo), min(f, X(hi)))
            if lo > f:
                lo = float(f)
            if lo > 0.0 and lo >= hi:                  # one double product each, as in the reference code
                lo, hi = lo * 0.99, hi * 1.01
            fit[l, ig], mn[l, ig], mx[l, ig] = f, lo, hi
    return AvgRef(fit, mn, mx, cond, cancel)


def fit_bound(ref):
    """The relative bound on a device (or oracle) fit: 64 eps max(1, condition); for the transmission methods plus
    eps condition / v for the cancellation in 1 - exp(-x) (see average_reference)."""
    return EPS * (64.0 * np.maximum(1.0, ref.cond) + ref.cond * ref.cancel)


def molar_scale(p_hl, vmr):
    """what a plain optical depth is multiplied by where reference_surface_vmr > 0: (g 0.001 M / vmr) / dp, dp as the double
    difference of the half levels"""
    dp = np.diff(np.asarray(p_hl, dtype=np.float64)).astype(X)
    return (X(ACCEL_GRAVITY) * X(0.001) * X(MOLAR_MASS_DRY_AIR) / X(vmr)) / dp


def relative_error(got, ref):
    """|got - ref| / |ref| per cell in extended precision; 0 where both are 0, inf where only the reference is"""
    got, ref = np.asarray(got).astype(X), np.asarray(ref).astype(X)
    d = np.abs(got - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = d / np.abs(ref)
    return np.where(d == 0, 0.0, r).astype(np.float64)


def assert_branches(method, p, od, g, fit, mn, mx):
    """what the designed g points must give, whoever computed (fit, mn, mx) as plain optical depth"""
    nlay = od.shape[0]
    lm = layer_methods(method, p)
    assert not fit[:, G_ALL_ZERO].any() and not mn[:, G_ALL_ZERO].any() and not mx[:, G_ALL_ZERO].any()
    assert not fit[:, [0, 7]].any() and not mn[:, [0, 7]].any() and not mx[:, [0, 7]].any()       # the empty g points
    for ig in (G_CONSTANT, G_SINGLE):
        v = od[:, np.flatnonzero(g == ig)[0]].astype(np.float64)
        assert np.array_equal(mn[:, ig], v * 0.99) and np.array_equal(mx[:, ig], v * 1.01) and np.array_equal(fit[:, ig], v)
    sat = od[:, g == G_SATURATED].astype(np.float64)
    for l in range(nlay):
        if lm[l] in TRANSMISSION_K:
            # the clamp gives 36.7 / (1.66 k) at most 22.2, below every optical depth of the g point: the fit is its minimum
            assert -math.log1p(-CLAMP) / LW_DIFFUSIVITY < 22.2
            assert fit[l, G_SATURATED] == mn[l, G_SATURATED] == sat[l].min()
        else:
            assert mn[l, G_SATURATED] < fit[l, G_SATURATED] < mx[l, G_SATURATED]
        if lm[l] == "logarithmic":
            # exp(num / den_nz) lies inside the range of the non-zero values; times cnt / ntot < 0.75 it is not clamped
            part = od[l, g == G_PARTLY_ZERO].astype(np.float64)
            frac = np.count_nonzero(part) / part.size
            assert 0.6 < frac < 0.75 and mn[l, G_PARTLY_ZERO] == 0.0
            assert frac * part[part > 0].min() <= fit[l, G_PARTLY_ZERO] <= frac * part.max()
    assert np.array_equal(mx[:, G_SATURATED], sat.max(1))


# --------------------------------------------------------------------------------------------------------- width intervals
# points of one g point inside the designed intervals: nothing; one lane; 63, 64, 65 around one trip of the stride-64 tail;
# 255, 256 (one whole trip of the four-load loop and an empty tail), 257; 511, 512, 513 around its second trip; 1100
RUNS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1100)
LEAD = 100


def width_intervals(g, wn, ig):
    """(wavenumber1, wavenumber2, points of g point ig inside every interval).  The intervals (w1, w2] cut the segment of
    g point ig into its first LEAD points, runs of RUNS points, and the rest; a last interval holds everything.  Every
    bound between two runs IS a wavenumber of the g point: the point on w2 belongs to the interval, the point on w1 does not."""
    s = wn[g == ig]
    assert s.size > LEAD + sum(RUNS)
    bounds, at = [s[LEAD - 1]], LEAD
    for n in RUNS:
        at += n
        bounds.append(s[at - 1])
    below, top = wn[0] - 1.0, wn[-1]
    w1 = np.array([below] + bounds + [below])
    w2 = np.array(bounds + [top, top])
    return w1, w2, [LEAD] + list(RUNS) + [s.size - at, s.size]


# ------------------------------------------------------------------------------------------------- the map's work buffer
def _up(n):
    return -(-n // 256) * 256


def work_bytes(call, nchunk, ng, n):
    """bytes of the map's work buffer that a call asks gmap_work() for (carve_work of create_lut.hip over the pieces that
    gmap_layout.hpp lists per call)"""
    nchunk = max(nchunk, 1)
    if call == "average":
        return _up(nchunk * n * 6 * 8) + _up(3 * n * ng * 8) + _up(n * (2 * 8 + 4))
    if call == "planck_lut":
        return _up(nchunk * n * 8) + _up(n * ng * 8) + _up(n * 8)
    assert call == "gpoint_fraction"
    return _up(ng * (n + 1) * 8) + 2 * _up(n * 8) + _up(nchunk * 8)


# gpoint_fraction (15 intervals), then: the calls of the regrowth test on EDGE, in order
REGROWTH_CALLS = [("gpoint_fraction", 15), ("planck_lut", 1), ("average", 3), ("average", 54), ("planck_lut", 231), ("average", 3)]
