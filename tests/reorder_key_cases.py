"""Inputs and references for the kernels that produce the sort's input: the sorting keys of csrc/reorder.hip (generic longwave,
the 54-layer fast path, shortwave) and the merge kernels of csrc/merge.hip (test_reorder_key_cases.py on the CPU,
test_reorder_key_edges_gpu.py on the device).  numpy only, nothing here imports the library.

The longwave reference, lw_key_longdouble, is written from reorder_spectrum.cpp:111-190 in np.longdouble with expm1, so it is
the value of the formulas and not a copy of their double rounding.  It is of use only where the formulas are well conditioned:
`factor = 1 - eps / (D tau)` amplifies the rounding of `eps = 1 - exp(-D tau)` by 1 / eps, so on layers with tau ~ 1e-6 the
double oracle itself is 1e-6 away from it.  designed_od therefore draws every layer optical depth from {0} U [1e-3, 60]: there
the oracle stays within ORACLE_DIST (test_reorder_key_cases.py) of the long-double value and the device can be held to
TOL = 20 ORACLE_DIST, three orders below the bound that random spectra allow.

The shortwave key has closed forms on hand-built columns (THRESHOLD_COLUMNS): the threshold height is one interpolation between
two half-level pseudo heights, and where one of its two terms is zero the quotient is exact."""
import functools
import math
from collections import namedtuple

import numpy as np

L = np.longdouble

# rt_device.hpp / planck_function.cpp:29-31
PLANCK_H = 6.62606896e-34
BOLTZMANN_K = 1.3806504e-23
LIGHT_C = 2.99792458e8
LW_DIFFUSIVITY = 1.66
ACCEL_GRAVITY = 9.80665
SPECIFIC_HEAT_AIR = 1004.0

KEY_FLOOR = 1e-3          # the metric of the key: |delta| / max(|ref|, KEY_FLOOR)
KEY_RTOL = 1e-9           # the bound of test_reorder_gpu.py on random spectra: the ceiling of every bound here
ORACLE_DIST = 3.0e-14     # largest distance oracle <-> lw_key_longdouble over GEOMETRY x thr (measured 2.927e-14)
TOL = 20 * ORACLE_DIST

LAYER_COUNTS = (1, 2, 53, 54, 55, 80, 81, 160, 161, 320)
BLOCK_EDGE_LAYERS = (54, 81, 161)
THRESHOLDS = (0.0, 0.5)


def key_distance(key, ref):
    """Largest |key - ref| / max(|ref|, 1e-3) over the points where ref is a number (0.0 where there is none)."""
    ref = np.asarray(ref)
    m = ~np.isnan(np.asarray(ref, dtype=np.float64))
    if not m.any():
        return 0.0
    d = np.abs(np.asarray(key, dtype=L)[m] - np.asarray(ref, dtype=L)[m])
    return float(np.max(d / np.maximum(np.abs(np.asarray(ref, dtype=L)[m]), L(KEY_FLOOR))))


def block_threads(nlay):
    """Threads per block of the generic longwave kernel: the largest of 256, 128, 64 whose nlay x threads doubles fit 160 KiB."""
    if nlay <= 80:
        return 256
    if nlay <= 160:
        return 128
    if nlay <= 320:
        return 64
    raise ValueError("more than 320 layers do not fit")


def pressure_grid(nlay):
    """synthetic.pressure_grid, restated so that this module imports nothing of the package."""
    p = np.empty(nlay + 1)
    p[0] = 0.01
    p[1:] = np.exp(np.linspace(np.log(1.0), np.log(101325.0), nlay))
    return p


def wavenumber_grid(nwav, lo=0.0, hi=3260.0):
    dw = (hi - lo) / nwav
    return lo + (np.arange(nwav, dtype=np.float64) + 0.5) * dw, np.full(nwav, dw)


def idealised_temperature(p):
    """reorder_spectrum.cpp:121-124: linear in ln p through (1 Pa, 173.15 K) and (1e5 Pa, 288.15 K).  Only an input here (the
    tests pass the library's own profile to library, oracle and reference alike)."""
    w = (np.log(np.asarray(p, dtype=np.float64)) - math.log(1.0)) / (math.log(100000.0) - math.log(1.0))
    return (1.0 - w) * (273.15 - 100.0) + w * (273.15 + 15.0)


def lw_key_longdouble(p, t, wn, dwn, od, thr):
    """(key, column optical depth) of reorder_spectrum.cpp:111-190 for the longwave, in np.longdouble.

    planck_function.cpp:22-54, radiative_transfer_lw.cpp:27-60 (D = 1.66, the `eps > 1e-5` switch), heating_rate.h:30-50, the
    clamp to cooling (:175), the ratio of the two layer sums (:178-183) and the `thr > 0 && col < thr` override (:187-190).
    The column optical depth is the double sum in layer order, as the reference forms it: the override compares THAT number."""
    p, t, wn, dwn = (np.asarray(a, dtype=L) for a in (p, t, wn, dwn))
    od64 = np.asarray(od, dtype=np.float64)
    tau = od64.astype(L)
    nlay, nwav = tau.shape
    with np.errstate(all="ignore"):
        inv_cm_2_hz = L(100.0) * L(LIGHT_C)
        freq = wn * inv_cm_2_hz
        pref = (dwn * L(2.0) * L(PLANCK_H) * inv_cm_2_hz * L(np.pi) / (L(LIGHT_C) * L(LIGHT_C))) * (freq * freq * freq)
        hk = L(PLANCK_H) / L(BOLTZMANN_K)
        planck = pref[None, :] / np.expm1(hk * freq[None, :] / t[:, None])                     # (nlay + 1, nwav)
        eps = -np.expm1(-L(LW_DIFFUSIVITY) * tau)
        fac = np.where(eps > L(1.0e-5), L(1.0) - eps / (L(LW_DIFFUSIVITY) * np.where(tau > 0, tau, L(1.0))), L(0.5) * eps)
        dn = np.zeros((nlay + 1, nwav), dtype=L)
        for l in range(nlay):
            dn[l + 1] = dn[l] * (L(1.0) - eps[l]) + planck[l] * (eps[l] - fac[l]) + planck[l + 1] * fac[l]
        up = np.empty_like(dn)
        up[nlay] = planck[nlay]                                                                 # emissivity 1
        for l in range(nlay - 1, -1, -1):
            up[l] = up[l + 1] * (L(1.0) - eps[l]) + planck[l + 1] * (eps[l] - fac[l]) + planck[l] * fac[l]
        conv = -(L(ACCEL_GRAVITY) / L(SPECIFIC_HEAT_AIR)) / (p[1:] - p[:-1])
        hr = conv[:, None] * (dn[1:] - dn[:-1] - up[1:] + up[:-1])
        hr = np.where(hr > 0, L(0.0), hr)
        logp = np.log(p)
        d_height = logp[1:] - logp[:-1]
        pseudo_height = logp[nlay] - L(0.5) * (logp[:-1] + logp[1:])
        key = np.sum(hr * (d_height * pseudo_height)[:, None], axis=0) / np.sum(hr * d_height[:, None], axis=0)
    col = np.zeros(nwav)
    for l in range(nlay):
        col = col + od64[l]
    if thr > 0.0:
        key = np.where(col < thr, col.astype(L) - L(thr), key)
    return key, col


def designed_od(nlay, nwav, dtype, seed):
    """(nlay, nwav) layer optical depths 10 ** U(-3, log10 60), about 30 % of the entries exactly 0, the first five columns
    all zero (0 / 0 with thr = 0, the key -thr with thr > 0) - but never the last column, so that one column is left where
    nwav is 1 -, cast to dtype."""
    rs = np.random.RandomState(seed)
    od = 10.0 ** rs.uniform(-3.0, np.log10(60.0), (nlay, nwav))
    od[rs.uniform(size=(nlay, nwav)) < 0.3] = 0.0
    od[:, :min(5, nwav - 1)] = 0.0
    return od.astype(dtype)


def sequential_column(od):
    """The column optical depth as every kernel forms it: double additions in layer order."""
    od = np.asarray(od)
    col = np.zeros(od.shape[1])
    with np.errstate(over="ignore"):
        for l in range(od.shape[0]):
            col = col + od[l].astype(np.float64)
    return col


# ------------------------------------------------------------------------------------------------ 3a: layer count and block edges

GeometryCase = namedtuple("GeometryCase", "nlay nwav dtype strided")


def _geometry():
    cases = []
    for nlay in LAYER_COUNTS:
        b = block_threads(nlay)
        widths = [2 * b + 1]
        if nlay in BLOCK_EDGE_LAYERS:
            widths = [1, b - 1, b, b + 1] + widths
        for nwav in widths:
            for dtype in ("float32", "float64"):
                cases.append(GeometryCase(nlay, nwav, dtype, False))
    # rows of nwav + 3 elements: odd, so that every second row starts off an 8-byte (f32) / 16-byte (f64) boundary
    # (nwav = 2 B + 2 here: nwav + 3 is odd, and the third block holds two threads)
    cases.append(GeometryCase(54, 2 * block_threads(54) + 2, "float32", True))
    cases.append(GeometryCase(54, 2 * block_threads(54) + 2, "float64", True))
    cases.append(GeometryCase(81, 2 * block_threads(81) + 2, "float32", True))
    return cases


GEOMETRY = _geometry()
STRIDE_PAD = 3


def geometry_id(c):
    return "nlay%d-nwav%d-%s%s" % (c.nlay, c.nwav, c.dtype, "-strided" if c.strided else "")


@functools.lru_cache(maxsize=None)
def geometry_inputs(case):
    """(p, t, wn, dwn, od) of a GEOMETRY case; computed once and shared, never written to."""
    p = pressure_grid(case.nlay)
    wn, dwn = wavenumber_grid(case.nwav)
    od = designed_od(case.nlay, case.nwav, case.dtype, 1000 * case.nlay + case.nwav)
    out = (p, idealised_temperature(p), wn, dwn, od)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def geometry_reference(case, thr):
    """(key, col) of lw_key_longdouble for a GEOMETRY case; the key stays np.longdouble."""
    p, t, wn, dwn, od = geometry_inputs(case)
    key, col = lw_key_longdouble(p, t, wn, dwn, od, thr)
    key.setflags(write=False)
    col.setflags(write=False)
    return key, col


# ---------------------------------------------------------------------------------------------------------- 3b: threshold edges

THRESHOLD_PRESSURE = np.array([1.0, 10.0, 100.0, 1000.0, 1.0e5])
THRESHOLD_NWAV = 513
THRESHOLD_INDICES = (0, 255, 256, 512)        # first / last thread of the first block, first of the second, the lone third


def pseudo_height_hl(p):
    """ph[i] = ln(p_s / p[i]) formed as the library and the oracle form it: the difference of two libm logarithms (math.log,
    not numpy's vectorised one, so that the expected heights below carry the very bits)."""
    return np.array([math.log(p[-1]) - math.log(x) for x in p])


# name, layer optical depths (top first), expected shortwave key as f(ph, thr) for thr = 0.5 and thr = 0, and whether that
# expectation is exact (one of the two interpolation terms is zero, or the `col <= thr` branch: one subtraction)
ThresholdColumn = namedtuple("ThresholdColumn", "name od key_half exact_half key_zero exact_zero")

_TINY = 0.25 - 2.0 ** -54      # .25 + _TINY = .5 - 2^-54, the double just below .5

THRESHOLD_COLUMNS = (
    ThresholdColumn("col == thr", (0.25, 0.25, 0.0, 0.0),
                    lambda ph: 0.0, True,                                               # col <= thr: col - thr
                    lambda ph: (0.25 * ph[0]) / 0.25, True),                            # crosses in layer 0 with cum = 0
    ThresholdColumn("crossing on level 1", (0.5, 1.0, 0.0, 0.0),
                    lambda ph: (0.5 * ph[1]) / 0.5, True,                               # next_col == thr: weight 0 on ph[0]
                    lambda ph: (0.5 * ph[0]) / 0.5, True),
    ThresholdColumn("two zero layers, then the crossing", (0.0, 0.0, 1.0, 0.0),
                    lambda ph: (0.5 * ph[3] + 0.5 * ph[2]) / 1.0, False,
                    lambda ph: 0.0, True),                                              # 0 >= 0 in the zero top layer: 0 / 1e-12
    ThresholdColumn("zero top layer", (0.0, 0.75, 0.0, 0.0),
                    lambda ph: (0.5 * ph[2] + 0.25 * ph[1]) / 0.75, False,
                    lambda ph: 0.0, True),
    ThresholdColumn("fmax(1e-12, tau) divisor", (1.0e-13, 0.0, 0.0, 0.0),
                    lambda ph: 1.0e-13 - 0.5, True,
                    lambda ph: (1.0e-13 * ph[0]) / 1.0e-12, True),                      # the divisor is 1e-12, not tau
    ThresholdColumn("zero column", (0.0, 0.0, 0.0, 0.0),
                    lambda ph: -0.5, True,
                    lambda ph: 0.0, True),                                              # col <= thr with both 0
    ThresholdColumn("all of it in the last layer", (0.0, 0.0, 0.0, 0.5),
                    lambda ph: 0.0, True,                                               # col == thr again, reached at the surface
                    lambda ph: 0.0, True),
    ThresholdColumn("one ulp below thr", (0.25, _TINY, 0.0, 0.0),
                    lambda ph: -2.0 ** -54, True,
                    lambda ph: (0.25 * ph[0]) / 0.25, True),
)
THIN_COLUMN = 4                # the 1e-13 column: its longwave key lies in the thin regime and is not compared


def threshold_pattern(shift, nwav=THRESHOLD_NWAV):
    """Index of the THRESHOLD_COLUMNS entry at every wavenumber: (j + shift) % 8.  Over shift = 0 .. 7 every column stands
    once at each of THRESHOLD_INDICES."""
    return (np.arange(nwav) + shift) % len(THRESHOLD_COLUMNS)


def threshold_od(shift, nlay=4, dtype="float64", nwav=THRESHOLD_NWAV):
    """(nlay, nwav): the hand-built columns in the top four layers, zero below."""
    pat = threshold_pattern(shift, nwav)
    od = np.zeros((nlay, nwav))
    od[:4] = np.array([c.od for c in THRESHOLD_COLUMNS]).T[:, pat]
    return od.astype(dtype)


def threshold_expected_sw(shift, ph, thr, nwav=THRESHOLD_NWAV):
    """(key, exact mask) of the shortwave key on threshold_od(shift) for pseudo heights ph of the top four layers' levels."""
    pat = threshold_pattern(shift, nwav)
    if thr == 0.5:
        vals = np.array([c.key_half(ph) for c in THRESHOLD_COLUMNS])
        exact = np.array([c.exact_half for c in THRESHOLD_COLUMNS])
    elif thr == 0.0:
        vals = np.array([c.key_zero(ph) for c in THRESHOLD_COLUMNS])
        exact = np.array([c.exact_zero for c in THRESHOLD_COLUMNS])
    else:
        raise ValueError("closed forms are written for thr 0.5 and 0")
    return vals[pat], exact[pat]


# ------------------------------------------------------------------------------------------------------------- 3c: the error flag

FLAG_THR = 0.25
FLAG_HARMLESS = 300
FLAG_INDEX = 299               # the offending column: in the second, last block of 256


def flag_pressure(nlay, top, second=None):
    """Half-level pressures with the top level at pseudo height `top`, optionally a second one at `second`, and the rest
    log-spaced from pseudo height 29.4 down to the surface at 1e5 Pa.  A column with tau 1 in the top layer and thr .25
    crosses in layer 0 at .25 x 29.4 + .75 x top: 30.225 for top = 30.5, 29.475 for top = 29.5."""
    ps = 1.0e5
    tops = [top] if second is None else [top, second]
    return np.concatenate((ps * np.exp(-np.array(tops)), ps * np.exp(np.linspace(-29.4, 0.0, nlay + 1 - len(tops)))))


def flag_od(nlay, kind="offending"):
    """FLAG_HARMLESS harmless columns - nothing in the top layer, so they cross below pseudo height 29.4, or stay under the
    threshold, or are zero - and, for kind "offending", the column (1, 0, ...) put in at FLAG_INDEX.

    The "latch" kinds go with flag_pressure(nlay, 30.5, 30.2), two levels above 30.  "latch_harmless": nothing in the top TWO
    layers; with thr = 0 every column crosses in the empty top layer (0 >= 0) at height 0 / 1e-12 = 0 - a latch that waits
    for `next_col > thr` finds level 1 or 2 instead.  "latch_offending" adds the column (.25, 0, 1, 0, ...) at FLAG_INDEX:
    with thr = .25 it crosses ON level 1, height ph[1] = 30.2, a refusal; a latch with `>` finds ph[2] = 29.4."""
    od = designed_od(nlay, FLAG_HARMLESS, "float64", 77 + nlay)
    od[0] = 0.0
    od[:, 7] = 0.0
    od[-1, 7] = 0.125                                         # under the threshold
    if kind.startswith("latch"):
        od[1] = 0.0
    bad = np.zeros((nlay, 1))
    if kind == "offending":
        bad[0, 0] = 1.0
    elif kind == "latch_offending":
        bad[0, 0], bad[2, 0] = 0.25, 1.0
    elif kind not in ("harmless", "latch_harmless"):
        raise ValueError(kind)
    if bad.any():
        od = np.concatenate((od[:, :FLAG_INDEX], bad, od[:, FLAG_INDEX:]), axis=1)
    return np.ascontiguousarray(od)


# --------------------------------------------------------------------------------------------------- 3d: shortwave key geometry

SW_THR = 0.25
SwCase = namedtuple("SwCase", "nlay nwav dtype strided")
SW_GEOMETRY = [SwCase(nlay, nwav, dtype, False) for nlay in (1, 54) for nwav in (1, 255, 256, 257)
               for dtype in ("float32", "float64")] + [SwCase(54, 257, "float32", True)]


def sw_od(case):
    """Optical depths over thirteen decades, a fifth of them zero, with a float32 subnormal and 1e30 among them (alone in the
    single column of nwav = 1: the subnormal at the top where there are layers to follow it)."""
    rs = np.random.RandomState(31 * case.nlay + case.nwav)
    od = 10.0 ** rs.uniform(-9.0, 4.0, (case.nlay, case.nwav))
    od[rs.uniform(size=od.shape) < 0.2] = 0.0
    od[0, 0] = 1.0e-40                                        # subnormal as float32
    od[case.nlay // 2, -1] = 1.0e30
    if case.nwav > 2:
        od[:, 1] = 1.0e-40                                    # a column that never leaves the subnormals
    return od.astype(case.dtype)


# --------------------------------------------------------------------------------------------------------------------- 3e: merge

def derive_d_wavenumber(wn):
    """read_spectrum.cpp:55-65."""
    d = np.empty_like(wn)
    d[1:-1] = 0.5 * (wn[2:] - wn[:-2])
    d[0] = 0.5 * d[1]
    d[-1] = 0.5 * d[-2]
    return d


MERGE_SHAPES = [(nlay, nwav) for nlay in (1, 12) for nwav in (1, 256, 257)]
MERGE_SENTINEL = -7.0


def merge_gases(nlay, nwav):
    """[(od float32, scale), (od float64, scale)]: the second gas has an infinite optical depth in a layer whose scale is 0."""
    rs = np.random.RandomState(5 * nlay + nwav)
    od1 = rs.lognormal(-3.0, 3.0, (nlay, nwav)).astype(np.float32)
    od2 = rs.lognormal(-3.0, 3.0, (nlay, nwav))
    s1 = rs.uniform(0.5, 2.0, nlay)
    s2 = rs.uniform(0.5, 2.0, nlay)
    s2[nlay - 1] = 0.0
    od2[nlay - 1, nwav // 2] = np.inf
    od1[0, 0] = np.float32(np.inf)                            # inf x (scale > 0) = inf, and inf + finite stays inf
    return [(od1, s1), (od2, s2)]


def merge_expected(gases):
    """read_merged_spectrum.cpp:152-166: product and sum rounded separately, gases in order; the first is stored, not added."""
    want = None
    with np.errstate(invalid="ignore"):
        for od, s in gases:
            term = od.astype(np.float64) * s[:, None]
            want = term if want is None else want + term
    return want
