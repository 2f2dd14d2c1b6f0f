"""Interval sums, fits and errors at every tile, super-tile and chunk edge (K5a-K5d of csrc/find_g.hip).

An interval's error is built from `interval_row_acc` (ragged head, 256-point tiles, 65 536-point super tiles, the tiles behind
them, ragged tail), from the tile sums of one of two producers (`k_tile_sums`, or the per-wave sums of the 54-layer FLOAT
preparation through `k_combine_wave_sums`) and from the RT chunks of `interval_chunk_pts`; the interval table reaches the
kernels in their arguments (up to 64 intervals) or through a copied table.  The intervals here are given by their first and
last sorted index - band = interval, bounds 0 and 1 - and placed on every one of those edges on purpose.

References: the fits of the linear / transmission / transmission-2 / square-root methods against the gas's OWN resident rows,
summed exactly and put through find_g_points.cpp:54-106 in mpmath (bound derived below, `_fit_reference`); the logarithmic
fit, every error and the shortwave fits against the CPU oracle over the same slice, with the tolerances of test_find_g_gpu.py
and test_find_g_sw_gpu.py."""
import ctypes as C
import functools
import math
import time
from concurrent.futures import ThreadPoolExecutor

import mpmath
import numpy as np
import pytest
import torch

import test_find_g_sw_gpu as sw
from test_find_g_gpu import ERR_RTOL, _dev, _lw_problem, _make_gas, _oracle_eq

pytestmark = pytest.mark.gpu

mp = mpmath.mp
mp.dps = 40

TILE = 256                 # points per tile (TILE of find_g.hip)
S = 65536                  # points per super tile (TILE * SUPER)
N = 3 * S + 777            # two interior super-tile edges, a ragged last tile (9 points), a last wave that is not full
N_LONG = 600_011           # the run-time sweep's chunk grows beyond one granule only past 8 * num_cu * 256 points
I0 = 4321                  # an unaligned start for the chunk-edge lengths
FLUX_WEIGHT = 0.02
# The synthetic target gas has ~5 % columns that are exactly zero; they sort to the front.  Every sorted array is rotated by
# SHIFT (the gas takes the ordering as an input), so that the short intervals at 0, S and 2S hold ordinary columns - an
# off-by-one on a row of zeros would go unnoticed - and the zero columns lie inside the third super tile, in the long ones.
SHIFT = 150_000
LOG_LAYER = 7              # logarithmic case: the layer whose optical depth is set to zero at the sorted points LOG_ZEROS
LOG_ZEROS = (250, 520)


@pytest.fixture(autouse=True)
def _every_request_on_the_device(monkeypatch):
    """As in test_find_g_gpu.py: the memo of interval errors would answer a repeated interval without running it."""
    monkeypatch.setenv("ECCKD_NO_ERROR_MEMO", "1")


@pytest.fixture(scope="module", autouse=True)
def _module_time():
    t0 = time.time()
    yield
    for cached in (_lw_base, _lw_case, _sw_case, _lw_reference_errors):      # a few GB of host arrays: not for the rest of the session
        cached.cache_clear()
    print(f"\ntest_interval_edges_gpu: {time.time() - t0:.1f} s for the module (CPU oracle included)")


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------------------
# The interval list

def interval_list(n, G, L0):
    """[(i1, i2)] inclusive sorted indices, and how many chunk-edge entries did not fit into n.
    G: points of one block iteration of the sweep (128: longwave mirror kernel, 256: every other sweep); L0: the longest
    interval whose chunk is one granule = (chunks per interval) * G, interval_chunk_pts.
    In the comments t1 / t2 are the first whole tile and one past the last, s1 / s2 the same for super tiles."""
    iv = [
        # 1. no whole tile inside (t1 >= t2): the raw loop of interval_row_acc
        (0, 0),                    # the row's first point
        (255, 255),                # last point of tile 0
        (256, 256),                # first point of tile 1
        (n - 1, n - 1),            # last point of the ragged last tile
        (1, 254),                  # inside one tile, one loop turn
        (1, 510),                  # the longest such interval (2 TILE - 2 points): two loop turns for most threads
        (255, 256),                # across a tile edge
        (257, 511),                # ends on a tile's last point, starts behind its first
        # 2. whole tiles, no whole super tile (s1 >= s2): head / tile loop / tail
        (0, 255),                  # exactly one tile: no head, no tail
        (0, 256),                  # one tile and one tail point
        (1, 512),                  # 255 head points, one tile, one tail point
        (255, 767),                # one head point, two tiles, no tail
        (256, S - 1),              # tiles 1..255 and nothing else; ends on the super-tile edge
        (1, 2 * S - 2),            # the longest: 2 * 256 - 2 tiles, two turns of the tile loop per thread, 255 head and tail points
        (S - 256, S + 255),        # two tiles across a super-tile edge
        # 3. whole super tiles (s1 < s2)
        (0, S - 1),                # exactly super tile 0: no head tiles, none behind
        (0, S),                    # ... and one tail point
        (1, 2 * S),                # 255 head points, 255 head tiles, super tile 1, no tile behind, one tail point
        (S - 1, 2 * S - 1),        # one head point, no head tile, super tile 1
        (S, 2 * S - 1),            # exactly super tile 1
        (S, 2 * S),                # ... and one tail point
        (S - 257, 2 * S + 256),    # one head point, ONE head tile, super tile 1, ONE tile behind, one tail point
        (0, 3 * S - 1),            # three super tiles in the super-tile loop
        (0, n - 1),                # every super tile, the tiles behind the last one, the ragged last tile as the tail
        (S + 1, n - 1),            # 255 head points, 255 head tiles, super tiles from 2, tiles behind, ragged tail
    ]
    # 4. chunk edges at an unaligned start: chunk = one granule up to L0 points, two from L0 + 1
    lengths = [G - 1,              # less than one block iteration: dead lanes in the only tile
               G,                  # exactly one
               G + 1,              # two chunks, the second of one point
               2 * G,
               L0 - 1,             # the last chunk one point short
               L0,                 # (chunks per interval) full chunks of one granule
               L0 + 1,             # chunk becomes 2 G
               L0 + G + 1]         # 2 G chunks with a ragged last one of G + 1 points
    fits = [(I0, I0 + m - 1) for m in lengths if I0 + m - 1 <= n - 1]      # where num_cu * G makes L0 exceed n they are dropped
    if _long(iv + fits) > 8:
        # at most eight intervals of more than 100 000 points per case (the CPU oracle's time): where the lengths around L0
        # are that long themselves, [0, 3S-1] goes - [0, n-1] holds as many super tiles in the loop, [0, S-1] and [S, 2S-1]
        # end on a super-tile edge with no tile behind
        iv.remove((0, 3 * S - 1))
    return iv + fits, len(lengths) - len(fits)


def _long(iv):
    return sum(1 for a, b in iv if b - a + 1 > 100_000)


# ---------------------------------------------------------------------------------------------------------------------------
# Exact sums of the gas's own rows

def _dd_reduce(h):
    """Sum along the last axis as (hi, lo) pairs: a pairwise tree of error-free additions (Knuth's TwoSum, exact for any two
    doubles) whose rounding errors are carried in lo.  hi + lo is the exact sum up to the roundings of the lo additions:
    ~ levels * n * 2^-106 relative for non-negative terms, 1e-24 at 600 000 points."""
    l = np.zeros_like(h)
    while h.shape[-1] > 1:
        if h.shape[-1] & 1:
            pad = np.zeros(h.shape[:-1] + (1,))
            h, l = np.concatenate([h, pad], axis=-1), np.concatenate([l, pad], axis=-1)
        a, b = h[..., 0::2], h[..., 1::2]
        s = a + b
        bb = s - a
        e = (a - (s - bb)) + (b - bb)
        l = (l[..., 0::2] + l[..., 1::2]) + e
        h = s
    return h[..., 0], l[..., 0]


class _RowSums:
    """Interval sums of every row of a (rows, n) array to ~30 digits: exact (hi, lo) sums of blocks of 1024 points once,
    then per interval the raw points of the two ragged ends and the blocks between them."""
    BLOCK = 1024

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows)
        r, n = self.rows.shape
        nb = -(-n // self.BLOCK)
        padded = np.zeros((r, nb * self.BLOCK))
        padded[:, :n] = self.rows
        self.hi, self.lo = _dd_reduce(padded.reshape(r, nb, self.BLOCK))

    def __call__(self, i1, i2):
        B = self.BLOCK
        b1, b2 = -(-i1 // B), (i2 + 1) // B
        if b1 >= b2:
            terms = self.rows[:, i1:i2 + 1]
        else:
            terms = np.concatenate([self.rows[:, i1:b1 * B], self.hi[:, b1:b2], self.lo[:, b1:b2],
                                    self.rows[:, b2 * B:i2 + 1]], axis=1)
        hi, lo = _dd_reduce(terms)
        return [mp.mpf(float(x)) + mp.mpf(float(y)) for x, y in zip(hi, lo)]


# ---------------------------------------------------------------------------------------------------------------------------
# The fit from exact sums, and how far the device may be from it

EPS = 2.0 ** -53                         # unit roundoff of a double
ULP = 2.0 ** -52
# The device adds the non-negative terms of a sum through at most ~40 roundings (thread accumulation, the 256-thread tree, and
# below it the trees of the tile and super-tile sums), so each sum is within 64 * 2^-53 relative of the exact one.
SUM_RTOL = 64 * EPS
CLAMP = 0.9999999999999999
KD = 1.66                                # LW_DIFFUSIVITY


def _fit_reference(method, a, b):
    """fit_optical_depth_lw (find_g_points.cpp:54-106) of one layer from the exact sums a (weighted metric) and b (weights),
    and the bound on the device's relative distance from it - derived, not measured (None: no bound, see below).

    x = a / b: both sums within SUM_RTOL and one correctly rounded division, dx = 2 SUM_RTOL + EPS (+ second order).
      linear        x                               dx
      square-root   x^2                             2 dx + EPS (the product)
      transmission  |-log(1 - min(CLAMP, x)) / kD|  w = 1 - x is formed in double precision: x' = x (1 + d), |d| <= dx, moves
                    it by t = x dx / (1 - x) relative, its own rounding by EPS; log w moves by -log(1 - t) + EPS, the fit by
                    that over |log(1 - x)| (for small t the condition number x / ((1 - x) |log(1 - x)|) times dx, plus
                    EPS / |log(1 - x)|: a double next to 1 cannot hold an x below 1e-16 any better); + 4 ulp for the device's
                    log and the division by kD.  x above the clamp: the clamped value itself, no term for the sums; the 4 ulp
                    stay, because the reference's log is mpmath's and the device's is not correctly rounded.  Within 2 x dx
                    of 1 the clamp may or may not have acted on the device: no bound, the fit lies between the reference and
                    the clamped one (the test allows two such fits per case; the synthetic gases have none)."""
    x = a / b
    dx = 2 * SUM_RTOL + EPS + 4 * SUM_RTOL * SUM_RTOL
    if method == "linear":
        return x, dx
    if method == "square-root":
        return x * x, 2 * dx + EPS + dx * dx
    scale = KD * (2.0 if method == "transmission-2" else 1.0)
    clamped = -mp.log(mp.mpf(1.0 - CLAMP)) / scale
    if x > CLAMP:
        return clamped, 4 * ULP
    if x == 0:
        return mp.mpf(0), 0.0
    w = 1 - x
    t = x * dx / w
    if t >= 0.5:
        return -mp.log(w) / scale, None
    dlog = -mp.log(1 - t) + EPS
    return -mp.log(w) / scale, float(dlog / abs(mp.log(w))) + 4 * ULP


def _fit_multiples(method, fit, a_sums, b_sums):
    """|device - reference| / (bound * reference) per layer (0 where they agree exactly, inf where a zero bound is missed)."""
    out = []
    for l, (a, b) in enumerate(zip(a_sums, b_sums)):
        ref, bound = _fit_reference(method, a, b)
        dev = mp.mpf(float(fit[l]))
        assert math.isfinite(fit[l]) and fit[l] >= 0.0
        if bound is None:
            clamped = -mp.log(mp.mpf(1.0 - CLAMP)) / (KD * (2.0 if method == "transmission-2" else 1.0))
            out.append(0.0 if ref * (1 - 1e-9) <= dev <= clamped * (1 + 4 * ULP) else math.inf)
        elif dev == ref:
            out.append(0.0)
        elif bound == 0.0 or ref == 0:
            out.append(math.inf)
        else:
            out.append(float(abs(dev - ref) / (bound * abs(ref))))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The cases: one target gas and a background each, built once

_SORTED_LW = ("planck", "surf_planck", "bg_s", "metric", "hr", "fds", "fut", "wn_s")
_SORTED_SW = ("od_s", "bg_s", "ssi_s", "hr", "fds", "fut", "metric")
_EXTRAS_SW = ("flux_up_toa_low", "flux_up_toa_high", "hr_low", "hr_high", "flux_dn_surf_low", "flux_dn_surf_high")
LW_CASES = {54: dict(n=N, G=128, bpc=3, od_dtype=np.float32),        # k_gas_prep_lw_mirror + K4's wave sums, the <54> mirror sweep
            30: dict(n=N, G=128, bpc=3, od_dtype=np.float64),        # general preparation + k_tile_sums, the <30> mirror sweep
            12: dict(n=N_LONG, G=256, bpc=8, od_dtype=np.float64)}   # general preparation, run-time sweep
SW_CASES = {54: dict(n=N, G=256, bpc=2, method="total-transmission", od_dtype=np.float32),   # the two-fit fast sweep
            12: dict(n=N, G=256, bpc=8, method="transmission", od_dtype=np.float64)}        # run-time sweep


def _rotate(o, keys, n):
    """The same problem with the sorted order rotated by SHIFT: columns are independent, so every sorted array just rolls."""
    r = dict(o)
    r["rank"] = (o["rank"].astype(np.int64) + SHIFT) % n
    for k in keys:
        r[k] = np.roll(o[k], SHIFT, axis=-1)
    return r


@functools.lru_cache(maxsize=None)
def _lw_base(oracle, nlay):
    n = LW_CASES[nlay]["n"]
    o = _rotate(_lw_problem(oracle, n, nlay=nlay, seed=71 + nlay, method="transmission"), _SORTED_LW, n)
    o["od_s"] = o["od"][:, np.argsort(o["rank"])]
    return o


@functools.lru_cache(maxsize=None)
def _lw_case(oracle, nlay, method):
    """Host arrays and oracle inputs of the longwave case (sorted order), by averaging method."""
    o = _lw_base(oracle, nlay)
    if method == "transmission":
        return o
    o, n = dict(o), LW_CASES[nlay]["n"]
    if method == "logarithmic":
        # one layer without absorption at the sorted points LOG_ZEROS: intervals inside have no positive metric there
        # (nnz == 0 -> 0, find_g_points.cpp:92), intervals across its ends some (nnz < ntot, :94-98)
        ireorder = np.argsort(o["rank"])
        od = o["od"].copy()
        od[LOG_LAYER, ireorder[LOG_ZEROS[0]:LOG_ZEROS[1] + 1]] = 0.0
        o["od"], o["od_s"] = od, od[:, ireorder]
        fdn, fup = oracle.radiative_transfer_lw(o["planck"], o["bg_s"] + o["od_s"], np.ones(n), o["surf_planck"])
        o.update(hr=oracle.heating_rate(o["p"], fdn, fup), fds=fdn[-1].copy(), fut=fup[0].copy())
    o["metric"] = oracle.metric(method, o["od_s"])
    return o


@functools.lru_cache(maxsize=None)
def _sw_case(oracle, nlay):
    c = SW_CASES[nlay]
    o = sw._sw_problem(oracle, c["n"], nlay=nlay, seed=73 + nlay, method=c["method"])
    ex = o["extras"]
    o = _rotate(o, _SORTED_SW, c["n"])
    if ex is not None:
        o["extras"] = dict(ex, **{k: np.roll(ex[k], SHIFT, axis=-1) for k in _EXTRAS_SW})
    return o


def _case_intervals(c):
    iv, dropped = interval_list(c["n"], c["G"], c["bpc"] * _num_cu() * c["G"])
    return iv, dropped


class _Gases:
    """The gases of this module, made when first asked for and closed at its end; with the exact row sums of a longwave one."""

    def __init__(self, ctx, oracle):
        self.ctx, self.oracle, self.made, self.sums = ctx, oracle, {}, {}

    def lw(self, nlay, method):
        key = ("lw", nlay, method)
        if key not in self.made:
            self.made[key] = _make_gas(self.ctx, _lw_case(self.oracle, nlay, method), method, flux_weight=FLUX_WEIGHT,
                                       od_dtype=LW_CASES[nlay]["od_dtype"])
        return self.made[key]

    def lw_sums(self, nlay, method):
        key = (nlay, method)
        if key not in self.sums:
            gas = self.lw(nlay, method)
            self.sums[key] = (_RowSums(gas.view("weighted_metric")), _RowSums(gas.view("planck_hl")[1:]))
        return self.sums[key]

    def sw(self, nlay):
        from ecckd_amd import api
        key = ("sw", nlay)
        if key not in self.made:
            c, o = SW_CASES[nlay], _sw_case(self.oracle, nlay)
            ex = o["extras"] or {}
            od = o["od"].astype(c["od_dtype"])
            assert np.array_equal(od.astype(np.float64), o["od"])
            self.made[key] = api.GasSW(self.ctx, o["p"], _dev(self.ctx, o["ssi"]), _dev(self.ctx, o["rank"].astype(np.int32)),
                                       _dev(self.ctx, od), _dev(self.ctx, o["bg"]), c["method"], FLUX_WEIGHT, 0.0, sw.MU0,
                                       _dev(self.ctx, o["albedo"]), ex.get("min_scaling", 1.0), ex.get("max_scaling", 1.0))
        return self.made[key]

    def close(self):
        for g in self.made.values():
            g.close()


@pytest.fixture(scope="module")
def gases(ctx, oracle):
    g = _Gases(ctx, oracle)
    yield g
    g.close()


def _errors(gas, iv, albedo=None):
    i1 = np.array([a for a, _ in iv])
    npts = np.array([b - a + 1 for a, b in iv])
    return gas.calc_error_multi(i1, npts, np.zeros(len(iv)), np.ones(len(iv)), band_albedo=albedo)


def _in_threads(fn, items):
    """The oracle's C functions release the interpreter lock: the intervals of a case side by side."""
    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(fn, items))


def _oracle_errors(oracle, eq, iv, albedo=None):
    """calc_error(0, 1) of the oracle's CkdEquipartition built over the slice [i1, i2] of eq's arrays, for every interval: the
    slice is the same structure with every spectral array starting at i1 and i2 - i1 + 1 points (the row stride stays), so
    the long intervals are not copied."""
    spectral = ("ssi", "surf_emissivity", "surf_planck", "flux_dn_surf", "flux_up_toa", "planck_hl", "bg_od", "metric", "hr",
                "flux_dn_surf_low", "flux_up_toa_low", "flux_dn_surf_high", "flux_up_toa_high", "hr_low", "hr_high")
    per_layer = ("layer_weight", "pressure_hl")
    assert {name for name, ctype in eq.s._fields_ if ctype is oracle.dp} == set(spectral + per_layer)    # a new array must be placed

    def one(k):
        i1, i2 = iv[k]
        s = type(eq.s).from_buffer_copy(eq.s)
        for name in spectral:
            if getattr(s, name):
                setattr(s, name, C.cast(C.addressof(getattr(s, name).contents) + 8 * i1, oracle.dp))
        s.npoints = i2 - i1 + 1
        if albedo is not None:
            s.surf_albedo = float(albedo[k])
        status = C.c_int(0)
        e = oracle.lib().orc_ckd_calc_error(C.byref(s), C.c_double(0.0), C.c_double(1.0), C.byref(status))
        assert status.value == 0
        return e
    return np.array(_in_threads(one, range(len(iv))))


def _oracle_errors_lw(oracle, o, method, iv):
    return _oracle_errors(oracle, _oracle_eq(oracle, o, method, FLUX_WEIGHT), iv)


@functools.lru_cache(maxsize=None)
def _lw_reference_errors(oracle, nlay, method, num_cu):
    # num_cu is part of the cache key only: the list (_case_intervals reads the device itself) depends on it
    iv, _ = _case_intervals(LW_CASES[nlay])
    return _oracle_errors_lw(oracle, _lw_case(oracle, nlay, method), method, iv)


def _assert_close(what, iv, got, ref, rtol, atol):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, [iv[k] for k in np.nonzero(np.isnan(got) != np.isnan(ref))[0]])
    ok = np.isfinite(ref)
    bad = ok & ~np.isclose(got, np.where(ok, ref, 0.0), rtol=rtol, atol=atol)
    rel = np.abs(got[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), atol / rtol)
    print(f"{what}: {ok.sum()} intervals, largest |difference| / max(|reference|, {atol / rtol:g}) = {rel.max():.2e} (allowed {rtol:g})")
    assert not bad.any(), (what, [(iv[k], got[k], ref[k]) for k in np.nonzero(bad)[0]])


# ---------------------------------------------------------------------------------------------------------------------------
# The tests

def test_interval_list_reaches_every_branch():
    """A self-check of the interval list, not coverage of the kernel (no device code runs; the device is only asked for its
    CU count): that every case's entries reach every branch of interval_row_acc and chunks of one and of two granules, worked
    out with the index rules written down independently of the kernel's.  The counts assume nothing but the list; the number
    of entries that do not fit is stated for the 256 CUs of an MI355X."""
    from collections import Counter
    num_cu = _num_cu()
    for name, c in [(f"lw{k}", v) for k, v in LW_CASES.items()] + [(f"sw{k}", v) for k, v in SW_CASES.items()]:
        blocks = c["bpc"] * num_cu
        iv, dropped = _case_intervals(c)
        seen, chunks = Counter(), Counter()
        for i1, i2 in iv:
            assert 0 <= i1 <= i2 < c["n"]
            first, last = -(-i1 // TILE), (i2 + 1) // TILE - 1          # whole tiles first..last
            if first > last:
                seen["no tile"] += 1
            else:
                seen["head"] += i1 % TILE != 0
                seen["tail"] += (i2 + 1) % TILE != 0
                sfirst, slast = -(-first // 256), (last + 1) // 256 - 1    # whole super tiles sfirst..slast
                if sfirst > slast:
                    seen["tile loop"] += 1
                    seen["tile loop, two turns"] += last - first + 1 > 256
                else:
                    seen["super loop"] += 1
                    seen["head tiles"] += first % 256 != 0
                    seen["tiles behind"] += (last + 1) % 256 != 0
            m = i2 - i1 + 1
            per_block = -(-m // blocks)
            chunk = -(-per_block // c["G"]) * c["G"]                   # the smallest multiple of G with at most `blocks` chunks
            chunks[chunk // c["G"]] += 1
            assert -(-m // chunk) <= blocks
        for branch in ("no tile", "head", "tail", "tile loop", "tile loop, two turns", "super loop", "head tiles", "tiles behind"):
            assert seen[branch] >= 1, (name, branch)
        assert _long(iv) <= 8, name                       # the CPU side stays cheap
        # chunks of two granules (L0 + 1, L0 + G + 1) on a fast longwave case and on the run-time longwave case; on an
        # MI355X (256 CUs) the four entries from L0 - 1 on do not fit into the shortwave run-time case (8 * 256 * 256 > n)
        if name in ("lw54", "lw30", "lw12", "sw54"):
            assert dropped == 0 and chunks[2] >= 2, (name, dropped, chunks)
        if num_cu == 256:
            assert dropped == {"sw12": 4}.get(name, 0), (name, dropped)
        assert chunks[1] >= 24 and len(iv) == 33 - dropped - ((0, 3 * S - 1) not in iv)


def test_exact_row_sums_agree_with_fsum():
    """The reference's own arithmetic: the (hi, lo) block sums against math.fsum, which is exactly rounded."""
    rs = np.random.RandomState(3)
    rows = np.abs(rs.standard_normal((3, 70_001))) * 10.0 ** rs.uniform(-30, 0, (3, 70_001))
    sums = _RowSums(rows)
    for i1, i2 in [(0, 0), (5, 1000), (1023, 1024), (1, 70_000), (1024, 4095), (333, 50_000)]:
        for r, s in enumerate(sums(i1, i2)):
            assert float(s) == math.fsum(rows[r, i1:i2 + 1].tolist())


@pytest.mark.parametrize("nlay,method", [(54, "transmission"), (54, "transmission-2"), (30, "transmission"),
                                         (30, "square-root"), (12, "transmission"), (12, "linear")])
def test_fits_match_exact_sums_of_the_resident_rows(gases, nlay, method):
    """a. ecckd_fit_optical_depth of every listed interval against the gas's own rows summed exactly: what is left is the
    re-association of the sum hierarchy and one log.  That entry point launches the unfused pair k_interval_sums + k_fit_lw
    (always with a copied interval table); the fused k_interval_sums_fit_lw of the error path calls the same
    interval_row_acc and the same fit_lw_layer - the fit arithmetic is one function for both - and is pinned by the error
    tests.  Largest observed multiples of the derived bound on an MI355X:
    0.500 for the transmission methods (thin layers: half an ulp of 1 - a / b; 0.055 where a / b >= 0.1), 0.033 square-root,
    0.057 linear ("Interval edges")."""
    gas = gases.lw(nlay, method)
    a_of, b_of = gases.lw_sums(nlay, method)
    iv, _ = _case_intervals(LW_CASES[nlay])
    worst, where, worst_thick, unbounded = 0.0, None, 0.0, 0
    for i1, i2 in iv:
        fit = gas.fit_optical_depth(i1, i2 - i1 + 1, [0.0], [1.0])[0]
        a, b = a_of(i1, i2), b_of(i1, i2)
        assert all(x > 0 for x in b)
        unbounded += sum(_fit_reference(method, x, y)[1] is None for x, y in zip(a, b))
        mult = _fit_multiples(method, fit, a, b)
        if max(mult) > worst:
            worst, where = max(mult), ((i1, i2), int(np.argmax(mult)))
        # where a / b is not small the bound is that of the sums; in thin layers the rounding of 1 - a / b takes it over
        worst_thick = max([worst_thick] + [m for m, x, y in zip(mult, a, b) if x >= 0.1 * y])
    print(f"fits {nlay} layers {method}: largest multiple of the derived bound {worst:.3f} at (interval, layer) {where}, "
          f"{worst_thick:.3f} where a / b >= 0.1; {unbounded} of {len(iv) * nlay} fits next to the clamp without a bound")
    assert worst <= 1.0, (worst, where)
    assert unbounded <= 2


def test_logarithmic_fit_and_its_zero_count_branches(gases, oracle):
    """a. (logarithmic): the second weight row and the counts of positive metrics are not among the views, so the reference
    is the oracle's fit from its own arrays (rtol 1e-10: independently prepared rows).  One layer has no absorption at the
    sorted points LOG_ZEROS: nnz == 0 -> 0 for the intervals inside, nnz < ntot for those across its ends."""
    nlay = 30
    o = _lw_case(oracle, nlay, "logarithmic")
    gas = gases.lw(nlay, "logarithmic")
    iv, _ = _case_intervals(LW_CASES[nlay])
    n = LW_CASES[nlay]["n"]
    planck, metric = np.ascontiguousarray(o["planck"]), np.ascontiguousarray(o["metric"])
    none, some = [], []
    for i1, i2 in iv:
        fit = gas.fit_optical_depth(i1, i2 - i1 + 1, [0.0], [1.0])[0]
        ref = np.empty(nlay)
        oracle.lib().orc_fit_optical_depth_lw(C.c_int(oracle.AVG["logarithmic"]), C.c_int(nlay), C.c_size_t(n), C.c_size_t(i1),
                                              C.c_size_t(i2), oracle._p(planck), oracle._p(metric), oracle._p(ref))
        assert np.allclose(fit, ref, rtol=1e-10, atol=0.0), ((i1, i2), fit, ref)
        nnz = np.count_nonzero(metric[:, i1:i2 + 1] > 0.0, axis=1)
        assert np.array_equal(fit == 0.0, nnz == 0), (i1, i2)
        if nnz[LOG_LAYER] == 0:
            none.append((i1, i2))
        elif nnz[LOG_LAYER] < i2 - i1 + 1:
            some.append((i1, i2))
            # the count really scales the fit: without the factor nnz / ntot it would be off by far more than the tolerance
            assert nnz[LOG_LAYER] / (i2 - i1 + 1) < 1.0 - 1e-6
    assert (255, 256) in none and (257, 511) in none and (1, 510) in some and (0, n - 1) in some, (none, some)


@pytest.mark.parametrize("nlay,method", [(54, "transmission"), (30, "transmission"), (12, "transmission"),
                                         (30, "logarithmic"), (12, "linear")])
def test_errors_match_the_oracle(gases, oracle, nlay, method):
    """b. ecckd_calc_error_multi of every listed interval (one batch, the table in the kernel arguments) against the oracle's
    calc_error over the same slice."""
    gas = gases.lw(nlay, method)
    iv, _ = _case_intervals(LW_CASES[nlay])
    assert len(iv) <= 64
    err = _errors(gas, iv)
    ref = _lw_reference_errors(oracle, nlay, method, _num_cu())
    assert np.all(np.isfinite(err)) and np.all(np.isfinite(ref))
    _assert_close(f"errors {nlay} layers {method}", iv, err, ref, ERR_RTOL, 1e-12)


def _sw_albedos(iv):
    """The list with a band albedo per interval (0.15 and 0, alternating), and six of its intervals once more with the other
    one: two otherwise equal intervals that differ in the `albedo` field of the interval table alone."""
    twice = [iv.index(x) for x in [(1, 510), (255, 767), (S, 2 * S), (S - 257, 2 * S + 256), (I0, I0 + 255), (I0, I0 + 512 - 1)]]
    alb = [0.15 if k % 2 == 0 else 0.0 for k in range(len(iv))]
    return iv + [iv[k] for k in twice], np.array(alb + [0.15 - alb[k] for k in twice]), twice


@pytest.mark.parametrize("nlay", [54, 12])
def test_shortwave_fits_and_errors_match_the_oracle(gases, oracle, nlay):
    """c. The same list through a shortwave gas: fits against the oracle's shortwave fit, errors - each interval with its own
    band albedo - against the oracle's shortwave calc_error over the same slice; tolerances of test_find_g_sw_gpu.py."""
    c, o = SW_CASES[nlay], _sw_case(oracle, nlay)
    method, n = c["method"], c["n"]
    gas = gases.sw(nlay)
    iv0, _ = _case_intervals(c)
    L = oracle.lib()
    ssi, bg, od, metric = (np.ascontiguousarray(o[k]) for k in ("ssi_s", "bg_s", "od_s", "metric"))

    def oracle_fit(interval):
        i1, i2 = interval
        ref = np.empty(nlay)
        if method == "total-transmission":
            L.orc_fit_optical_depth_sw_total_trans(C.c_int(nlay), C.c_size_t(n), C.c_size_t(i1), C.c_size_t(i2), oracle._p(ssi),
                                                   oracle._p(bg), oracle._p(od), oracle._p(ref))
        else:
            L.orc_fit_optical_depth_sw(C.c_int(oracle.AVG[method]), C.c_int(nlay), C.c_size_t(n), C.c_size_t(i1), C.c_size_t(i2),
                                       oracle._p(ssi), oracle._p(metric), oracle._p(ref))
        return ref
    for (i1, i2), ref in zip(iv0, _in_threads(oracle_fit, iv0)):
        fit = gas.fit_optical_depth(i1, i2 - i1 + 1, [0.0], [1.0])[0]
        assert np.array_equal(np.isinf(fit), np.isinf(ref)) and np.array_equal(np.isnan(fit), np.isnan(ref)), (i1, i2)
        m = np.isfinite(ref)
        assert np.allclose(fit[m], ref[m], rtol=1e-7, atol=1e-13), ((i1, i2), fit, ref)
    iv, alb, twice = _sw_albedos(iv0)
    assert len(iv) <= 64
    err = _errors(gas, iv, alb)
    ref = _oracle_errors(oracle, sw._oracle_eq(oracle, o, method, FLUX_WEIGHT, 0.0), iv, alb)
    assert np.isfinite(ref).sum() >= len(iv) - 8
    _assert_close(f"shortwave errors {nlay} layers {method}", iv, err, ref, sw.ERR_RTOL, 1e-10)
    # the albedo matters: else this test would not notice one taken from a neighbour's entry
    pairs = [(k, len(iv0) + j) for j, k in enumerate(twice) if np.isfinite(ref[k]) and np.isfinite(ref[len(iv0) + j])]
    assert len(pairs) >= 4
    for k, k2 in pairs:
        assert abs(ref[k] - ref[k2]) > 1e-6 * abs(ref[k]) + 1e-8, iv[k]


@pytest.mark.parametrize("kind", ["lw", "sw"])
def test_table_route_gives_the_bits_of_the_argument_route(gases, kind):
    """d. More than KARG_MAX = 64 intervals in a batch go through a copied table, up to 64 in the kernel arguments; an
    interval's error has the same bits either way and alone.  129 = 65 + 64 intervals (the list, repeated): as one batch, as
    a batch of exactly 65 and one of exactly 64, the first 64 again, and every interval of the list alone."""
    if kind == "lw":
        gas, (iv0, _), alb0 = gases.lw(54, "transmission"), _case_intervals(LW_CASES[54]), None
    else:
        gas, (iv0, _) = gases.sw(54), _case_intervals(SW_CASES[54])
        iv0, alb0, _ = _sw_albedos(iv0)
    reps = -(-129 // len(iv0))
    iv = (iv0 * reps)[:129]
    alb = None if alb0 is None else np.tile(alb0, reps)[:129]
    part = lambda a, b: _errors(gas, iv[a:b], None if alb is None else alb[a:b])
    e_all = part(0, 129)
    assert np.all(np.isfinite(e_all) | np.isnan(e_all)) and np.isfinite(e_all).sum() >= 100
    same = lambda x, y: np.array_equal(x, y, equal_nan=True)
    assert same(np.concatenate([part(0, 65), part(65, 129)]), e_all)            # table | arguments
    assert same(part(0, 64), e_all[:64])                                        # arguments
    assert same(np.concatenate([part(0, 32), part(32, 64), part(64, 96), part(96, 129)]), e_all)
    alone = np.array([part(k, k + 1)[0] for k in range(len(iv0))])
    assert same(alone, e_all[:len(iv0)])
    assert same(e_all[len(iv0):2 * len(iv0)], e_all[:len(iv0)])                 # the repeats, at other places of the table


def test_fit_and_error_do_not_depend_on_the_alignment(gases, oracle):
    """e. One length (2 S + 513 points: head, head tiles, a super tile, tiles behind, tail) at five alignments of its start:
    a head / tail slip that depends on the alignment, not on the length."""
    nlay, method = 30, "transmission"
    gas = gases.lw(nlay, method)
    a_of, b_of = gases.lw_sums(nlay, method)
    iv = [(i1, i1 + 2 * S + 513 - 1) for i1 in (0, 1, 255, 256, I0)]
    for i1, i2 in iv:
        fit = gas.fit_optical_depth(i1, i2 - i1 + 1, [0.0], [1.0])[0]
        assert max(_fit_multiples(method, fit, a_of(i1, i2), b_of(i1, i2))) <= 1.0, (i1, i2)
    ref = _oracle_errors_lw(oracle, _lw_case(oracle, nlay, method), method, iv)
    _assert_close("errors at five alignments", iv, _errors(gas, iv), ref, ERR_RTOL, 1e-12)
