"""The longwave mirror sweep counts an interval's chunks from the 128-byte line below its first point (csrc/chunk_layout.hpp,
k_rt_lw_bb_mirror of csrc/find_g.hip): the `head` = i1 mod 16 lanes below the first point are dead lanes of the interval's
first tile.  Intervals whose first index is 0, 1 and 15 modulo 16 - inside one line, ending on a line's last point, of 127,
128, 129 and 257 points, starting at the spectrum's last point, and the whole spectrum - on a spectrum of 4 096 + 3 * 16
points, with 54 and 30 layers, DOUBLE background rows and FLOAT pairs:

  a. each error is within ERR_RTOL (test_find_g_gpu.py) of the CPU oracle's calc_error over the same slice;
  b. each error has the same bits alone, in a batch with all the others and through ecckd_calc_error_multi;
  c. a gas made with ECCKD_RT_UNALIGNED=1 (chunks counted from the first point, as before) passes a. as well, gives the
     same bits where the interval starts on a line - the two layouts are one there - and other bits somewhere else: the
     default really is another order of summation;
  d. a spectrum of 4 096 + 7 points - a row is no whole number of lines - gives the same bits with and without the knob:
     head is 0 for both.

Every chunk is one granule of 128 points at these sizes (a round of blocks holds far more), so the whole spectrum has 33
chunks by either count and the 257-point intervals three; what differs is where the chunks begin."""
import functools

import numpy as np
import pytest

from test_find_g_gpu import ERR_RTOL, _lw_problem, _make_gas
from test_interval_edges_gpu import FLUX_WEIGHT, _assert_close, _oracle_errors_lw

pytestmark = pytest.mark.gpu

N = 4096 + 16 * 3
N_ODD = 4096 + 7
METHOD = "transmission"
CASES = [(54, "double"), (54, "float"), (30, "double"), (30, "float")]


@pytest.fixture(autouse=True)
def _every_request_on_the_device(monkeypatch):
    monkeypatch.setenv("ECCKD_NO_ERROR_MEMO", "1")
    monkeypatch.delenv("ECCKD_RT_UNALIGNED", raising=False)
    monkeypatch.delenv("ECCKD_RT_GENERIC", raising=False)
    monkeypatch.delenv("ECCKD_BG64", raising=False)


def intervals(n):
    """[(i1, i2)] inclusive; r = i1 mod 16 in 0, 1, 15."""
    iv = []
    for r in (0, 1, 15):
        iv.append((1024 + r, 1024 + 15 if r == 15 else 1024 + r + 5))      # wholly inside one line (r = 15: its last point alone)
        iv.append((2048 + r, 2048 + 5 * 16 - 1))                           # ends on a line's last point
        for k, m in enumerate((127, 128, 129, 257)):
            iv.append((512 * (k + 1) + 160 + r, 512 * (k + 1) + 160 + r + m - 1))
    last = n - 1
    iv.append((last, last))                                                # starts at the last point
    iv.append((0, last))                                                   # the whole spectrum
    assert all(0 <= a <= b < n for a, b in iv)
    return iv


@functools.lru_cache(maxsize=None)
def _problem(oracle, n, nlay, bg_kind):
    """Host arrays and the oracle's inputs in sorted order; bg_kind "float": a background whose values are floats (kept as
    FLOAT pairs by the gas), with the truth recomputed for it."""
    o = _lw_problem(oracle, n, nlay=nlay, seed=91 + nlay, method=METHOD)
    if bg_kind == "float":
        o = dict(o)
        ireorder = np.argsort(o["rank"])
        o["bg"] = o["bg"].astype(np.float32).astype(np.float64)
        o["bg_s"] = np.ascontiguousarray(o["bg"][:, ireorder])
        fdn, fup = oracle.radiative_transfer_lw(o["planck"], o["bg_s"] + o["od"][:, ireorder], np.ones(n), o["surf_planck"])
        o.update(hr=oracle.heating_rate(o["p"], fdn, fup), fds=fdn[-1].copy(), fut=fup[0].copy())
    return o


@functools.lru_cache(maxsize=None)
def _reference(oracle, nlay, bg_kind):
    return _oracle_errors_lw(oracle, _problem(oracle, N, nlay, bg_kind), METHOD, intervals(N))


def _gas(ctx, o, nlay, bg_kind):
    gas = _make_gas(ctx, o, METHOD, flux_weight=FLUX_WEIGHT, od_dtype=np.float32 if nlay == 54 else np.float64)
    # the sweep under test: FLOAT pairs or DOUBLE rows (ecckd_gas_sweep_bytes_per_point tells which the gas holds)
    assert gas.sweep_bytes_per_point() == (nlay + 1) * 8 + nlay * (4 if bg_kind == "float" else 8)
    return gas


def _alone(gas, iv):
    return np.array([gas.calc_error_batch(a, b - a + 1, [0.0], [1.0])[0] for a, b in iv])


def _multi(gas, iv):
    return gas.calc_error_multi(np.array([a for a, _ in iv]), np.array([b - a + 1 for a, b in iv]), np.zeros(len(iv)), np.ones(len(iv)))


@pytest.mark.parametrize("nlay,bg_kind", CASES)
def test_errors_from_the_aligned_origin(ctx, oracle, monkeypatch, nlay, bg_kind):
    o = _problem(oracle, N, nlay, bg_kind)
    iv = intervals(N)
    assert {a % 16 for a, _ in iv} == {0, 1, 15} and N % 16 == 0
    ref = _reference(oracle, nlay, bg_kind)
    assert np.all(np.isfinite(ref))

    gas = _gas(ctx, o, nlay, bg_kind)
    together = _multi(gas, iv)
    _assert_close(f"a. {nlay} layers, {bg_kind} background", iv, together, ref, ERR_RTOL, 1e-12)
    # b. alone (band = interval), alone through the multi-band entry, all of them in the other order, and as the intervals of
    # ONE band - the spectrum - given by bounds half a point outside their indices (the band length enters the logarithmic
    # fit only)
    assert np.array_equal(_alone(gas, iv), together)
    assert np.array_equal(np.array([_multi(gas, [x])[0] for x in iv]), together)
    assert np.array_equal(_multi(gas, iv[::-1])[::-1], together)
    b1 = np.array([max((a - 0.5) / (N - 1), 0.0) for a, _ in iv])
    b2 = np.array([min((b + 0.5) / (N - 1), 1.0) for _, b in iv])
    assert np.array_equal(gas.calc_error_batch(0, N, b1, b2), together)
    gas.close()

    # c. the layout counted from the first point
    monkeypatch.setenv("ECCKD_RT_UNALIGNED", "1")
    gas = _gas(ctx, o, nlay, bg_kind)
    monkeypatch.delenv("ECCKD_RT_UNALIGNED")
    plain = _multi(gas, iv)
    assert np.array_equal(_multi(gas, iv), plain)          # the knob belongs to the gas: taking it away changes nothing
    gas.close()
    _assert_close(f"c. {nlay} layers, {bg_kind} background, chunks from the first point", iv, plain, ref, ERR_RTOL, 1e-12)
    on_line = np.array([a % 16 == 0 for a, _ in iv])
    assert np.array_equal(plain[on_line], together[on_line])
    assert np.any(plain[~on_line] != together[~on_line])


@pytest.mark.parametrize("nlay,bg_kind", CASES)
def test_rows_that_are_no_whole_lines_keep_their_layout(ctx, oracle, monkeypatch, nlay, bg_kind):
    """d."""
    assert N_ODD % 16 != 0
    o = _problem(oracle, N_ODD, nlay, bg_kind)
    iv = intervals(N_ODD)
    gas = _gas(ctx, o, nlay, bg_kind)
    default = _multi(gas, iv)
    gas.close()
    monkeypatch.setenv("ECCKD_RT_UNALIGNED", "1")
    gas = _gas(ctx, o, nlay, bg_kind)
    plain = _multi(gas, iv)
    gas.close()
    assert np.all(np.isfinite(default)) and np.all(default >= 0.0) and default[-1] > 0.0
    assert np.array_equal(default, plain)
