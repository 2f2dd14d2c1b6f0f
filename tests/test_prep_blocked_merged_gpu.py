"""A 54-layer longwave gas whose background is given as the list of spectra it is merged from (api.GasLW(bg_sources=...),
ecckd_gas_create_lw_merged): the merge happens inside the scatter that brings the columns into rank order, and the
preparation kernel stores the operands of the sweep line-blocked itself (k_gas_prep_lw_mirror<.., true>, csrc/find_g.hip),
testing a DOUBLE background for values that are no floats on the way.  Only where values are computed and stored changes,
so nothing here has a tolerance.

The comparator is the path that is left as it was: api.GasLW(bg_optical_depth=M) made with ECCKD_RT_ROWMAJOR=1 (row-major
matrices, k_pack_bg32 after the preparation, no blocked stores), M built by api.merge_spectrum source after source; M is
also restated in float64 numpy - the product, then the sum, in order (numpy does not fuse).

Compared bit for bit: the views bg_optical_depth, planck_hl, hr, weighted_metric, flux_dn_surf, flux_up_toa; the bytes the
sweep reads per point; the errors of a batch of intervals (first indices off a line, a one-point interval, the whole band).

  nwav 16     one line, one live quarter wave
  nwav 1 168  73 lines - no multiple of 64 or 128: the last scatter block, the last K4 pair and the last wave are ragged
  nwav 4 112  several K4 blocks plus one line
  nwav 1 000  rows that are no whole lines: the new entry lands on the row-major layout

with 1, 2 and 5 FLOAT sources (per-layer factors that are no powers of two), a DOUBLE source among FLOAT ones, and none;
with and without the first gas's Planck matrix (the reusing gas attaches to the blocked copy the first gas's preparation
wrote); a float-exact background (one FLOAT source, factor 1.0), which must end as FLOAT pairs; the new entry under each of
ECCKD_RT_ROWMAJOR, ECCKD_RT_UNALIGNED and ECCKD_BG64; and what the entry refuses."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ecckd_amd import synthetic as syn

pytestmark = pytest.mark.gpu

NLAY = 54
METHOD, FLUX_WEIGHT = "transmission", 0.02
VIEWS = ("bg_optical_depth", "planck_hl", "hr", "weighted_metric", "flux_dn_surf", "flux_up_toa")
SIZES = (16, 1168, 4112, 1000)
KNOBS = ("ECCKD_RT_ROWMAJOR", "ECCKD_RT_UNALIGNED", "ECCKD_BG64")
# kind -> the dtypes of the sources
KINDS = {"float1": ("f4",), "float2": ("f4",) * 2, "float5": ("f4",) * 5, "mixed": ("f4", "f8", "f4"), "none": ()}


@pytest.fixture(autouse=True)
def _every_request_on_the_device(monkeypatch):
    monkeypatch.setenv("ECCKD_NO_ERROR_MEMO", "1")
    for knob in KNOBS + ("ECCKD_RT_GENERIC",):
        monkeypatch.delenv(knob, raising=False)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """Host arrays of a problem of n points: target spectrum (FLOAT), five FLOAT and one DOUBLE background spectrum, factors
    [6][NLAY] that are no powers of two, and a rank that is a permutation without any order in it."""
    p = syn.pressure_grid(NLAY)
    wn, dwn = syn.wavenumber_grid(n)
    rng = np.random.default_rng(4000 + n)
    spectra = [syn.optical_depth(np, p, wn, syn.SEED_BASE + 7 * k, nlines=8, column_scale=3.0 + k).astype(np.float32) for k in range(6)]
    wide = syn.optical_depth(np, p, wn, syn.SEED_BASE + 99, nlines=8, column_scale=2.0).astype(np.float64) * (1.0 + 2.0 ** -40)
    assert np.any(wide.astype(np.float32).astype(np.float64) != wide)           # a DOUBLE source whose values are no floats
    scale = 0.3701 + 0.0131 * np.arange(NLAY)[None, :] + 0.2117 * np.arange(6)[:, None]
    assert not np.any(np.log2(scale) == np.round(np.log2(scale)))
    return dict(p=p, t_hl=syn.temperature_profile(p), wn=wn, dwn=dwn, rank=rng.permutation(n).astype(np.int32), od=spectra[0],
                f4=spectra[1:], f8=wide, scale=scale)


def _dev(ctx, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)


def _sources(ctx, inp, kind, scale=None):
    """[(device tensor, factors[NLAY])] of a kind, and the same on the host."""
    host, nf = [], 0
    for s, dt in enumerate(KINDS[kind]):
        if dt == "f4":
            host.append((inp["f4"][nf], inp["scale"][s] if scale is None else np.full(NLAY, scale)))
            nf += 1
        else:
            host.append((inp["f8"], inp["scale"][s]))
    return [(_dev(ctx, od), sp) for od, sp in host], host


def _merged_numpy(host):
    m = None
    for od, sp in host:
        term = od.astype(np.float64) * sp[:, None]
        m = term if m is None else m + term
    return m


def _new(ctx, inp, src, **kw):
    from ecckd_amd import api
    return api.GasLW(ctx, inp["p"], inp["t_hl"], _dev(ctx, inp["wn"]), _dev(ctx, inp["dwn"]), _dev(ctx, inp["rank"]), _dev(ctx, inp["od"]),
                     None, METHOD, FLUX_WEIGHT, bg_sources=src, **kw)


def _comparator(ctx, monkeypatch, inp, src, host, **kw):
    """The gas of the merged matrix on the path left as it was; the matrix is checked against numpy on the way."""
    from ecckd_amd import api
    merged = None
    for od, sp in src:
        merged = api.merge_spectrum(ctx, od, sp, merged)
    if merged is not None:
        ctx.synchronize()
        assert np.array_equal(merged.cpu().numpy(), _merged_numpy(host))
    monkeypatch.setenv("ECCKD_RT_ROWMAJOR", "1")
    gas = api.GasLW(ctx, inp["p"], inp["t_hl"], _dev(ctx, inp["wn"]), _dev(ctx, inp["dwn"]), _dev(ctx, inp["rank"]), _dev(ctx, inp["od"]),
                    merged, METHOD, FLUX_WEIGHT, **kw)
    monkeypatch.delenv("ECCKD_RT_ROWMAJOR")
    return gas


def _intervals(n):
    """[(i1, i2)] inclusive: the whole band, first indices 1, 5, 7 and 15 modulo 16, one-point intervals, an end off a line."""
    iv = [(0, n - 1), (1, n - 2), (5, 5), (n - 1, n - 1), (7, min(n - 1, 200)), (15, n - 1), (n // 2, n // 2 + 3)]
    assert all(0 <= a <= b < n for a, b in iv) and {1, 5, 7, 15} <= {a % 16 for a, _ in iv}
    return iv


def _errors(gas, n):
    iv = _intervals(n)
    return gas.calc_error_multi(np.array([a for a, _ in iv]), np.array([b - a + 1 for a, b in iv]), np.zeros(len(iv)), np.ones(len(iv)))


def _is_blocked(gas):
    from ecckd_amd.api import EcckdError
    try:
        return gas.view_ptr("planck_hl_blocked")[0] is not None
    except EcckdError:
        return False


def _same_gas(got, want, n):
    assert got.sweep_bytes_per_point() == want.sweep_bytes_per_point()
    e_got, e_want = _errors(got, n), _errors(want, n)
    assert np.all(np.isfinite(e_want)) and e_want[0] > 0.0
    assert np.array_equal(e_got, e_want)
    for name in VIEWS:
        assert np.array_equal(got.view(name), want.view(name)), name
    assert np.array_equal(_errors(got, n), e_want)            # after the background rows were rebuilt for the view


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", SIZES)
def test_merged_sources_give_the_gas_of_the_merged_matrix(ctx, monkeypatch, n, kind):
    inp = _inputs(n)
    src, host = _sources(ctx, inp, kind)
    want = _comparator(ctx, monkeypatch, inp, src, host)
    got = _new(ctx, inp, src)
    assert _is_blocked(got) == (n % 16 == 0) and not _is_blocked(want)
    # merged from scaled spectra: DOUBLE rows; no background: FLOAT pairs (of zeros)
    assert got.sweep_bytes_per_point() == (NLAY + 1) * 8 + NLAY * (4 if kind == "none" else 8)
    _same_gas(got, want, n)
    if kind != "none":
        ireorder = np.argsort(inp["rank"])
        assert np.array_equal(got.view("bg_optical_depth"), _merged_numpy(host)[:, ireorder])
    if _is_blocked(got):
        # the blocked Planck matrix the preparation wrote is the row-major one in the layout of sweep_layout.hpp
        raw = got.view("planck_hl_blocked")
        assert np.array_equal(raw.reshape(n // 16, NLAY + 1, 16).transpose(1, 0, 2).reshape(NLAY + 1, n), want.view("planck_hl"))
    got.close()
    want.close()


@pytest.mark.parametrize("n", (1168, 1000))
def test_reusing_gas_attaches_to_the_first_gas_s_blocked_planck_matrix(ctx, monkeypatch, n):
    inp = _inputs(n)
    src, host = _sources(ctx, inp, "float2")
    src5, host5 = _sources(ctx, inp, "float5")
    first = _new(ctx, inp, src)
    second = _new(ctx, inp, src5, planck_hl_reuse=first.view_ptr("planck_hl")[0])
    want_first = _comparator(ctx, monkeypatch, inp, src, host)
    want_second = _comparator(ctx, monkeypatch, inp, src5, host5, planck_hl_reuse=want_first.view_ptr("planck_hl")[0])
    if n % 16 == 0:
        assert _is_blocked(first) and second.view_ptr("planck_hl_blocked")[0] == first.view_ptr("planck_hl_blocked")[0]
    else:
        assert not _is_blocked(first) and not _is_blocked(second)
    _same_gas(second, want_second, n)
    _same_gas(first, want_first, n)
    first.close()                                              # the copy lives on with its second holder
    assert np.array_equal(_errors(second, n), _errors(want_second, n))
    for g in (second, want_second, want_first):
        g.close()


@pytest.mark.parametrize("n", (16, 1168, 1000))
def test_float_exact_background_ends_as_float_pairs(ctx, monkeypatch, n):
    """One FLOAT source with the factor 1.0: every merged value is a float."""
    inp = _inputs(n)
    src, host = _sources(ctx, inp, "float1", scale=1.0)
    want = _comparator(ctx, monkeypatch, inp, src, host)
    got = _new(ctx, inp, src)
    assert got.sweep_bytes_per_point() == (NLAY + 1) * 8 + NLAY * 4
    assert _is_blocked(got) == (n % 16 == 0)
    _same_gas(got, want, n)
    got.close()
    want.close()


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("kind", ("float2", "mixed"))
def test_new_entry_under_the_knobs(ctx, monkeypatch, knob, kind):
    """The knob holds for both gases; the comparator is row-major under every one of them."""
    n = 1168
    inp = _inputs(n)
    src, host = _sources(ctx, inp, kind)
    monkeypatch.setenv(knob, "1")
    want = _comparator(ctx, monkeypatch, inp, src, host)
    monkeypatch.setenv(knob, "1")                              # (the comparator took ECCKD_RT_ROWMAJOR away again)
    got = _new(ctx, inp, src)
    monkeypatch.delenv(knob)
    # ECCKD_RT_ROWMAJOR and ECCKD_RT_UNALIGNED: no blocked operands; ECCKD_BG64: DOUBLE rows, blocked by the copy as before
    assert _is_blocked(got) == (knob == "ECCKD_BG64")
    _same_gas(got, want, n)
    got.close()
    want.close()


def test_a_log_metric_gas_takes_the_temporary(ctx, monkeypatch):
    """Off the column-staged path (here: the logarithmic method) the entry merges into a temporary and runs the one body."""
    from ecckd_amd import api
    n = 1168
    inp = _inputs(n)
    src, host = _sources(ctx, inp, "mixed")
    args = (ctx, inp["p"], inp["t_hl"], _dev(ctx, inp["wn"]), _dev(ctx, inp["dwn"]), _dev(ctx, inp["rank"]), _dev(ctx, inp["od"]))
    merged = None
    for od, sp in src:
        merged = api.merge_spectrum(ctx, od, sp, merged)
    want = api.GasLW(*args, merged, "logarithmic", FLUX_WEIGHT)
    got = api.GasLW(*args, None, "logarithmic", FLUX_WEIGHT, bg_sources=src)
    _same_gas(got, want, n)
    got.close()
    want.close()


def test_refusals(ctx):
    from ecckd_amd import api, _lib
    n = 1168
    inp = _inputs(n)
    src, _ = _sources(ctx, inp, "float2")
    with pytest.raises(api.EcckdError, match="not both"):
        api.GasLW(ctx, inp["p"], inp["t_hl"], _dev(ctx, inp["wn"]), _dev(ctx, inp["dwn"]), _dev(ctx, inp["rank"]), _dev(ctx, inp["od"]),
                  src[0][0], METHOD, FLUX_WEIGHT, bg_sources=src)
    keep = [_dev(ctx, inp[k]) for k in ("wn", "dwn", "rank", "od")]
    p, t = np.ascontiguousarray(inp["p"]), np.ascontiguousarray(inp["t_hl"])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    scale = np.ascontiguousarray(inp["scale"][:2])

    def create(nbg, ptrs, types, strides):
        h = C.c_void_p()
        rc = ctx.lib.ecckd_gas_create_lw_merged(
            ctx.handle, NLAY, n, dp(p), dp(t), C.c_void_p(keep[0].data_ptr()), C.c_void_p(keep[1].data_ptr()),
            C.c_void_p(keep[2].data_ptr()), nbg, (C.c_void_p * 2)(*ptrs), (C.c_int * 2)(*types), (C.c_size_t * 2)(*strides), dp(scale),
            C.c_void_p(keep[3].data_ptr()), _lib.F32, n, _lib.AVG[METHOD], FLUX_WEIGHT, 0.0, None, C.byref(h))
        assert h.value is None
        api.check(rc)

    good = [od.data_ptr() for od, _ in src]
    with pytest.raises(api.EcckdError, match=r"nbg \(-1\) must be between 0 and 16"):
        create(-1, good, [_lib.F32] * 2, [n, n])
    with pytest.raises(api.EcckdError, match=r"d_bg_od\[1\] is NULL"):
        create(2, [good[0], None], [_lib.F32] * 2, [n, n])
    with pytest.raises(api.EcckdError, match=r"bg_stride\[0\] \(1167\) < nwav \(1168\)"):
        create(2, good, [_lib.F32] * 2, [n - 1, n])
    with pytest.raises(api.EcckdError, match=r"bg_type\[1\] must be 4 or 8"):
        create(2, good, [_lib.F32, 5], [n, n])
    ctx.synchronize()
