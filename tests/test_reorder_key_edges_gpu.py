"""The kernels that produce the sort's input at the edges of their own code: the sorting keys of csrc/reorder.hip - generic
longwave (block size halved at 81 and 161 layers, 160 KiB of LDS at 80, 160 and 320), the 54-layer fast path, shortwave - and
the merge kernels of csrc/merge.hip.  Inputs and references are those of reorder_key_cases.py; test_reorder_key_cases.py holds
them against the oracle on the CPU.

Longwave key on designed optical depths ({0} U [1e-3, 60] per layer), metric |delta| / max(|ref|, 1e-3):
    ORACLE_DIST = 3.0e-14   oracle <-> np.longdouble restatement (measured 2.927e-14 on the CPU)
    TOL         = 6.0e-13   = 20 ORACLE_DIST, the bound of the device against BOTH
    device      = 2.75e-14  largest distance to the long-double value measured on an MI355X over the 47 cases x 2 thresholds
                            (1.81e-14 to the oracle): 5 % of TOL.  Fast path, with its single exp per layer and its scalar
                            exp: 2.75e-14 / 1.81e-14; generic kernel: 1.46e-14 / 1.57e-14
The launches of exactly 160 KiB of dynamic LDS (80, 160 and 320 layers) are accepted by the runtime and give these figures.
The column optical depth is bit-equal everywhere.  Shortwave keys: bit-equal to closed forms where one interpolation term is
zero, rtol 1e-14 otherwise (the two-term interpolation is contracted to an FMA).  merge.hip: bit-equal.

90 tests, 2.7 s on one MI355X, host references included; the slowest 0.09 s."""
import ctypes as C

import numpy as np
import pytest
import torch

import reorder_key_cases as K

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _dev(ctx, a):
    return torch.as_tensor(np.array(a, order="C"), device=ctx.device)      # a copy: the shared inputs are read-only


def _dev_rows(ctx, od, strided, fill=NAN):
    """od on the device: contiguous, or a view of a tensor whose rows are STRIDE_PAD elements longer, the padding `fill`."""
    if not strided:
        return _dev(ctx, od)
    nlay, nwav = od.shape
    wide = np.full((nlay, nwav + K.STRIDE_PAD), fill, dtype=od.dtype)
    wide[:, :nwav] = od
    view = _dev(ctx, wide)[:, :nwav]
    assert view.stride(0) == nwav + K.STRIDE_PAD or nlay == 1
    return view


def _within(key, ref, bound):
    return K.key_distance(key, ref) <= bound


# --------------------------------------------------------------------------------- a. longwave key, layer count and block edges

@pytest.mark.parametrize("case", K.GEOMETRY, ids=K.geometry_id)
def test_lw_key_at_layer_count_and_block_edges(ctx, oracle, case):
    from ecckd_amd import api
    p, t, wn, dwn, od = K.geometry_inputs(case)
    d_od = _dev_rows(ctx, od, case.strided)
    d_wn, d_dwn = _dev(ctx, wn), _dev(ctx, dwn)
    for thr in K.THRESHOLDS:
        ref, _ = K.geometry_reference(case, thr)
        okey, ocol, status = oracle.reorder_key(p, t, wn, dwn, od.astype(np.float64), None, thr)
        assert status == 0
        key, col = api.reorder_key_lw(ctx, p, t, d_wn, d_dwn, d_od, thr)
        key, col = key.cpu().numpy(), col.cpu().numpy()
        d_ref, d_orc = K.key_distance(key, ref), K.key_distance(key, okey)
        print("%s thr %.1f: device <-> long double %.3g, device <-> oracle %.3g (TOL %.3g)"
              % (K.geometry_id(case), thr, d_ref, d_orc, K.TOL))
        assert np.array_equal(col, ocol)
        assert np.array_equal(np.isnan(key), np.isnan(ref.astype(np.float64)))
        assert np.array_equal(np.isnan(key), np.isnan(okey))
        assert d_ref <= K.TOL
        assert d_orc <= K.TOL


def test_lw_key_layer_count_limit(ctx, oracle):
    from ecckd_amd import api, EcckdError
    for nlay in (320, 321):
        p = K.pressure_grid(nlay)
        t = K.idealised_temperature(p)
        wn, dwn = K.wavenumber_grid(3)
        od = K.designed_od(nlay, 3, "float64", 9)
        args = (ctx, p, t, _dev(ctx, wn), _dev(ctx, dwn), _dev(ctx, od), 0.5)
        if nlay == 321:
            with pytest.raises(EcckdError) as e:
                api.reorder_key_lw(*args)
            assert e.value.code == 147 and "supported maximum (320)" in e.value.message
        else:
            key, col = api.reorder_key_lw(*args)
            okey, ocol, _ = oracle.reorder_key(p, t, wn, dwn, od, None, 0.5)
            assert np.array_equal(col.cpu().numpy(), ocol) and _within(key.cpu().numpy(), okey, K.TOL)


# -------------------------------------------------------------------------------------- b. threshold edges, all three kernels

def _check_sw_closed_forms(key, col, od, want, exact):
    assert np.array_equal(col, K.sequential_column(od))
    assert np.array_equal(key[exact], want[exact])
    assert np.allclose(key[~exact], want[~exact], rtol=1e-14, atol=0)


@pytest.mark.parametrize("nlay", [4, 54], ids=["generic-grid", "54-layer-grid"])
@pytest.mark.parametrize("thr", [0.5, 0.0])
def test_sw_key_threshold_edges(ctx, oracle, thr, nlay):
    """The hand-built columns at threads 0, 255, 256 and 512 against their closed forms; as float32 (where `one ulp below`
    rounds to `col == thr`) against the oracle."""
    from ecckd_amd import api
    p = K.THRESHOLD_PRESSURE if nlay == 4 else K.pressure_grid(nlay)
    ph = K.pseudo_height_hl(p)
    for shift in range(len(K.THRESHOLD_COLUMNS)):
        od = K.threshold_od(shift, nlay)
        want, exact = K.threshold_expected_sw(shift, ph, thr)
        key, col = api.reorder_key_sw(ctx, p, _dev(ctx, od), thr)
        _check_sw_closed_forms(key.cpu().numpy(), col.cpu().numpy(), od, want, exact)
    od32 = K.threshold_od(5, nlay, "float32")
    n = od32.shape[1]
    okey, ocol, status = oracle.reorder_key(p, None, np.ones(n), np.ones(n), od32.astype(np.float64), np.ones(n), thr)
    key, col = api.reorder_key_sw(ctx, p, _dev(ctx, od32), thr)
    assert status == 0 and np.array_equal(col.cpu().numpy(), ocol)
    assert np.allclose(key.cpu().numpy(), okey, rtol=1e-14, atol=0)


@pytest.mark.parametrize("nlay", [4, 54], ids=["generic", "fast-path"])
@pytest.mark.parametrize("thr", [0.5, 0.0])
def test_lw_key_threshold_edges(ctx, oracle, thr, nlay):
    """`thr > 0 && col < thr` gives -thr + col bit for bit - and nothing else does: a column whose sum EQUALS the threshold, or
    lies above it, has the heating-rate key (NaN where it only heats, as in the oracle)."""
    from ecckd_amd import api
    p = K.THRESHOLD_PRESSURE if nlay == 4 else K.pressure_grid(nlay)
    t = api.idealised_temperature(p)
    wn, dwn = K.wavenumber_grid(K.THRESHOLD_NWAV)
    d_wn, d_dwn = _dev(ctx, wn), _dev(ctx, dwn)
    overridden = compared = 0
    for shift in range(len(K.THRESHOLD_COLUMNS)):
        od = K.threshold_od(shift, nlay)
        okey, ocol, status = oracle.reorder_key(p, t, wn, dwn, od, None, thr)
        assert status == 0
        key, col = api.reorder_key_lw(ctx, p, t, d_wn, d_dwn, _dev(ctx, od), thr)
        key, col = key.cpu().numpy(), col.cpu().numpy()
        assert np.array_equal(col, ocol)
        under = (col < thr) & (thr > 0.0)
        assert np.array_equal(key[under], (-thr + col)[under])
        rest = ~under & (K.threshold_pattern(shift) != K.THIN_COLUMN)
        assert np.array_equal(np.isnan(key[rest]), np.isnan(okey[rest]))
        assert _within(key[rest], okey[rest], K.KEY_RTOL)
        overridden += int(under.sum())
        compared += int((rest & ~np.isnan(okey)).sum())
    # thr .5: the zero, the 1e-13 and the one-ulp-below column; thr 0: none
    assert overridden == (3 * K.THRESHOLD_NWAV if thr > 0 else 0) and compared > 0


# -------------------------------------------------------------------------------------------------------- c. the error flag

def _flag_calls(ctx, nlay_generic):
    """(name, nlay, call(p, od, thr) -> (key, col), oracle arguments) for the three kernels; constant 250 K for the longwave."""
    from ecckd_amd import api

    def lw(p, od, thr):
        n = od.shape[1]
        wn = np.linspace(100.0, 2000.0, n)
        return api.reorder_key_lw(ctx, p, np.full(p.size, 250.0), _dev(ctx, wn), _dev(ctx, np.ones(n)), _dev(ctx, od), thr)

    def sw(p, od, thr):
        return api.reorder_key_sw(ctx, p, _dev(ctx, od), thr)

    return (("shortwave", nlay_generic, sw, True), ("longwave generic", nlay_generic, lw, False),
            ("longwave fast path", 54, lw, False), ("shortwave 54", 54, sw, True))


def _flag_oracle(oracle, p, od, thr, shortwave):
    n = od.shape[1]
    return oracle.reorder_key(p, np.full(p.size, 250.0), np.linspace(100.0, 2000.0, n), np.ones(n), od,
                              np.ones(n) if shortwave else None, thr)


def _matches_oracle(oracle, call, p, od, thr, shortwave):
    okey, ocol, status = _flag_oracle(oracle, p, od, thr, shortwave)
    assert status == 0
    key, col = call(p, od, thr)
    key, col = key.cpu().numpy(), col.cpu().numpy()
    assert np.array_equal(col, ocol)
    if shortwave:
        assert np.allclose(key, okey, rtol=1e-14, atol=0)
    else:
        assert np.array_equal(np.isnan(key), np.isnan(okey)) and _within(key, okey, K.KEY_RTOL)


def test_error_flag_from_the_last_block_and_cleared_for_the_next_call(ctx, oracle):
    """One column of 301, in the second block, whose threshold height exceeds 30: PROCESSING_ERROR from all three kernels; the
    next call on the same context, without that column, succeeds and matches the oracle; so does the full call under a top
    level at pseudo height 29.5."""
    from ecckd_amd import api, EcckdError
    for name, nlay, call, shortwave in _flag_calls(ctx, 2):
        high, low = K.flag_pressure(nlay, 30.5), K.flag_pressure(nlay, 29.5)
        bad, harmless = K.flag_od(nlay, "offending"), K.flag_od(nlay, "harmless")
        assert _flag_oracle(oracle, high, bad, K.FLAG_THR, shortwave)[2] == 1
        with pytest.raises(EcckdError) as e:
            call(high, bad, K.FLAG_THR)
        assert e.value.code == 148 and "threshold pseudo-height exceeds 30" in e.value.message, name
        _matches_oracle(oracle, call, high, harmless, K.FLAG_THR, shortwave)          # the flag did not stick
        _matches_oracle(oracle, call, low, bad, K.FLAG_THR, shortwave)
        if not shortwave:
            # the idealised temperature is negative at such pressures: refused before the kernel runs
            n = bad.shape[1]
            with pytest.raises(EcckdError) as e:
                api.reorder_key_lw(ctx, high, api.idealised_temperature(high), _dev(ctx, np.linspace(100.0, 2000.0, n)),
                                   _dev(ctx, np.ones(n)), _dev(ctx, bad), K.FLAG_THR)
            assert e.value.code == 147 and "temperature_hl must be positive" in e.value.message, name


def test_error_flag_tells_the_latch_of_each_kernel(ctx, oracle):
    """Two levels above pseudo height 30.  thr = 0: every column crosses in its empty top layer (0 >= 0) at height 0, no
    refusal.  thr = .25 and the column (.25, 0, 1, ...): it crosses ON level 1, at 30.2 - a refusal; a latch written with `>`
    would find level 2 at 29.4.  In the longwave kernels the flag is all that shows of the threshold height."""
    from ecckd_amd import EcckdError
    for name, nlay, call, shortwave in _flag_calls(ctx, 3):
        p = K.flag_pressure(nlay, 30.5, 30.2)
        harmless, bad = K.flag_od(nlay, "latch_harmless"), K.flag_od(nlay, "latch_offending")
        _matches_oracle(oracle, call, p, harmless, 0.0, shortwave)
        assert _flag_oracle(oracle, p, bad, K.FLAG_THR, shortwave)[2] == 1
        with pytest.raises(EcckdError) as e:
            call(p, bad, K.FLAG_THR)
        assert e.value.code == 148, name
        _matches_oracle(oracle, call, p, harmless, K.FLAG_THR, shortwave)


# ------------------------------------------------------------------------------------------------ d. shortwave key geometry

@pytest.mark.parametrize("case", K.SW_GEOMETRY, ids=K.geometry_id)
def test_sw_key_geometry(ctx, oracle, case):
    from ecckd_amd import api
    p = K.pressure_grid(case.nlay)
    od = K.sw_od(case)
    n = case.nwav
    okey, ocol, status = oracle.reorder_key(p, None, np.ones(n), np.ones(n), od.astype(np.float64), np.ones(n), K.SW_THR)
    assert status == 0
    key, col = api.reorder_key_sw(ctx, p, _dev_rows(ctx, od, case.strided), K.SW_THR)
    assert np.array_equal(col.cpu().numpy(), K.sequential_column(od))
    assert np.array_equal(ocol, K.sequential_column(od))
    assert np.allclose(key.cpu().numpy(), okey, rtol=1e-14, atol=0)


def test_sw_key_refuses_rows_that_are_not_contiguous(ctx):
    from ecckd_amd import api, EcckdError
    od = torch.ones((2, 16), dtype=torch.float64, device=ctx.device)
    p = K.pressure_grid(2)
    with pytest.raises(EcckdError) as e:
        api.reorder_key_sw(ctx, p, od[:, ::2], 0.25)
    assert e.value.code == 147 and "contiguous" in e.value.message
    with pytest.raises(EcckdError) as e:
        api.reorder_key_lw(ctx, p, [200.0, 210.0, 220.0], od[0, :8], od[0, :8], od[:, ::2], 0.25)
    assert e.value.code == 147 and "contiguous" in e.value.message
    key, col = api.reorder_key_sw(ctx, p, od[:, :8], 0.25)                   # a row stride alone is fine
    assert col.cpu().tolist() == [2.0] * 8


# ------------------------------------------------------------------------------------------------------------- e. merge.hip

@pytest.mark.parametrize("n", [3, 4, 256, 257])
def test_derive_d_wavenumber_sizes(ctx, n):
    from ecckd_amd import api
    wn = np.cumsum(np.random.RandomState(n).uniform(1e-4, 2e-3, n)) + 250.0
    got = api.derive_d_wavenumber(ctx, _dev(ctx, wn)).cpu().numpy()
    assert np.array_equal(got, K.derive_d_wavenumber(wn))


def test_derive_d_wavenumber_refuses_two_points(ctx):
    from ecckd_amd import api, EcckdError
    with pytest.raises(EcckdError) as e:
        api.derive_d_wavenumber(ctx, _dev(ctx, np.array([1.0, 2.0])))
    assert e.value.code == 147 and "at least 3" in e.value.message


@pytest.mark.parametrize("nlay,nwav", K.MERGE_SHAPES)
def test_merge_spectrum_strides_first_and_padding(ctx, nlay, nwav):
    """ecckd_merge_spectrum_dev called directly: od_stride = nwav + 3, merged_stride = nwav + 5; a float32 gas stored with
    first = 1 over NaN, a float64 gas added; the padding of the output keeps its sentinel, that of the inputs is NaN."""
    from ecckd_amd import api
    gases = K.merge_gases(nlay, nwav)
    out_stride = nwav + 5
    start = np.full((nlay, out_stride), K.MERGE_SENTINEL)
    start[:, :nwav] = NAN
    d_merged = _dev(ctx, start)
    wants = []
    for i, (od, scale) in enumerate(gases):
        d_od = _dev_rows(ctx, od, True)
        ctx.fence_from_torch()
        api.check(ctx.lib.ecckd_merge_spectrum_dev(ctx.handle, nlay, nwav, C.c_void_p(d_od.data_ptr()), od.dtype.itemsize,
                                                   nwav + K.STRIDE_PAD, scale.ctypes.data_as(C.POINTER(C.c_double)),
                                                   int(i == 0), C.c_void_p(d_merged.data_ptr()), out_stride))
        got = d_merged.cpu().numpy()
        want = K.merge_expected(gases[:i + 1])
        wants.append(want)
        assert np.array_equal(got[:, :nwav], want, equal_nan=True), "after gas %d" % i
        assert np.all(got[:, nwav:] == K.MERGE_SENTINEL)
    with np.errstate(invalid="ignore"):
        plain = gases[0][0].astype(np.float64) * gases[0][1][:, None]
    assert np.array_equal(wants[0], plain) and not np.isnan(wants[0]).any()      # first = 1 did not read the NaNs
    assert np.isnan(wants[1][nlay - 1, nwav // 2])                               # 0 x inf, as numpy
    assert np.isnan(wants[1]).sum() == 1


def test_merge_spectrum_api_strided_view_and_bad_strides(ctx):
    from ecckd_amd import api, EcckdError
    nlay, nwav = 12, 257
    gases = K.merge_gases(nlay, nwav)
    merged = None
    for od, scale in gases:
        merged = api.merge_spectrum(ctx, _dev_rows(ctx, od, True), scale, merged)
    assert np.array_equal(merged.cpu().numpy(), K.merge_expected(gases), equal_nan=True)
    d_od = _dev(ctx, gases[1][0])
    ctx.fence_from_torch()
    rc = ctx.lib.ecckd_merge_spectrum_dev(ctx.handle, nlay, nwav, C.c_void_p(d_od.data_ptr()), 8, nwav - 1,
                                          gases[1][1].ctypes.data_as(C.POINTER(C.c_double)), 1,
                                          C.c_void_p(merged.data_ptr()), nwav)
    assert rc == 147
    with pytest.raises(EcckdError):
        api.check(rc)


# --------------------------------------------------------------------------------------------------- f. small related items

def test_band_ranges_on_bounds_empty_and_overlapping(oracle):
    from ecckd_amd import api
    wn = np.arange(10, dtype=np.float64) * 10.0                                 # 0, 10, .., 90
    cases = {
        "on the bounds": ([0.0, 30.0, 60.0], [30.0, 60.0, 90.0]),                 # right-open, the last one closed
        "an empty band": ([0.0, 41.0, 50.0], [40.0, 49.0, 90.0]),
        "an empty last band": ([0.0, 50.0, 91.0], [50.0, 80.0, 95.0]),            # 80 and 90 in no band
        "overlapping": ([0.0, 20.0], [50.0, 70.0]),                               # the later band takes 20 .. 40
        "one band, closed": ([10.0], [90.0]),
    }
    for name, (b1, b2) in cases.items():
        iband, begin, end = api.band_ranges(wn, b1, b2)
        oiband, _, _ = oracle.stable_argsort_bands(wn, np.zeros(wn.size), np.array(b1), np.array(b2))
        assert np.array_equal(iband.astype(np.int32), oiband), name
        for b in range(len(b1)):
            last = b == len(b1) - 1
            inside = np.flatnonzero((wn >= b1[b]) & ((wn <= b2[b]) if last else (wn < b2[b])))
            assert (begin[b], end[b]) == ((inside[0], inside[-1]) if inside.size else (0, -1)), (name, b)
    iband, begin, end = api.band_ranges(wn, *cases["on the bounds"])
    assert iband.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2]
    iband, begin, end = api.band_ranges(wn, *cases["an empty band"])
    assert (begin[1], end[1]) == (0, -1) and iband.tolist() == [0, 0, 0, 0, -1, 2, 2, 2, 2, 2]
    iband, begin, end = api.band_ranges(wn, *cases["overlapping"])
    assert iband.tolist() == [0, 0, 1, 1, 1, 1, 1, 1, -1, -1] and (begin[0], end[0]) == (0, 4)


def test_reorder_spectrum_shortwave_branch(ctx, oracle):
    """ecckd_reorder_spectrum with ssi given: the shortwave key, then the band sort, on host arrays."""
    from ecckd_amd import api
    nlay, nwav = 54, 600
    p = K.pressure_grid(nlay)
    wn, dwn = K.wavenumber_grid(nwav, 250.0, 50000.0)
    od = K.sw_od(K.SwCase(nlay, nwav, "float32", False))
    b1, b2 = np.array([250.0, wn[300]]), np.array([wn[300], 50000.0])
    key, col, iband, rank = api.reorder_spectrum(ctx, p, wn, dwn, od, np.ones(nwav), K.SW_THR, b1, b2)
    okey, ocol, status = oracle.reorder_key(p, None, wn, dwn, od.astype(np.float64), np.ones(nwav), K.SW_THR)
    assert status == 0 and np.array_equal(col, ocol)
    assert np.allclose(key, okey, rtol=1e-14, atol=0)
    oiband, _, orank = oracle.stable_argsort_bands(wn, key, b1, b2)
    assert np.array_equal(iband.astype(np.int32), oiband) and np.array_equal(rank, orank)
    assert np.array_equal(np.bincount(iband), [300, 300])
