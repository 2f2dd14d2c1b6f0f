"""CPU checks of the inputs and references of test_reorder_key_edges_gpu.py (reorder_key_cases.py).

On designed_od - every layer optical depth in {0} U [1e-3, 60] - the double oracle and the np.longdouble restatement of the
longwave key have the same NaN positions in every GEOMETRY case with thr 0 and 0.5, and their largest distance under
|delta| / max(|ref|, 1e-3) is

    ORACLE_DIST = 3.0e-14   (measured 2.927e-14)

from which the device bound of the GPU tests follows: TOL = 20 ORACLE_DIST = 6e-13 (the device evaluates the same double
formulas with an exp and a division of < 1 ulp each and FMA contraction: differently rounded, equally accurate).  Largest device
distance measured on an MI355X: 2.75e-14 (test_reorder_key_edges_gpu.py).  The oracle reproduces the closed-form shortwave keys of
THRESHOLD_COLUMNS - bit for bit where one interpolation term is zero -, and every GEOMETRY width lies on the intended side of a
block edge of the independently stated block_threads."""
import math

import numpy as np
import pytest

import reorder_key_cases as K


def test_long_double_is_wider_than_double():
    assert np.finfo(K.L).eps < 2.0 ** -60


def test_restated_grids_are_the_packages(oracle):
    from ecckd_amd import synthetic as syn
    for nlay in K.LAYER_COUNTS:
        p = K.pressure_grid(nlay)
        assert np.array_equal(p, syn.pressure_grid(nlay))
        assert np.allclose(K.idealised_temperature(p), oracle.idealised_temperature(p), rtol=1e-14, atol=0)
    for nwav in (1, 63, 513):
        for a, b in zip(K.wavenumber_grid(nwav), syn.wavenumber_grid(nwav)):
            assert np.array_equal(a, b)


def test_designed_od_stays_out_of_the_thin_regime():
    for c in K.GEOMETRY:
        od = K.geometry_inputs(c)[4]
        assert od.dtype == np.dtype(c.dtype) and od.shape == (c.nlay, c.nwav)
        live = od[od != 0]
        assert live.min() >= np.float32(1e-3) * (1 - 1e-7) and live.max() <= 60.0 * (1 + 1e-7)
        zeros = np.mean(od[:, min(5, c.nwav - 1):] == 0)
        if od.size > 2000:
            assert 0.25 < zeros < 0.35
        assert not od[:, :min(5, c.nwav - 1)].any()


def test_oracle_and_long_double_agree_on_designed_od(oracle, capsys):
    worst, where = 0.0, None
    for c in K.GEOMETRY:
        p, t, wn, dwn, od = K.geometry_inputs(c)
        for thr in K.THRESHOLDS:
            ref, rcol = K.geometry_reference(c, thr)
            okey, ocol, status = oracle.reorder_key(p, t, wn, dwn, od.astype(np.float64), None, thr)
            assert status == 0
            assert np.array_equal(ocol, rcol)
            assert np.array_equal(np.isnan(okey), np.isnan(ref.astype(np.float64))), (c, thr)
            if thr == 0.0 and c.nwav > 5:
                assert np.isnan(okey[:5]).all()                                  # the zero columns: 0 / 0
            d = K.key_distance(okey, ref)
            if d > worst:
                worst, where = d, (K.geometry_id(c), thr)
    with capsys.disabled():
        print("\noracle <-> long double on designed_od: %.4g at %s (ORACLE_DIST %.3g)" % (worst, where, K.ORACLE_DIST))
    # the constant IS this measurement, rounded up: not a looser number
    assert 0.5 * K.ORACLE_DIST < worst <= K.ORACLE_DIST
    assert K.TOL == 20 * K.ORACLE_DIST and K.TOL < K.KEY_RTOL / 1000


def test_thin_layers_are_why_a_designed_input_is_needed(oracle):
    """On layers with tau ~ 1e-6 the oracle is orders of magnitude further from the long-double value: the reason for
    designed_od and for the KEY_RTOL of test_reorder_gpu.py."""
    nlay, nwav = 54, 257
    p = K.pressure_grid(nlay)
    t = K.idealised_temperature(p)
    wn, dwn = K.wavenumber_grid(nwav)
    od = 10.0 ** np.random.RandomState(3).uniform(-6.5, -5.5, (nlay, nwav))
    okey, _, _ = oracle.reorder_key(p, t, wn, dwn, od, None, 0.0)
    ref, _ = K.lw_key_longdouble(p, t, wn, dwn, od, 0.0)
    assert K.key_distance(okey, ref) > 1000 * K.ORACLE_DIST


def test_block_threads_and_geometry_sides():
    assert [K.block_threads(n) for n in (1, 80, 81, 160, 161, 320)] == [256, 256, 128, 128, 64, 64]
    with pytest.raises(ValueError):
        K.block_threads(321)
    for n in K.LAYER_COUNTS:
        b = K.block_threads(n)
        assert n * b * 8 <= 160 * 1024 and (b == 256 or n * 2 * b * 8 > 160 * 1024)
    assert [n * K.block_threads(n) * 8 for n in (80, 160, 320)] == [163840] * 3     # the launches of exactly 160 KiB
    blocks = lambda c: -(-c.nwav // K.block_threads(c.nlay))
    seen = {}
    for c in K.GEOMETRY:
        seen.setdefault(c.nlay, set()).add((c.nwav, blocks(c)))
    for n in K.LAYER_COUNTS:
        b = K.block_threads(n)
        assert (2 * b + 1, 3) in seen[n]                                            # two full blocks and one thread
    for n in K.BLOCK_EDGE_LAYERS:
        b = K.block_threads(n)
        assert {(1, 1), (b - 1, 1), (b, 1), (b + 1, 2), (2 * b + 1, 3)} <= seen[n]
    for n in K.LAYER_COUNTS:
        assert {c.dtype for c in K.GEOMETRY if c.nlay == n} == {"float32", "float64"}
    strided = sorted((c.nlay, c.dtype) for c in K.GEOMETRY if c.strided)
    assert strided == [(54, "float32"), (54, "float64"), (81, "float32")]
    assert all((c.nwav + K.STRIDE_PAD) % 2 == 1 for c in K.GEOMETRY if c.strided)
    assert max(c.nlay * c.nwav for c in K.GEOMETRY) <= 320 * 129


def _sw(oracle, p, od, thr):
    n = od.shape[1]
    return oracle.reorder_key(p, None, np.ones(n), np.ones(n), od.astype(np.float64), np.ones(n), thr)


@pytest.mark.parametrize("thr", [0.5, 0.0])
def test_oracle_reproduces_the_closed_form_shortwave_keys(oracle, thr):
    p = K.THRESHOLD_PRESSURE
    ph = K.pseudo_height_hl(p)
    assert ph[-1] == 0.0 and ph[1] == math.log(1e5) - math.log(10.0)
    for shift in range(len(K.THRESHOLD_COLUMNS)):
        od = K.threshold_od(shift)
        want, exact = K.threshold_expected_sw(shift, ph, thr)
        key, col, status = _sw(oracle, p, od, thr)
        assert status == 0
        assert np.array_equal(col, K.sequential_column(od))
        assert np.array_equal(key[exact], want[exact])
        assert np.allclose(key[~exact], want[~exact], rtol=1e-14, atol=0)
    # the same columns on top of 50 empty layers of the 54-layer grid
    p54 = K.pressure_grid(54)
    ph54 = K.pseudo_height_hl(p54)
    od = K.threshold_od(3, nlay=54)
    want, exact = K.threshold_expected_sw(3, ph54, thr)
    key, col, status = _sw(oracle, p54, od, thr)
    assert status == 0 and np.array_equal(key[exact], want[exact])
    assert np.allclose(key[~exact], want[~exact], rtol=1e-14, atol=0)


def test_threshold_columns_are_what_their_names_say():
    cols = {c.name: np.array(c.od) for c in K.THRESHOLD_COLUMNS}
    assert K.sequential_column(cols["col == thr"][:, None])[0] == 0.5
    below = K.sequential_column(cols["one ulp below thr"][:, None])[0]
    assert below < 0.5 and np.nextafter(below, 1.0) == 0.5
    assert np.cumsum(cols["crossing on level 1"])[0] == 0.5
    assert K.THRESHOLD_COLUMNS[K.THIN_COLUMN].od[0] == 1e-13
    # every column at every one of the four indices, over the eight shifts
    for j in K.THRESHOLD_INDICES:
        assert sorted(K.threshold_pattern(s)[j] for s in range(8)) == list(range(8))
    assert K.THRESHOLD_NWAV == 2 * 256 + 1


def test_flag_cases_cross_where_they_should(oracle):
    for nlay in (2, 54):
        for top, want_status in ((30.5, 1), (29.5, 0)):
            p = K.flag_pressure(nlay, top)
            assert np.all(np.diff(p) > 0) and math.log(p[-1] / p[0]) == pytest.approx(top)
            od = K.flag_od(nlay)
            assert od.shape == (nlay, K.FLAG_HARMLESS + 1) and od[0, K.FLAG_INDEX] == 1.0
            assert K.FLAG_INDEX // 256 == (od.shape[1] - 1) // 256 == 1
            t = np.full(nlay + 1, 250.0)
            n = od.shape[1]
            for ssi in (None, np.ones(n)):
                _, _, status = oracle.reorder_key(p, t, np.linspace(100, 2000, n), np.ones(n), od, ssi, K.FLAG_THR)
                assert status == want_status
            harmless = K.flag_od(nlay, "harmless")
            assert harmless.shape == (nlay, K.FLAG_HARMLESS)
            _, _, status = oracle.reorder_key(p, t, np.linspace(100, 2000, n - 1), np.ones(n - 1), harmless, None, K.FLAG_THR)
            assert status == 0
            # the idealised profile is negative up there: the longwave entry must be given another one
            assert K.idealised_temperature(p)[0] < 0


def test_latch_cases_tell_greater_equal_from_greater(oracle):
    for nlay in (3, 54):
        p = K.flag_pressure(nlay, 30.5, 30.2)
        ph = K.pseudo_height_hl(p)
        assert np.all(np.diff(p) > 0) and ph[0] > ph[1] > 30.0 > ph[2]
        t = np.full(nlay + 1, 250.0)
        for kind, thr, want_status in (("latch_harmless", 0.0, 0), ("latch_offending", K.FLAG_THR, 1),
                                       ("latch_harmless", K.FLAG_THR, 0)):
            od = K.flag_od(nlay, kind)
            n = od.shape[1]
            for ssi in (None, np.ones(n)):
                key, col, status = oracle.reorder_key(p, t, np.linspace(100, 2000, n), np.ones(n), od, ssi, thr)
                assert status == want_status, (nlay, kind, thr)
            if thr == 0.0:
                assert np.all(key == 0.0)                                         # shortwave: the crossing in the empty top layer
            if kind == "latch_offending":
                assert key[K.FLAG_INDEX] == ph[1]


def test_shortwave_and_merge_inputs():
    for c in K.SW_GEOMETRY:
        od = K.sw_od(c)
        assert od.dtype == np.dtype(c.dtype) and od.shape == (c.nlay, c.nwav)
        assert (od == np.asarray(1e30, dtype=c.dtype)).any()
        if c.dtype == "float32" and c.nlay * c.nwav > 1:
            tiny = od[(od > 0) & (od < np.finfo(np.float32).tiny)]
            assert tiny.size > 0                                                  # a float32 subnormal is among the data
    assert sum(c.strided for c in K.SW_GEOMETRY) == 1
    for nlay, nwav in K.MERGE_SHAPES:
        gases = K.merge_gases(nlay, nwav)
        assert [od.dtype for od, _ in gases] == [np.float32, np.float64]
        want = K.merge_expected(gases)
        assert np.isnan(want[nlay - 1, nwav // 2])                                # 0 x inf
        assert np.isinf(want[0, 0]) or (nlay == 1 and nwav == 1)
    wn = np.array([1.0, 2.0, 4.0])
    assert np.array_equal(K.derive_d_wavenumber(wn), [0.75, 1.5, 0.75])
