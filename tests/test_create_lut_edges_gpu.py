"""The segmented reductions of csrc/create_lut.hip (K6/K7) pinned at their chunk, lane-stride and method edges, against the
extended-precision reference of create_lut_cases.py (validated on the CPU by test_create_lut_cases.py).

What each case pins (kernels and statements of create_lut.hip):

  STRIDE (64, 64, 65 and 66 chunks: 131 071, 131 072, 131 073 and 133 121 points; 3 layers)
      the second trip of `for (c = c0 + lane; c < c1; c += 64)` of combine_chunks: in k_gavg_final (test_average), and in
      k_combine_chunks with [nrows][ng] output (test_planck_lut, test_erythemal, test_sum_rows_over_more_than_64_chunks) and
      with the last column of width[ng][nint + 1] as output (test_fractions_exact)
  EDGE with 43 and 54 layers against 42
      the second trip of `for (t = tid; t < nlay * 6; t += GA_THREADS)` at the end of k_gavg_partial (test_average)
  EDGE (g points of 0, 1, 2047, 2048, 2049, 4096, 4097 and 0 points)
      `ii[p] = live[p] ? i : c.p1` of chunk_positions and the `live[p]` skip of k_gavg_partial, k_planck_lut_partial,
      k_erythemal_partial and k_width_chunk_sums at a chunk of one point, one short of full, full, and full plus a chunk of
      one (test_average, test_planck_lut, test_erythemal, test_fractions_exact); `c1 > c0` of k_gavg_final at the empty g
      points
  width intervals of 0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513 and 1100 points with bounds ON wavenumbers
      `for (; i + 192 < hi; i += 256)` of k_gpoint_width, its hand-over to `for (; i < hi; i += 64)`, and both ends of
      (w1, w2] in its two binary searches (test_fractions_exact)
  designed optical depths (EDGE, test_average with "designed" / "designed-fltmax", test_hybrid_switches_at_100_hpa)
      k_gavg_final: `exp(num / den_nz) * (cnt / ntot)`; `cnt == 0.0`; `fmin(0.9999999999999999, num / den)`;
      `mn > 0.0 && mn >= mx`; host code of ecckd_average_to_gpoints: `pfl > 100.0e2 ? M_LOG : M_TRANS3`
  test_results_do_not_depend_on_other_g_points
      a read across c.p1 or before c.p0 in any partial kernel, a chunk partial of another g point in a final kernel
  test_regrowth_and_reproducibility
      gmap_work(): release and regrow under a sequence of calls of growing need
  NONE_ONLY
      `nchunk > 0` of ecckd_average_to_gpoints and `!m->chunks.empty()` of reduce_rows: no partial kernel is launched, the
      combining kernels read nothing

Bounds.  min and max are copies of inputs: equal to the reference where reference_surface_vmr <= 0.  The fit is within
64 eps max(1, condition) of the reference (condition: of the fit with respect to a relative error of its sums): all terms of
den, and of num outside the logarithmic method, are non-negative; each term carries under 10 roundings; the fixed tree is
under 30 additions deep; so a sum is within about 40 eps, and 64 leaves room for the final log / exp.  For the four
transmission methods the bound has a second term, eps condition / v with v = num / den, which comes from the
arithmetic and not from a measurement: a term 1 - exp(-x) is formed in double from an exp that is below 1 and carries an absolute error of up to eps / 2,
whatever x is - for a thin layer (x = 1e-9 in the uppermost layers here) that is a RELATIVE error of eps / (2 x) of the term
and so of the sum, which no condition number of the fit accounts for.  The double-precision oracle forms its terms in the
same way and shows the same error (test_create_lut_cases.py).  Where v is not small the second term is nothing beside the
first.  The Planck look-up table and the erythemal weights (all terms positive) are within 64 eps.

Measured on an MI355X, the largest error / (eps max(1, condition)) over all cases of this file - for the transmission methods
over the cells with v >= 0.01 (second term at most 100 eps condition) - and, in brackets, the largest error / bound over ALL
cells:
  average  linear                              4.43  (0.069)      average  transmission                     22.87  (0.252)
  average  square-root                         3.66  (0.057)      average  transmission-2                   24.47  (0.408)
  average  logarithmic                         1.93  (0.030)      average  transmission-3                   25.31  (0.270)
  average  hybrid-logarithmic-transmission-3  25.31  (0.270)      average  transmission-10                  21.69  (0.301)
  planck_lut  EDGE  5.26    STRIDE  15.34  (of 64)                erythemal  EDGE  1.42    STRIDE  1.62  (of 64)
Every test prints its figures (pytest -s); MEASURED keeps the largest of a session.
"""
import functools

import numpy as np
import pytest
import torch

import create_lut_cases as K

pytestmark = pytest.mark.gpu

VMR = 4.0e-4
POISON = 1.0e30            # what lies past a row of optical depths (row stride > nwav): must not be read
PAD = 37

MEASURED = {}              # (operation, method) -> largest error / (eps max(1, condition)) seen in this session


def _note(op, method, value, bound_ratio=None):
    key = (op, method)
    old = MEASURED.get(key, (0.0, 0.0))
    MEASURED[key] = (max(old[0], float(value)), max(old[1], float(bound_ratio or 0.0)))
    print("measured %-12s %-34s error / (eps max(1, cond)) %8.2f   error / bound %6.3f   (so far %8.2f, %6.3f)" %
          ((op, method, value, bound_ratio or 0.0) + MEASURED[key]))


def _dev(ctx, a):
    return torch.as_tensor(np.array(a, order="C"), device=ctx.device)      # (a packed copy: the cached inputs are read-only)


def _gmap(ctx, g, ng, wn, dwn):
    from ecckd_amd import api
    return api.GPointMap(ctx, _dev(ctx, g), ng, _dev(ctx, wn), _dev(ctx, dwn))


def _layout_map(ctx, name):
    g = K.layout_g(name)
    wn, dwn = K.grid(g.size)
    return _gmap(ctx, g, K.layout_ng(name), wn, dwn)


def _wide(ctx, od):
    """the optical depths in rows that are PAD longer than the spectrum, POISON behind every row -> the view of the rows"""
    nlay, nwav = od.shape
    wide = torch.full((nlay, nwav + PAD), POISON, dtype=getattr(torch, str(od.dtype)), device=ctx.device)
    wide[:, :nwav] = _dev(ctx, od)
    return wide[:, :nwav]


@functools.lru_cache(maxsize=2)
def _lw_weights(name, nlay):
    wn, dwn = K.grid(K.layout_g(name).size)
    return K.planck_terms(K.temperature_fl(K.pressure_grid(nlay)), wn, dwn)


def _weight_args(ctx, kind, name, nlay):
    """(keyword arguments of average_optical_depth, the reference's weights)"""
    nwav = K.layout_g(name).size
    if kind == "lw":
        return dict(temperature_fl=K.temperature_fl(K.pressure_grid(nlay))), _lw_weights(name, nlay)
    ssi = K.ssi_weights(nwav)
    return dict(ssi=_dev(ctx, ssi)), ssi.astype(K.X)


@functools.lru_cache(maxsize=None)
def _reference(name, nlay, variant, dtype, weights, method):
    g = K.layout_g(name)
    w = _lw_weights(name, nlay) if weights == "lw" else K.ssi_weights(g.size).astype(K.X)
    return K.average_reference(g, K.layout_ng(name), K.pressure_grid(nlay), K.optical_depth(name, nlay, variant, dtype),
                               method, w)


# (layout, layers, optical depths, precisions).  42 layers: one trip of the LDS combine of k_gavg_partial (252 values for 256
# threads); 43 and 54: two.  The largest finite FLOAT once.
AVERAGE_CASES = [("EDGE", 42, "smooth", ("float32", "float64")),
                 ("EDGE", 43, "smooth", ("float32", "float64")),
                 ("EDGE", 54, "smooth", ("float32", "float64")),
                 ("EDGE", 54, "designed", ("float32", "float64")),
                 ("EDGE", 54, "designed-fltmax", ("float32",)),
                 ("STRIDE", 3, "smooth", ("float32", "float64"))]
AVERAGE_PARAMS = [(name, nlay, variant, dtype, weights) for name, nlay, variant, dtypes in AVERAGE_CASES for dtype in dtypes
                  for weights in ("lw", "ssi")]


@pytest.mark.parametrize("method", K.METHODS)
@pytest.mark.parametrize("name,nlay,variant,dtype,weights", AVERAGE_PARAMS, ids=lambda v: str(v))
def test_average(ctx, name, nlay, variant, dtype, weights, method):
    """Every cell of fit, min and max, as plain optical depth and as molar absorption, with rows of optical depths that are
    longer than the spectrum and with packed rows; on the designed optical depths also what each designed g point must give."""
    g, ng = K.layout_g(name), K.layout_ng(name)
    p = K.pressure_grid(nlay)
    od = K.optical_depth(name, nlay, variant, dtype)
    ref = _reference(name, nlay, variant, dtype, weights, method)
    gm = _layout_map(ctx, name)
    assert gm.counts().tolist() == K.LAYOUTS[name][0]
    kw, _ = _weight_args(ctx, weights, name, nlay)
    d_od = _wide(ctx, od)
    assert d_od.stride(0) == g.size + PAD
    fit, mn, mx = gm.average_optical_depth(p, d_od, method, -1.0, **kw)
    packed = gm.average_optical_depth(p, d_od.contiguous(), method, -1.0, **kw)
    sfit, smn, smx = gm.average_optical_depth(p, d_od, method, VMR, **kw)
    gm.close()
    for a, b in zip((fit, mn, mx), packed):
        assert np.array_equal(a, b)
    assert fit.shape == (nlay, ng) and np.all(np.isfinite(fit))
    err, bound = K.relative_error(fit, ref.fit), K.fit_bound(ref)
    thick = ref.cancel <= 100.0
    _note("average", method, np.max(np.where(thick, err / (K.EPS * ref.cond), 0.0)), np.max(err / bound))
    assert np.array_equal(mn, ref.mn) and np.array_equal(mx, ref.mx)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, "%d cells, first (layer, g) %s: %r instead of %r" % (len(bad), bad[0].tolist(), fit[tuple(bad[0])],
                                                                              ref.fit[tuple(bad[0])])
    # as molar absorption: (g 0.001 M / vmr) x / dp, three more roundings
    scale = K.molar_scale(p, VMR)[:, None]
    assert np.all(K.relative_error(sfit, ref.fit * scale) <= bound + 4 * K.EPS)
    assert np.all(K.relative_error(smn, ref.mn.astype(K.X) * scale) <= 4 * K.EPS)
    assert np.all(K.relative_error(smx, ref.mx.astype(K.X) * scale) <= 4 * K.EPS)
    if variant != "smooth":
        K.assert_branches(method, p, od, g, fit, mn, mx)


@pytest.mark.parametrize("name,nlay,variant", [("EDGE", 54, "designed"), ("EDGE", 43, "smooth"), ("STRIDE", 3, "smooth")])
def test_hybrid_switches_at_100_hpa(ctx, name, nlay, variant):
    """hybrid-logarithmic-transmission-3: the layer whose full-level pressure is exactly 10000 Pa has the bits it has under
    transmission-3 (`>` 100 hPa selects logarithmic), like every layer above it; the layer below it and all further down have
    the bits of logarithmic."""
    p = K.pressure_grid(nlay)
    at = K.layer_at_100hpa(p)
    d_od = _dev(ctx, K.optical_depth(name, nlay, variant, "float32"))
    gm = _layout_map(ctx, name)
    kw, _ = _weight_args(ctx, "lw", name, nlay)
    hyb, t3, log = (gm.average_optical_depth(p, d_od, m, VMR, **kw)
                    for m in ("hybrid-logarithmic-transmission-3", "transmission-3", "logarithmic"))
    gm.close()
    differ = 0
    for h, a, b in zip(hyb, t3, log):
        assert np.array_equal(h[:at + 1], a[:at + 1]) and np.array_equal(h[at + 1:], b[at + 1:])
        differ += int(not np.array_equal(a[at], b[at])) + int(not np.array_equal(a[at + 1], b[at + 1]))
    assert differ >= 2                  # (the two methods do differ in these layers: the comparison can tell them apart)


LUT_ROWS_STRIDE = [0, 1, 2, 3, 115, 228, 229, 230]


@pytest.mark.parametrize("nlut", [1, 4, 231])
@pytest.mark.parametrize("name", ["EDGE", "STRIDE"])
def test_planck_lut(ctx, name, nlut):
    """120 .. 350 K in steps of 1 K: 231 rows, 57 blocks of four waves and one of three; 4 rows: one full block; 1 row: three
    waves leave at once.  EDGE: every cell.  STRIDE with 231 rows: the rows LUT_ROWS_STRIDE of every g point (a row's index
    enters the addressing alone, which EDGE checks at every row; the reference of all 231 x 530 000 terms would take minutes)."""
    g, ng = K.layout_g(name), K.layout_ng(name)
    wn, dwn = K.grid(g.size)
    t = np.arange(120.0, 351.0)[:nlut] if nlut > 1 else np.array([287.5])
    gm = _layout_map(ctx, name)
    lut = gm.planck_lut(t)
    gm.close()
    assert lut.shape == (nlut, ng)
    rows = LUT_ROWS_STRIDE if (name == "STRIDE" and nlut == 231) else list(range(nlut))
    ref = K.planck_lut_reference(g, ng, t[rows], wn, dwn)
    err = K.relative_error(lut[rows], ref)
    _note("planck_lut", name, err.max() / K.EPS)
    assert np.all(err <= 64 * K.EPS), np.argwhere(err > 64 * K.EPS)[:5].tolist()
    empty = np.array(K.LAYOUTS[name][0]) == 0
    assert not lut[:, empty].any() and np.all(lut[:, ~empty] > 0) and np.all(np.isfinite(lut))


@pytest.mark.parametrize("name", ["EDGE", "STRIDE"])
def test_erythemal(ctx, name):
    g, ng = K.layout_g(name), K.layout_ng(name)
    wn, dwn = K.erythemal_grid(g.size)
    gm = _gmap(ctx, g, ng, wn, dwn)
    got = gm.erythemal_spectrum()
    gm.close()
    ref = K.erythemal_reference(g, ng, wn, dwn)
    empty = np.array(K.LAYOUTS[name][0]) == 0
    assert np.all(np.isnan(got[empty])) and np.all(np.isnan(ref[empty].astype(np.float64)))       # 0 / 0
    err = K.relative_error(got[~empty], ref[~empty])
    _note("erythemal", name, err.max() / K.EPS)
    assert np.all(err <= 64 * K.EPS), (got, ref)


def test_sum_rows_over_more_than_64_chunks(ctx):
    """ecckd_gmap_sum_rows goes through k_combine_chunks like the Planck table: integer rows below 2^24 over STRIDE, against integer sums"""
    g, ng = K.layout_g("STRIDE"), K.layout_ng("STRIDE")
    rows = np.random.default_rng(9).integers(0, 2 ** 24, size=(3, g.size))
    have = g >= 0
    want = np.stack([np.bincount(g[have], weights=r[have].astype(np.float64), minlength=ng) for r in rows])
    assert want.max() < 2.0 ** 53
    gm = _layout_map(ctx, "STRIDE")
    for dtype in ("float32", "float64"):
        assert np.array_equal(gm.sum_rows(_dev(ctx, rows.astype(dtype))), want)
    gm.close()


@pytest.mark.parametrize("name,ig", [("EDGE", K.G_SMOOTH), ("STRIDE", 0)])
def test_fractions_exact(ctx, name, ig):
    """Integer widths: every width and every total is an exact sum in any order, the fraction is the correctly rounded quotient
    - bit for bit; an empty g point has 0 / 0.  The last interval holds everything: its fraction is exactly 1, so the sum that
    k_gpoint_width forms of a whole segment is the sum that k_width_chunk_sums and k_combine_chunks form of it."""
    g, ng = K.layout_g(name), K.layout_ng(name)
    wn, dwn = K.grid(g.size)
    w1, w2, _ = K.width_intervals(g, wn, ig)
    gm = _layout_map(ctx, name)
    got = gm.gpoint_fraction(w1, w2)
    gm.close()
    want = K.fraction_reference(g, ng, wn, dwn, w1, w2)[0]
    assert got.shape == want.shape
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, "(g, interval) %s: %r instead of %r" % (bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    empty = np.array(K.LAYOUTS[name][0]) == 0
    assert np.all(np.isnan(got[empty])) and np.all(got[~empty, -1] == 1.0)


def test_none_only(ctx):
    """no point has a g point: no chunk; averages and table are zeros, fractions and erythemal weights 0 / 0; nothing raises"""
    g, ng = K.layout_g("NONE_ONLY"), K.layout_ng("NONE_ONLY")
    wn, dwn = K.grid(g.size)
    gm = _layout_map(ctx, "NONE_ONLY")
    assert gm.counts().tolist() == [0, 0, 0]
    p = K.pressure_grid(54)
    d_od = _dev(ctx, K.optical_depth("NONE_ONLY", 54, "smooth", "float32"))
    for method in K.METHODS:
        for vmr in (-1.0, VMR):
            for out in gm.average_optical_depth(p, d_od, method, vmr, temperature_fl=K.temperature_fl(p)):
                assert out.shape == (54, ng) and not out.any()
    for out in gm.average_optical_depth(p, d_od, "linear", -1.0, ssi=_dev(ctx, K.ssi_weights(g.size))):
        assert not out.any()
    lut = gm.planck_lut(np.arange(120.0, 351.0))
    assert lut.shape == (231, ng) and not lut.any()
    assert np.all(np.isnan(gm.gpoint_fraction(np.array([599.0, 601.0]), np.array([601.0, 700.0]))))
    assert np.all(np.isnan(gm.erythemal_spectrum()))
    gm.close()


def test_results_do_not_depend_on_other_g_points(ctx):
    """A second map holds ONE g point of EDGE - the same points in the same order - and a third of the other points, without a
    g point: other natural positions, another place in the sorted order.  Its averages, table rows and fractions have the bits
    they have in the full map: a segment's result is a function of its own points and chunking alone."""
    g, ng = K.layout_g("EDGE"), K.layout_ng("EDGE")
    wn, dwn = K.grid(g.size)
    p = K.pressure_grid(54)
    t_fl = K.temperature_fl(p)
    od = K.optical_depth("EDGE", 54, "designed", "float32")
    t_lut = np.arange(120.0, 351.0, 10.0)
    w1, w2, _ = K.width_intervals(g, wn, K.G_SMOOTH)
    methods = ("linear", "transmission-3", "logarithmic", "square-root")

    def results(gm, d_od):
        out = [a for m in methods for a in gm.average_optical_depth(p, d_od, m, VMR, temperature_fl=t_fl)]
        return out, gm.planck_lut(t_lut), gm.gpoint_fraction(w1, w2)

    gm = _layout_map(ctx, "EDGE")
    full = results(gm, _dev(ctx, od))
    gm.close()
    for ig, n in enumerate(K.LAYOUTS["EDGE"][0]):
        if n == 0:
            continue
        pos, g2 = K.isolated(g, ig)
        gm = _gmap(ctx, g2, ng, wn[pos], dwn[pos])
        assert gm.counts()[ig] == n and gm.counts().sum() == n
        avg, lut, frac = results(gm, _dev(ctx, od[:, pos]))
        gm.close()
        for a, b in zip(avg, full[0]):
            assert np.array_equal(a[:, ig], b[:, ig]), ig
            assert not np.delete(a, ig, axis=1).any()
        assert np.array_equal(lut[:, ig], full[1][:, ig]) and np.array_equal(frac[ig], full[2][ig]), ig


def test_regrowth_and_reproducibility(ctx):
    """One map serves calls of growing need (K.REGROWTH_CALLS: its work buffer is regrown before the first average and
    before the average of 54 layers, and reused by the calls after it); every result has the bits of the same call on a
    fresh map."""
    g = K.layout_g("EDGE")
    wn, _ = K.grid(g.size)
    w1, w2, _ = K.width_intervals(g, wn, K.G_SMOOTH)
    assert len(w1) == K.REGROWTH_CALLS[0][1]
    ods = {n: _dev(ctx, K.optical_depth("EDGE", n, "designed" if n == 54 else "smooth", "float32")) for n in (3, 54)}

    def call(gm, what, n):
        if what == "gpoint_fraction":
            return [gm.gpoint_fraction(w1, w2)]
        if what == "planck_lut":
            return [gm.planck_lut(np.arange(120.0, 351.0)[:n] if n > 1 else np.array([287.5]))]
        p = K.pressure_grid(n)
        return list(gm.average_optical_depth(p, ods[n], "hybrid-logarithmic-transmission-3", VMR,
                                             temperature_fl=K.temperature_fl(p)))

    one = _layout_map(ctx, "EDGE")
    for what, n in K.REGROWTH_CALLS:
        got = call(one, what, n)
        fresh_map = _layout_map(ctx, "EDGE")
        want = call(fresh_map, what, n)
        fresh_map.close()
        for a, b in zip(got, want):
            assert np.array_equal(a, b, equal_nan=True), (what, n)
        assert all(np.any(np.isfinite(a) & (a != 0)) for a in got)
    one.close()
