"""GPU tests of the zenith-angle quadrature in the fused line-by-line longwave fluxes per g point
(ecckd_lbl_gpoint_fluxes_lw_angles) and in the spectral-output mode of the same kernel (ecckd_lbl_spectral_fluxes_lw_angles):
nangle = N > 0 integrates N Gauss-Legendre angles per hemisphere, flux = sum_k 2 w_k mu_k L(mu_k), every L(mu_k) the
reference's no-scattering recurrence along the slant path tau / mu_k; nangle = 0 is the two-stream path as it was.

Checked against the angles evaluated one by one with numpy, against the band kernel (ecckd_lbl_band_fluxes_lw_angles),
against the two-stream entry points bit for bit at nangle = 0, against the composed path, for invariance and for the
physics of the quadrature.  The g-point maps are those of test_lbl_gpoint_fluxes_gpu.py: random, 7 % of the wavenumbers
without a g point, a run of -1 at the start and - where there are more than EMPTY_G g points - one g point without
wavenumbers."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from conftest import make_lw_case

pytestmark = pytest.mark.gpu

# (nlay, nwav, ng, dtype of the optical depths): the tile edge (256 wavenumbers per tile); one column; the headline depth;
# 200 g points in several launches - 128 columns per launch at 20 layers, 48 at 54
TILE_CASES = [(3, 255, 2, "float64"), (3, 256, 2, "float64"), (3, 257, 2, "float64")]
MAIN_CASES = [(20, 20011, 1, "float64"), (54, 20011, 16, "float32"), (20, 19999, 200, "float32"), (54, 20011, 200, "float32")]
CASES = TILE_CASES + MAIN_CASES
EMPTY_G = 3          # the g point without wavenumbers (ng > 3)
PARAMETER_ERROR = 147


@functools.lru_cache(maxsize=None)
def _case(nlay, nwav, ng, dtype):
    from ecckd_amd import synthetic as syn
    p, wn, dwn, od = make_lw_case(nwav, nlay=nlay, seed=11, dtype=dtype, nlines=48)
    t_hl = syn.temperature_profile(p)
    rng = np.random.default_rng(1234 + ng + nlay)
    g = rng.integers(0, ng, size=nwav).astype(np.int32)
    if ng > 1:
        g[g == EMPTY_G] = (EMPTY_G + 1) % ng
    g[rng.random(nwav) < 0.07] = -1
    g[:3] = -1                                       # (a run of unassigned points at the start of a tile)
    return p, wn, dwn, od, t_hl, g


_libm_exp = np.frompyfunc(math.exp, 1, 1)


def _numpy_angle(planck, od, sec):
    """The recurrence of radiative_transfer_lw.cpp:27-60 along sec * tau, as test_lbl_band_fluxes_lw_angle_quadrature states it,
    with the exponential of the C library (math.exp), which the oracle's radiative_transfer_lw calls too, in place of np.exp.
    numpy's vectorised exp differs from it in the last bit for one argument in ten, and 1 - eps / (sec tau) next to the 1e-5
    switch turns that bit into 2e-6 of fac: over the ~100 wavenumbers of one of 200 g points the two exponentials move THIS
    restatement by up to 9.3e-8 (20 layers, nangle = 1; 4.8e-8 at 54 layers) where the sums of 3 000 wavenumbers of that test
    stay within 1e-8.  At those elements the library differs from the np.exp form by the same 9.283447e-8 and 4.805007e-8, digit
    for digit: it agrees with the C library's form to 1e-14 there."""
    nlay, nwav = od.shape
    eps = 1.0 - _libm_exp(-sec * od).astype(np.float64)
    fac = np.where(eps > 1.0e-5, 1.0 - (eps * (1.0 / sec)) / np.where(od > 0, od, 1.0), 0.5 * eps)
    dn = np.zeros((nlay + 1, nwav)); up = np.zeros((nlay + 1, nwav))
    for l in range(nlay):
        dn[l + 1] = dn[l] * (1 - eps[l]) + planck[l] * (eps[l] - fac[l]) + planck[l + 1] * fac[l]
    up[nlay] = planck[nlay]
    for l in range(nlay - 1, -1, -1):
        up[l] = up[l + 1] * (1 - eps[l]) + planck[l + 1] * (eps[l] - fac[l]) + planck[l] * fac[l]
    return dn, up


@functools.lru_cache(maxsize=None)
def _restated(case, nangle):
    """flux = sum_k 2 w_k mu_k L(mu_k), angle by angle in float64 -> per g point and over all wavenumbers"""
    import pyoracle
    from ecckd_amd import api
    pyoracle.build()
    p, wn, dwn, od, t_hl, g = _case(*case)
    ng = case[2]
    planck = pyoracle.planck_function(t_hl, wn, dwn)
    od64 = od.astype(np.float64)
    mu, w = api.gauss_legendre_01(nangle)
    dn = np.zeros((od.shape[0] + 1, wn.size)); up = np.zeros_like(dn)
    for m, w_ in zip(mu, w):
        d, u = _numpy_angle(planck, od64, 1.0 / m)
        dn += 2 * w_ * m * d; up += 2 * w_ * m * u
    return _sum_per_g(dn, g, ng), _sum_per_g(up, g, ng), dn.sum(1), up.sum(1)


def _sum_per_g(f, g, ng):
    order = np.argsort(g, kind="stable")
    fs = np.ascontiguousarray(f[:, order])
    edge = np.searchsorted(g[order], np.arange(ng + 1))
    out = np.zeros((f.shape[0], ng))
    for ig in range(ng):
        out[:, ig] = fs[:, edge[ig]:edge[ig + 1]].sum(1, dtype=np.float64)
    return out


def _dev(ctx, a):
    return torch.as_tensor(a, device=ctx.device)


def _gmap(ctx, g, ng, wn, dwn):
    from ecckd_amd import api
    return api.GPointMap(ctx, _dev(ctx, g), ng, _dev(ctx, wn), _dev(ctx, dwn))


def _rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


@pytest.mark.parametrize("nangle", [1, 2, 4, 16])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_against_the_angles_one_by_one(ctx, case, nangle):
    """1. h_flux_* and h_bb_* against the numpy restatement of the quadrature summed per g point in float64.  rtol 1e-8 is what
    test_lbl_band_fluxes_lw_angle_quadrature uses for the same arithmetic: 1 - eps / (sec tau) next to the 1e-5 switch amplifies
    the last bit of exp by 1e5."""
    nlay, nwav, ng, dtype = case
    p, wn, dwn, od, t_hl, g = _case(*case)
    gm = _gmap(ctx, g, ng, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_hl, _dev(ctx, od), nangle=nangle)
    gm.close()
    wdn, wup, wbdn, wbup = _restated(case, nangle)
    for name, a, b in (("dn", dn, wdn), ("up", up, wup), ("bb_dn", bdn, wbdn), ("bb_up", bup, wbup)):
        print(name, "max rel diff", _rel(a, b))
    assert np.allclose(dn, wdn, rtol=1e-8, atol=1e-300)
    assert np.allclose(up, wup, rtol=1e-8, atol=1e-300)
    assert np.allclose(bdn, wbdn, rtol=1e-8, atol=1e-300)
    assert np.allclose(bup, wbup, rtol=1e-8, atol=1e-300)
    assert np.all(dn[0] == 0.0) and bdn[0] == 0.0                 # nothing comes down at the top of the atmosphere
    if ng > EMPTY_G:
        assert np.all(dn[:, EMPTY_G] == 0.0) and np.all(up[:, EMPTY_G] == 0.0)      # an empty g point: exactly 0


@pytest.mark.parametrize("nangle", [1, 4])
@pytest.mark.parametrize("nlay,nwav,nband,dtype", [(54, 20011, 13, "float32"), (20, 20011, 5, "float64")])
def test_band_kernel_consistency(ctx, nlay, nwav, nband, dtype, nangle):
    """2. g_point = band index over contiguous bands: the intensities are those of ecckd_lbl_band_fluxes_lw_angles, all terms
    >= 0, so the results differ by at most (the longest addition chain of the one + that of the other) x 2^-53 relative.  The
    chains are those of test_lbl_gpoint_fluxes_gpu.py::test_band_kernel_consistency with + N on each side: the fused path adds
    the N angle terms of a point before it bins the flux, the band kernel passes each addend through the N accumulations of
    its level (one per angle)."""
    from ecckd_amd import api
    p, wn, dwn, od, t_hl, _ = _case(nlay, nwav, 16, dtype)
    edges = np.linspace(0, nwav, nband + 1).astype(np.int64)
    begin, end = edges[:-1], edges[1:] - 1
    g = np.repeat(np.arange(nband, dtype=np.int32), np.diff(edges))
    d_od = _dev(ctx, od)
    gm = _gmap(ctx, g, nband, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_hl, d_od, nangle=nangle)
    gm.close()
    bdn_k, bup_k = api.lbl_band_fluxes_lw(ctx, t_hl, _dev(ctx, wn), _dev(ctx, dwn), d_od, begin, end, nangle=nangle)
    ntiles = -(-nwav // 256)
    tiles_per_block = max(1, -(-ntiles // 2048))
    nblocks = -(-ntiles // tiles_per_block)
    chain_fused = 8 + 32 * tiles_per_block + nblocks + nangle
    chain_band = 6 + 1 + 3 + int(np.max(-(-(end - begin + 1) // 256))) + nangle
    bound = (chain_fused + chain_band) * 2.0 ** -53
    print("chains", chain_fused, chain_band, "bound", bound)
    assert bound < 1e-12
    for name, a, b in (("dn", dn, bdn_k.T), ("up", up, bup_k.T)):
        print(name, "max rel diff", _rel(a, b))
        assert np.allclose(a, b, rtol=bound, atol=0.0)


@pytest.mark.parametrize("case", [TILE_CASES[2], MAIN_CASES[1], MAIN_CASES[3]], ids=str)
def test_nangle_zero_is_the_two_stream_path(ctx, case):
    """3. nangle = 0 through the new entry points against the calls without the argument, and against the two-stream C entry
    points themselves: g-point sums, broadband sums and FLOAT rows, bit for bit."""
    from ecckd_amd import _lib, api
    nlay, nwav, ng, dtype = case
    p, wn, dwn, od, t_hl, g = _case(*case)
    d_od, d_wn, d_dwn = _dev(ctx, od), _dev(ctx, wn), _dev(ctx, dwn)
    gm = _gmap(ctx, g, ng, wn, dwn)
    a = gm.lbl_fluxes_lw(t_hl, d_od)
    b = gm.lbl_fluxes_lw(t_hl, d_od, nangle=0)
    # the two-stream C entry point, which the wrapper no longer calls
    t = np.ascontiguousarray(t_hl, dtype=np.float64)
    c = [np.empty((nlay + 1, ng)), np.empty((nlay + 1, ng)), np.empty(nlay + 1), np.empty(nlay + 1)]
    hp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    od_type = _lib.F32 if dtype == "float32" else _lib.F64
    ctx.fence_from_torch()
    _lib.check(ctx.lib.ecckd_lbl_gpoint_fluxes_lw(gm.handle, nlay, hp(t), C.c_void_p(d_od.data_ptr()), od_type, d_od.stride(0),
                                                  hp(c[0]), hp(c[1]), hp(c[2]), hp(c[3])))
    gm.close()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert not np.array_equal(a[1], _gfl(ctx, case, 4)[1])          # (and the quadrature is another result)
    s0 = api.lbl_spectral_fluxes_lw(ctx, t_hl, d_wn, d_dwn, d_od)
    s1 = api.lbl_spectral_fluxes_lw(ctx, t_hl, d_wn, d_dwn, d_od, nangle=0)
    sdn = torch.empty((nlay + 1, nwav), dtype=torch.float32, device=ctx.device)
    sup = torch.empty_like(sdn)
    bdn, bup = np.empty(nlay + 1), np.empty(nlay + 1)
    ctx.fence_from_torch()
    _lib.check(ctx.lib.ecckd_lbl_spectral_fluxes_lw(ctx.handle, nlay, nwav, hp(t), C.c_void_p(d_wn.data_ptr()),
                                                    C.c_void_p(d_dwn.data_ptr()), C.c_void_p(d_od.data_ptr()), od_type, d_od.stride(0),
                                                    C.c_void_p(sdn.data_ptr()), C.c_void_p(sup.data_ptr()), nwav, hp(bdn), hp(bup)))
    ctx.synchronize()
    assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1]) and torch.equal(s0[0], sdn) and torch.equal(s0[1], sup)
    assert np.array_equal(s0[2], s1[2]) and np.array_equal(s0[3], s1[3]) and np.array_equal(s0[2], bdn) and np.array_equal(s0[3], bup)


def _gfl(ctx, case, nangle, od=None, g=None, ng=None):
    p, wn, dwn, od0, t_hl, g0 = _case(*case)
    gm = _gmap(ctx, g0 if g is None else g, case[2] if ng is None else ng, wn, dwn)
    out = gm.lbl_fluxes_lw(t_hl, _dev(ctx, od0 if od is None else od), nangle=nangle)
    gm.close()
    return out


@pytest.mark.parametrize("nangle", [1, 4])
@pytest.mark.parametrize("case", [TILE_CASES[2], MAIN_CASES[1], MAIN_CASES[2]], ids=str)
def test_spectral_mode(ctx, case, nangle):
    """4. The spectral-output mode.  Rows dn[nlay] and up[0] against the per-wavenumber doubles of the band kernel
    (boundary=True): a FLOAT rounding (2^-24 relative, 2^-150 absolute for a subnormal) of a double that agrees with the band
    kernel's to the bound of test 1 and better (1e-7 allows for it).  The FLOAT rows summed per g point by ecckd_gmap_sum_rows
    against the fused sums: rtol / atol of test_lbl_gpoint_fluxes_gpu.py::test_against_the_composed_path, whose argument does not
    depend on how the double flux of a point was formed."""
    from ecckd_amd import api
    nlay, nwav, ng, dtype = case
    p, wn, dwn, od, t_hl, g = _case(*case)
    d_od, d_wn, d_dwn = _dev(ctx, od), _dev(ctx, wn), _dev(ctx, dwn)
    sdn, sup, sbdn, sbup = api.lbl_spectral_fluxes_lw(ctx, t_hl, d_wn, d_dwn, d_od, nangle=nangle)
    assert sdn.dtype == torch.float32 and tuple(sdn.shape) == (nlay + 1, nwav)
    _, _, surf, toa = api.lbl_band_fluxes_lw(ctx, t_hl, d_wn, d_dwn, d_od, np.array([0]), np.array([nwav - 1]), boundary=True,
                                             nangle=nangle)
    rt, at = 2.0 ** -24 + 1e-7, 2.0 ** -150
    assert np.allclose(sdn[nlay].cpu().numpy().astype(np.float64), surf.cpu().numpy(), rtol=rt, atol=at)
    assert np.allclose(sup[0].cpu().numpy().astype(np.float64), toa.cpu().numpy(), rtol=rt, atol=at)
    assert np.all(sdn[0].cpu().numpy() == 0.0)
    gm = _gmap(ctx, g, ng, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_hl, d_od, nangle=nangle)
    cdn, cup = gm.sum_rows(sdn), gm.sum_rows(sup)
    gm.close()
    rtol, atol = 2.0 ** -23 * (0.5 + 1e-6), nwav * 2.0 ** -150
    for name, a, b in (("dn", cdn, dn), ("up", cup, up)):
        print(name, "max rel diff / 2^-23:", _rel(a, b) * 2.0 ** 23)
    assert np.allclose(cdn, dn, rtol=rtol, atol=atol)
    assert np.allclose(cup, up, rtol=rtol, atol=atol)
    assert np.allclose(sbdn, bdn, rtol=1e-12, atol=0.0) and np.allclose(sbup, bup, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("case", [MAIN_CASES[1], MAIN_CASES[2], MAIN_CASES[3]], ids=str)
def test_reproducible_and_float_double_agree(ctx, case):
    """5a. nangle = 4: two calls give the same bits; DOUBLE optical depths holding the upcast FLOAT values give the FLOAT bits."""
    from ecckd_amd import api
    p, wn, dwn, od, t_hl, g = _case(*case)
    assert od.dtype == np.float32
    a, b, c = _gfl(ctx, case, 4), _gfl(ctx, case, 4), _gfl(ctx, case, 4, od=od.astype(np.float64))
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    d_wn, d_dwn = _dev(ctx, wn), _dev(ctx, dwn)
    s1 = api.lbl_spectral_fluxes_lw(ctx, t_hl, d_wn, d_dwn, _dev(ctx, od), nangle=4)
    s2 = api.lbl_spectral_fluxes_lw(ctx, t_hl, d_wn, d_dwn, _dev(ctx, od.astype(np.float64)), nangle=4)
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])
    assert np.array_equal(s1[2], s2[2]) and np.array_equal(s1[3], s2[3])


@pytest.mark.parametrize("case", [MAIN_CASES[2], MAIN_CASES[3]], ids=str)
def test_a_launch_range_on_its_own(ctx, case):
    """5b. nangle = 4, 200 g points: the g points of the second launch range (columns per launch: 64 KB less the binner's 22 KB,
    over 16 (nlay + 1) bytes; the first launch also holds the column of the points without a g point) in a map that holds only
    them, every other wavenumber -1.  That map is swept with another split - at 20 layers in one launch instead of two, at 54
    layers in two (47 + 1 g points) instead of five - and a g point keeps its bits wherever it keeps its place among the
    columns of its launch: its ranks in every tile, and with them the pieces its sum is formed from, are then the same.  The
    last g point of the 54-layer range moves to a launch of its own, where its ranks start at 0: it agrees to the chain bound
    of test 2 (< 1e-12), not bit for bit."""
    nlay, nwav, ng, dtype = case
    p, wn, dwn, od, t_hl, g = _case(*case)
    cols = (65536 - (8 * 288 * 8 + 8 * 32 * 8 + 2 * 256 * 4)) // (16 * (nlay + 1))
    assert cols == {20: 128, 54: 48}[nlay]
    g0, g1 = cols - 1, min(ng, 2 * cols - 1)                       # the second launch bins [g0, g1)
    full = _gfl(ctx, case, 4)
    g_own = np.where((g >= g0) & (g < g1), g - g0, -1).astype(np.int32)
    own = _gfl(ctx, case, 4, g=g_own, ng=g1 - g0)
    same = min(g1 - g0, cols - 1)                                  # the g points of the new map's first launch
    assert same >= 47
    for k in (0, 1):
        assert np.array_equal(own[k][:, :same], full[k][:, g0:g0 + same])
        assert np.allclose(own[k][:, same:], full[k][:, g0 + same:g1], rtol=1e-12, atol=0.0)
    assert np.allclose(own[2], full[2], rtol=1e-12, atol=0.0) and np.allclose(own[3], full[3], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("nangle", [0, 3, 4, 16])
def test_isothermal_opaque_column(ctx, oracle, nangle):
    """6a. An isothermal (250 K), opaque (tau = 50) column radiates the Planck function whatever the angles, since
    sum_k 2 w_k mu_k = 1: every g point's up[0] and dn[nlay] are the Planck sums of its wavenumbers."""
    case = MAIN_CASES[1]
    nlay, nwav, ng, dtype = case
    p, wn, dwn, od, t_hl, g = _case(*case)
    t_iso = np.full(nlay + 1, 250.0)
    want = _sum_per_g(oracle.planck_function(t_iso, wn, dwn), g, ng)
    gm = _gmap(ctx, g, ng, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_iso, _dev(ctx, np.full((nlay, nwav), 50.0)), nangle=nangle)
    gm.close()
    print("max rel diff", _rel(up[0], want[0]), _rel(dn[nlay], want[nlay]))
    assert np.allclose(up[0], want[0], rtol=1e-12, atol=0.0) and np.allclose(dn[nlay], want[nlay], rtol=1e-12, atol=0.0)
    assert np.all(up[0, np.arange(ng) != EMPTY_G] > 0.0) and up[0, EMPTY_G] == 0.0


def test_quadrature_converges(ctx):
    """6b. The broadband upwelling profile converges as the angles are refined, and the two-stream value lies within 2 % of the
    converged one and not closer to it than 4 angles: the assertions of test_lbl_band_fluxes_lw_angle_quadrature."""
    case = MAIN_CASES[1]
    tot = {n: _gfl(ctx, case, n)[3] for n in (0, 1, 2, 4, 8, 16)}
    err = {n: np.max(np.abs(tot[n] - tot[16]) / tot[16]) for n in (0, 1, 2, 4, 8)}
    print("errors against 16 angles", err)
    assert err[1] > err[2] > err[4] > err[8]
    assert err[4] < err[0] < 0.02


def test_refusals(ctx):
    """7. nangle outside 0..16 is refused with PARAMETER_ERROR and `nangle` in the message, through ctypes and through the
    wrappers; 16 is accepted, and the context goes on working."""
    from ecckd_amd import _lib, api
    case = TILE_CASES[2]
    nlay, nwav, ng, dtype = case
    p, wn, dwn, od, t_hl, g = _case(*case)
    d_od, d_wn, d_dwn = _dev(ctx, od), _dev(ctx, wn), _dev(ctx, dwn)
    gm = _gmap(ctx, g, ng, wn, dwn)
    t = np.ascontiguousarray(t_hl, dtype=np.float64)
    hp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    out = [np.empty((nlay + 1, ng)), np.empty((nlay + 1, ng)), np.empty(nlay + 1), np.empty(nlay + 1)]
    sdn = torch.empty((nlay + 1, nwav), dtype=torch.float32, device=ctx.device)
    sup = torch.empty_like(sdn)
    ctx.fence_from_torch()
    for bad in (-1, 17):
        rc = ctx.lib.ecckd_lbl_gpoint_fluxes_lw_angles(gm.handle, bad, nlay, hp(t), C.c_void_p(d_od.data_ptr()), _lib.F64, d_od.stride(0),
                                                       hp(out[0]), hp(out[1]), hp(out[2]), hp(out[3]))
        assert rc == PARAMETER_ERROR and b"nangle" in ctx.lib.ecckd_last_error()
        rc = ctx.lib.ecckd_lbl_spectral_fluxes_lw_angles(ctx.handle, bad, nlay, nwav, hp(t), C.c_void_p(d_wn.data_ptr()),
                                                         C.c_void_p(d_dwn.data_ptr()), C.c_void_p(d_od.data_ptr()), _lib.F64,
                                                         d_od.stride(0), C.c_void_p(sdn.data_ptr()), C.c_void_p(sup.data_ptr()), nwav,
                                                         hp(out[2]), hp(out[3]))
        assert rc == PARAMETER_ERROR and b"nangle" in ctx.lib.ecckd_last_error()
        with pytest.raises(_lib.EcckdError, match="nangle") as e:
            gm.lbl_fluxes_lw(t_hl, d_od, nangle=bad)
        assert e.value.code == PARAMETER_ERROR
        with pytest.raises(_lib.EcckdError, match="nangle") as e:
            api.lbl_spectral_fluxes_lw(ctx, t_hl, d_wn, d_dwn, d_od, nangle=bad)
        assert e.value.code == PARAMETER_ERROR
    # 16 is accepted, and a valid call follows a refused one on the same context
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_hl, d_od, nangle=16)
    assert np.all(np.isfinite(up)) and np.all(bup > 0.0)
    s = api.lbl_spectral_fluxes_lw(ctx, t_hl, d_wn, d_dwn, d_od, nangle=16)
    assert np.allclose(s[3], bup, rtol=1e-12, atol=0.0)
    gm.close()
