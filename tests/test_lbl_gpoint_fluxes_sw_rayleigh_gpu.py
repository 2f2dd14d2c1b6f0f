"""ecckd_lbl_gpoint_fluxes_sw_rayleigh and ecckd_lbl_spectral_fluxes_sw_rayleigh (csrc/lbl_gpoint_fluxes_sw_rayleigh.hip): the
Rayleigh two-stream transfer of the band kernel met with the tile binner of gpoint_bin.hpp.

Against the two numpy references of tests/rayleigh_ref.py summed per g point in float64, exactly (`==`) on the layout inputs of
tests/gpoint_layouts.py with a Rayleigh optical depth of 0 - where the transfer is the no-scattering one and every flux a
small integer times a power of two - and against the existing kernels where they must agree.

Tolerances are absolute and scaled by the incoming flux, those of test_lbl_fluxes_sw_rayleigh_gpu.py: 1e-9 mu0 sum(ssi) of
the column (g point, or all wavenumbers) against the restatement two_stream_closed, rayleigh_ref.EXACT_BOUND against
two_stream_exact; for a FLOAT spectral row 1e-9 mu0 ssi + 2^-24 |value| (half an ulp of the cast)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gpoint_layouts as L
import rayleigh_ref as rr
from test_lbl_fluxes_sw_rayleigh_gpu import _angles, _case, _closed, _exact

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG = 7
HALF_ULP_F32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _gmap(nwav, ng=NG):
    """A random map over ng g points with some -1; g point 1 owns no wavenumber and g point ng - 2 owns exactly one."""
    rng = np.random.default_rng(7000 + nwav)
    pool = [g for g in range(ng) if g not in (1, ng - 2)]
    g = rng.choice(pool, size=nwav).astype(np.int32)
    g[rng.random(nwav) < 0.1] = -1
    g[int(rng.integers(0, nwav))] = ng - 2
    g.setflags(write=False)
    return g


def _dev(ctx, a, f32=False):
    import torch
    return torch.as_tensor(np.array(a, dtype=np.float32 if f32 else np.float64), device=ctx.device)   # (a copy: the cases are read-only)


def _make_map(ctx, g, ng):
    import torch
    from ecckd_amd import api
    nwav = g.size
    wn = np.linspace(2000.0, 20000.0, nwav) if nwav > 1 else np.array([2000.0])
    dwn = np.full(nwav, 18000.0 / max(nwav - 1, 1))
    return api.GPointMap(ctx, torch.as_tensor(np.array(g, dtype=np.int32), device=ctx.device), ng, _dev(ctx, wn), _dev(ctx, dwn))


def _run_g(ctx, nlay, nwav, nsza, with_albedo=True, f32=(False, False), angles=None):
    """the g-point entry on _case: (direct, dn, up) (nsza, nlay+1, NG), (bb_direct, bb_dn, bb_up) (nsza, nlay+1)"""
    ta, tr, ssi, albedo = _case(nlay, nwav)
    gm = _make_map(ctx, _gmap(nwav), NG)
    try:
        return gm.lbl_fluxes_sw_rayleigh(_angles(nsza) if angles is None else angles, _dev(ctx, ssi), _dev(ctx, ta, f32[0]),
                                         _dev(ctx, tr, f32[1]), _dev(ctx, albedo) if with_albedo else None)
    finally:
        gm.close()


def _run_s(ctx, nlay, nwav, nsza, with_albedo=True, f32=(False, False), angles=None):
    """the spectral entry on _case: three FLOAT arrays (nsza, nlay+1, nwav) and the three broadband arrays"""
    from ecckd_amd import api
    ta, tr, ssi, albedo = _case(nlay, nwav)
    out = api.lbl_spectral_fluxes_sw_rayleigh(ctx, _angles(nsza) if angles is None else angles, _dev(ctx, ssi), _dev(ctx, ta, f32[0]),
                                              _dev(ctx, tr, f32[1]), _dev(ctx, albedo) if with_albedo else None)
    return tuple(t.cpu().numpy() for t in out[:3]) + tuple(out[3:])


def _per_g(x, g, ng):
    """(nsza, nhl, nwav) -> (nsza, nhl, ng) in float64"""
    return np.stack([x[:, :, g == k].sum(-1) for k in range(ng)], axis=2)


def _check_g(ref, got, nlay, nwav, nsza, tol_rel, what):
    """(direct, diffuse, up) of a reference against the six arrays of the g-point entry"""
    _, _, ssi, _ = _case(nlay, nwav)
    g, mu = _gmap(nwav), _angles(nsza)
    d, dn, up = ref
    ssi_g = np.array([ssi[g == k].sum() for k in range(NG)])
    assert ssi_g[1] == 0.0 and np.sum(g == NG - 2) == 1
    for name, a, bb, b in (("direct", got[0], got[3], d), ("dn", got[1], got[4], d + dn), ("up", got[2], got[5], up)):
        err = np.max(np.abs(a - _per_g(b, g, NG)) / np.maximum(mu[:, None, None] * ssi_g, 1e-300) * (ssi_g > 0))
        err_bb = np.max(np.abs(bb - b.sum(-1)) / (mu[:, None] * ssi.sum()))
        print(f"{what} nlay={nlay} nwav={nwav} nsza={nsza} {name}: per g point {err:.3e}, broadband {err_bb:.3e} of the incoming flux "
              f"(allowed {tol_rel:.1e})")
        assert err <= tol_rel and err_bb <= tol_rel, (what, name, err, err_bb)
        assert np.all(a[:, :, 1] == 0.0)                             # the empty g point


def _check_s(ref, got, nlay, nwav, nsza, tol_rel, what):
    _, _, ssi, _ = _case(nlay, nwav)
    mu = _angles(nsza)
    d, dn, up = ref
    for name, a, bb, b in (("direct", got[0], got[3], d), ("dn", got[1], got[4], d + dn), ("up", got[2], got[5], up)):
        assert a.dtype == np.float32
        excess = np.abs(a.astype(np.float64) - b) - HALF_ULP_F32 * np.abs(b)
        err = np.max(excess / (mu[:, None, None] * ssi[None, None, :]))
        err_bb = np.max(np.abs(bb - b.sum(-1)) / (mu[:, None] * ssi.sum()))
        print(f"{what} nlay={nlay} nwav={nwav} nsza={nsza} spectral {name}: {err:.3e} beyond the FLOAT cast, broadband {err_bb:.3e} "
              f"(allowed {tol_rel:.1e})")
        assert err <= tol_rel and err_bb <= tol_rel, (what, name, err, err_bb)


SHAPES = [(1, 37, 1), (3, 256, 5), (8, 257, 8), (3, 600, 1), (54, 300, 5)]


@pytest.mark.parametrize("nlay,nwav,nsza", SHAPES)
def test_against_the_restatement(ctx, nlay, nwav, nsza):
    ref = _closed(nlay, nwav, nsza)
    _check_g(ref, _run_g(ctx, nlay, nwav, nsza), nlay, nwav, nsza, 1e-9, "closed")
    _check_s(ref, _run_s(ctx, nlay, nwav, nsza), nlay, nwav, nsza, 1e-9, "closed")


@pytest.mark.parametrize("nlay,nwav,nsza", [(1, 37, 1), (54, 300, 1)])
def test_against_the_exact_solve(ctx, nlay, nwav, nsza):
    ref = _exact(nlay, nwav, nsza)
    _check_g(ref, _run_g(ctx, nlay, nwav, nsza), nlay, nwav, nsza, rr.EXACT_BOUND, "exact")
    _check_s(ref, _run_s(ctx, nlay, nwav, nsza), nlay, nwav, nsza, rr.EXACT_BOUND, "exact")


# ------------------------------------------------------------------------------------- the binner's edges, exactly (tau_ray = 0)
def _exact_inputs(sp, nlay, nsza, with_albedo=True, dtype="float32"):
    """L.sw_inputs for a spectrum of this file's own: every flux is cos_sza x albedo x ssi or exactly 0"""
    rng = np.random.default_rng(1000003 * nlay + 1009 * sp.ng + 31 * nsza + sp.nwav)
    ssi = rng.integers(1, 2 ** 20, size=sp.nwav).astype(np.float64)
    albedo = (0.5 ** rng.integers(0, 3, size=sp.nwav)) if with_albedo else None
    cut = rng.integers(0, nlay + 1, size=sp.nwav)
    od = np.zeros((nlay, sp.nwav), dtype=dtype)
    at = np.nonzero(cut < nlay)[0]
    od[cut[at], at] = 1.0e6
    cos_sza = np.array([2.0 ** -e for e in L.COS_EXP[:nsza]])
    wn = np.linspace(2000.0, 20000.0, sp.nwav)
    return L.SwInputs(sp.g, sp.ng, sp.nwav, wn, np.full(sp.nwav, 18000.0 / (sp.nwav - 1)), cos_sza, ssi, albedo, od, cut)


def _exact_reference(inp, nlay):
    """L.sw_reference for such inputs: integer sums times powers of two, exact in double"""
    dn, up4 = L.sw_integer_sums(inp, nlay)
    mu = inp.cos_sza[:, None, None]
    fdn, fup = mu * dn.astype(np.float64), mu * (up4.astype(np.float64) * 0.25)
    return L.SwReference(fdn[:, :, :inp.ng], fup[:, :, :inp.ng], inp.cos_sza[:, None] * dn.sum(1).astype(np.float64),
                         inp.cos_sza[:, None] * (up4.sum(1).astype(np.float64) * 0.25))


def _check_exactly(ctx, inp, ref, spectral=None):
    """tau_ray = 0: direct == dn == the reference's dn and up == its up, per g point, broadband and (spectral given) per point"""
    from ecckd_amd import api
    gm = _make_map(ctx, inp.g, inp.ng)
    d_ssi, d_od = _dev(ctx, inp.ssi), _dev(ctx, inp.od, inp.od.dtype == np.float32)
    d_ray = _dev(ctx, np.zeros_like(inp.od), inp.od.dtype == np.float32)
    d_alb = _dev(ctx, inp.albedo) if inp.albedo is not None else None
    try:
        direct, dn, up, bdir, bdn, bup = gm.lbl_fluxes_sw_rayleigh(inp.cos_sza, d_ssi, d_od, d_ray, d_alb)
    finally:
        gm.close()
    assert np.array_equal(direct, ref.dn) and np.array_equal(dn, ref.dn) and np.array_equal(up, ref.up)
    assert np.array_equal(bdir, ref.bb_dn) and np.array_equal(bdn, ref.bb_dn) and np.array_equal(bup, ref.bb_up)
    if inp.albedo is None:
        assert np.all(up == 0.0) and np.all(bup == 0.0)              # a missing albedo is albedo 0
    if inp.ng >= 4:
        assert np.all(direct[:, :, 1] == 0.0)                        # the g point without a wavenumber
    if spectral is not None:
        sdir, sdn, sup, b0, b1, b2 = api.lbl_spectral_fluxes_sw_rayleigh(ctx, inp.cos_sza, d_ssi, d_od, d_ray, d_alb)
        want_dn, want_up = (x.astype(np.float32) for x in spectral)
        assert np.array_equal(sdir.cpu().numpy(), want_dn) and np.array_equal(sdn.cpu().numpy(), want_dn)
        assert np.array_equal(sup.cpu().numpy(), want_up)
        assert np.array_equal(b0, ref.bb_dn) and np.array_equal(b1, ref.bb_dn) and np.array_equal(b2, ref.bb_up)


EDGE_CASES = L.LAYOUT_CASES + L.ANGLE_CASES + L.TINY_CASES + [L.BIG_CASE]


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c.name for c in EDGE_CASES])
def test_binner_edges_exactly(ctx, case):
    """Rows 3 * level + flux in batches of 8 with a tail batch (12 rows at 3 layers, 15 at 4), last tiles of 1/7/8/9/255
    lanes, several tiles per block, and (BIG_CASE: 1367 logical blocks) physical blocks that loop over logical ones."""
    _check_exactly(ctx, L.sw_inputs(case), L.sw_reference(case), L.sw_spectral(case))


def rayleigh_cap(nlay):
    """columns per launch: the formula in the header of lbl_gpoint_fluxes_sw_rayleigh.hip"""
    return L.SF_ACC_BYTES // (24 * (nlay + 1))


def rayleigh_ranges(nlay, ng):
    return L.column_ranges(ng, min(rayleigh_cap(nlay), ng + 1))


RANGE_SPLITS = {43: [43], 44: [43, 1], 87: [43, 44], 88: [43, 44, 1]}


@pytest.mark.parametrize("ng", sorted(RANGE_SPLITS))
def test_launch_splits_at_54_layers_exactly(ctx, ng):
    nlay, nsza = 54, 2
    assert rayleigh_cap(nlay) == 44
    ranges = rayleigh_ranges(nlay, ng)
    assert [n for _, n, _ in ranges] == RANGE_SPLITS[ng] and [w for _, _, w in ranges] == [True] + [False] * (len(ranges) - 1)
    sp = L.spectrum(ng, ranges=tuple((g0, n) for g0, n, _ in ranges))   # some tiles lie wholly outside a launch's range
    inp = _exact_inputs(sp, nlay, nsza)
    _check_exactly(ctx, inp, _exact_reference(inp, nlay))


# ------------------------------------------------------------------------------------------------- against the existing kernels
def test_consistent_with_the_existing_kernels(ctx):
    from ecckd_amd import api
    nlay, nwav, nsza = 8, 600, 5
    ta, tr, ssi, albedo = _case(nlay, nwav)
    mu, g = _angles(nsza), _gmap(nwav)
    direct, dn, up, bdir, bdn, bup = _run_g(ctx, nlay, nwav, nsza)
    sdir = _run_s(ctx, nlay, nwav, nsza)[0]
    d_ssi, d_alb, d_tau = _dev(ctx, ssi), _dev(ctx, albedo), _dev(ctx, ta + tr)
    # the direct beam is the no-scattering chain on tau_abs + tau_ray formed in float64
    rdn = api.lbl_spectral_fluxes_sw(ctx, mu, d_ssi, d_tau, d_alb)[0].cpu().numpy()
    assert np.array_equal(sdir, rdn)
    gm = _make_map(ctx, g, NG)
    try:
        gdn = gm.lbl_fluxes_sw(mu, d_ssi, d_tau, d_alb)[0]
        np.testing.assert_allclose(direct, gdn, rtol=1e-13, atol=0.0)
        # the broadband rows against the band entry over one all-covering band (another order of summation)
        b = api.lbl_band_fluxes_sw_rayleigh(ctx, mu, d_ssi, _dev(ctx, ta), _dev(ctx, tr), [0], [nwav - 1], albedo=d_alb)
        for mine, theirs in zip((bdir, bdn, bup), b):
            np.testing.assert_allclose(mine, theirs[:, 0], rtol=1e-13, atol=0.0)
        # without scattering it is the no-scattering kernel
        ta3 = np.maximum(ta, 1e-3)                                   # (tau_abs = 0 too would leave nothing to attenuate)
        d_ta3 = _dev(ctx, ta3)
        direct0, dn0, up0, _, bdn0, _ = gm.lbl_fluxes_sw_rayleigh(mu, d_ssi, d_ta3, _dev(ctx, np.zeros_like(ta3)), d_alb)
        assert np.array_equal(dn0, direct0) and not np.any(np.isnan(bdn0))
        np.testing.assert_allclose(up0, gm.lbl_fluxes_sw(mu, d_ssi, d_ta3, d_alb)[1], rtol=1e-14, atol=0.0)
    finally:
        gm.close()


def test_an_angle_among_eight_has_the_bits_of_the_angle_alone(ctx):
    nlay, nwav = 8, 257
    all_g, all_s = _run_g(ctx, nlay, nwav, 8), _run_s(ctx, nlay, nwav, 8)
    for s in (0, 2, 7):
        one = _angles(8)[s:s + 1]
        for a, b in zip(all_g + all_s, _run_g(ctx, nlay, nwav, 1, angles=one) + _run_s(ctx, nlay, nwav, 1, angles=one)):
            assert np.array_equal(a[s], b[0])


@pytest.mark.parametrize("f32", [(False, False), (True, False), (False, True), (True, True)])
def test_optical_depth_types(ctx, f32):
    nlay, nwav, nsza = 3, 257, 5
    ref = _closed(nlay, nwav, nsza, True, f32)                       # on the values the device sees
    _check_g(ref, _run_g(ctx, nlay, nwav, nsza, f32=f32), nlay, nwav, nsza, 1e-9, f"closed f32={f32}")
    _check_s(ref, _run_s(ctx, nlay, nwav, nsza, f32=f32), nlay, nwav, nsza, 1e-9, f"closed f32={f32}")


_GRID_SCRIPT = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from ecckd_amd import api
import test_lbl_gpoint_fluxes_sw_rayleigh_gpu as t
with api.Context(0) as ctx:
    out = t._run_g(ctx, 3, 1100, 5) + t._run_s(ctx, 3, 1100, 5)
np.savez(sys.argv[1], *out)
"""


def test_physical_blocks_loop_over_logical_ones_when_the_grid_is_capped(ctx, tmp_path):
    """Five logical blocks on two physical ones (ECCKD_RAYLEIGH_GRID=2, read when the library launches: a process of its own):
    the bits of the unbounded run, and the restatement's values."""
    nlay, nwav, nsza = 3, 1100, 5
    assert L.tile_grid(nwav) == (1, 5)
    ref_g, ref_s = _run_g(ctx, nlay, nwav, nsza), _run_s(ctx, nlay, nwav, nsza)
    _check_g(_closed(nlay, nwav, nsza), ref_g, nlay, nwav, nsza, 1e-9, "closed")
    _check_s(_closed(nlay, nwav, nsza), ref_s, nlay, nwav, nsza, 1e-9, "closed")
    script = tmp_path / "grid.py"
    script.write_text(_GRID_SCRIPT % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, ECCKD_RAYLEIGH_GRID="2")
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    got = np.load(tmp_path / "out.npz")
    for i, a in enumerate(ref_g + ref_s):
        assert np.array_equal(a, got[f"arr_{i}"]), i


def test_bad_arguments(ctx):
    import torch
    from ecckd_amd import _lib
    nlay, nwav = 3, 37
    ta, tr, ssi, _ = _case(nlay, nwav)
    d_ta, d_tr, d_ssi = _dev(ctx, ta), _dev(ctx, tr), _dev(ctx, ssi)
    gm = _make_map(ctx, _gmap(nwav), NG)
    out = [np.empty((8, nlay + 1, NG)) for _ in range(3)]
    spec = [torch.empty((8, nlay + 1, nwav), dtype=torch.float32, device=ctx.device) for _ in range(3)]
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda t: C.c_void_p(t.data_ptr())

    def call_g(nsza=1, mu=(0.5,), abs_type=_lib.F64, abs_stride=nwav, ray_type=_lib.F64, ray_stride=nwav):
        m = np.array(list(mu) + [0.5] * 9, dtype=np.float64)
        return ctx.lib.ecckd_lbl_gpoint_fluxes_sw_rayleigh(gm.handle, nlay, nsza, hp(m), vp(d_ssi), None, vp(d_ta), abs_type, abs_stride,
                                                           vp(d_tr), ray_type, ray_stride, hp(out[0]), hp(out[1]), hp(out[2]), None, None,
                                                           None)

    def call_s(nsza=1, mu=(0.5,), abs_type=_lib.F64, abs_stride=nwav, ray_type=_lib.F64, ray_stride=nwav, flux_stride=nwav):
        m = np.array(list(mu) + [0.5] * 9, dtype=np.float64)
        return ctx.lib.ecckd_lbl_spectral_fluxes_sw_rayleigh(ctx.handle, nlay, nwav, nsza, hp(m), vp(d_ssi), None, vp(d_ta), abs_type,
                                                             abs_stride, vp(d_tr), ray_type, ray_stride, vp(spec[0]), vp(spec[1]),
                                                             vp(spec[2]), flux_stride, None, None, None)
    try:
        assert call_g() == 0 and call_s() == 0
        bad = (dict(nsza=0), dict(nsza=9), dict(mu=(0.0,)), dict(mu=(1.5,)), dict(abs_stride=nwav - 1), dict(ray_stride=nwav - 1),
               dict(abs_type=3), dict(ray_type=3))
        for kw in bad:
            assert call_g(**kw) == _lib.PARAMETER_ERROR, kw
            assert call_s(**kw) == _lib.PARAMETER_ERROR, kw
        assert call_s(flux_stride=nwav - 1) == _lib.PARAMETER_ERROR
    finally:
        gm.close()
