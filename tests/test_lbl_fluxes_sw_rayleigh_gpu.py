"""ecckd_lbl_band_fluxes_sw_rayleigh and ecckd_rt_sw_gpoints_rayleigh (csrc/lbl_fluxes_sw_rayleigh.hip, csrc/lbl_fluxes.hip)
against the two numpy references of tests/rayleigh_ref.py, against the no-scattering kernel where the two must agree, and at
the edges of the kernel's chunks, bounded grid and angle loop.

Tolerances are absolute and scaled by the incoming flux: 1e-9 mu0 sum(ssi) of the band (mu0 ssi for a spectral array) against
the restatement two_stream_closed, rayleigh_ref.EXACT_BOUND against the formula-free two_stream_exact."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import rayleigh_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _k(w):
    g1, g2 = 2.0 - 1.25 * w, 0.75 * w
    return np.sqrt((g1 - g2) * (g1 + g2))


def _angles(nsza):
    """nsza angles that hold mu0 = 0.5 (the resonance of every weakly scattering layer) and, from three angles on, an angle
    on the resonance of the layers _case builds with w = 0.3."""
    base = [0.5, 0.1, 1.0 / _k(0.3), 0.3, 0.7, 0.9, 1.0, 0.2]
    return np.array(base[:nsza])


@functools.lru_cache(maxsize=None)
def _case(nlay, nwav, seed=0):
    """One column: (tau_abs, tau_ray) float64 (nlay, nwav), ssi, albedo (nwav,).  Optical depths log-uniform in 1e-6..5; a
    fifth of the elements without scattering, a fifth without absorption, a tenth with w = 0.3 exactly as float64 sees it
    (an angle of _angles sits on their resonance), a tenth weakly scattering (next to the resonance of mu0 = 0.5)."""
    rng = np.random.default_rng(100 * nlay + nwav + seed)
    ta = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), (nlay, nwav)))
    tr = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), (nlay, nwav)))
    kind = rng.random((nlay, nwav))
    tr[kind < 0.2] = 0.0
    ta[(kind >= 0.2) & (kind < 0.4)] = 0.0
    sel = (kind >= 0.4) & (kind < 0.5)
    tr[sel] = 0.3 * ta[sel] / 0.7
    sel = (kind >= 0.5) & (kind < 0.6)
    tr[sel] = ta[sel] * 10.0 ** rng.uniform(-12, -4, int(sel.sum()))
    ssi = rng.uniform(0.5, 2.0, nwav)
    albedo = rng.choice([0.0, 0.15, 1.0], nwav)
    for a in (ta, tr, ssi, albedo):
        a.setflags(write=False)
    return ta, tr, ssi, albedo


def _bands(nwav):
    """Two bands with an empty one between them; the first ends inside a chunk wherever nwav > 20, and two wavenumbers at the
    end belong to no band."""
    e0 = min(nwav - 4, max(10, nwav // 3))
    return np.array([0, 5, e0 + 1]), np.array([e0, 4, nwav - 3])


@functools.lru_cache(maxsize=None)
def _closed(nlay, nwav, nsza, with_albedo=True, f32=(False, False), seed=0):
    """two_stream_closed for every angle on the values the device sees: (direct, diffuse, up), each (nsza, nlay+1, nwav)."""
    ta, tr, ssi, albedo = _case(nlay, nwav, seed)
    ta = ta.astype(np.float32).astype(np.float64) if f32[0] else ta
    tr = tr.astype(np.float32).astype(np.float64) if f32[1] else tr
    out = [rr.two_stream_closed(ta, tr, mu, albedo if with_albedo else 0.0, ssi) for mu in _angles(nsza)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def _band_sums(x, begin, end):
    """(nsza, nlay+1, nwav) -> (nsza, nband, nlay+1)"""
    return np.stack([x[:, :, b:e + 1].sum(-1) if e >= b else np.zeros(x.shape[:2]) for b, e in zip(begin, end)], axis=1)


def _in_bands(nwav, begin, end):
    m = np.zeros(nwav, dtype=bool)
    for b, e in zip(begin, end):
        m[b:e + 1] = True
    return m


def _run(ctx, nlay, nwav, nsza, with_albedo=True, f32=(False, False), seed=0, angles=None):
    import torch
    from ecckd_amd import api
    ta, tr, ssi, albedo = _case(nlay, nwav, seed)
    dev = lambda a, f=False: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32 if f else np.float64), device=ctx.device)
    begin, end = _bands(nwav)
    mu = _angles(nsza) if angles is None else angles
    out = api.lbl_band_fluxes_sw_rayleigh(ctx, mu, dev(ssi), dev(ta, f32[0]), dev(tr, f32[1]), begin, end,
                                          albedo=dev(albedo) if with_albedo else None, boundary=True)
    return out[:3] + tuple(t.cpu().numpy() for t in out[3:])


def _check_against(ref, got, nlay, nwav, nsza, tol_rel, what):
    """Band fluxes and spectral boundary arrays of the device against (direct, diffuse, up) of a reference."""
    _, _, ssi, _ = _case(nlay, nwav)
    begin, end = _bands(nwav)
    mu = _angles(nsza)
    d, dn, up = ref
    bdir, bdn, bup, sdir, sdn, tup = got
    scale = mu[:, None, None] * _band_sums(np.broadcast_to(ssi, (nsza, 1, nwav)), begin, end)      # (nsza, nband, 1)
    for name, a, b in (("direct", bdir, d), ("dn", bdn, d + dn), ("up", bup, up)):
        err = np.max(np.abs(a - _band_sums(b, begin, end)) / np.maximum(scale, 1e-300) * (scale > 0))
        print(f"{what} nlay={nlay} nwav={nwav} nsza={nsza} band {name}: {err:.3e} of the incoming flux (allowed {tol_rel:.1e})")
        assert err <= tol_rel, (what, name, err)
        assert np.all(a[:, 1] == 0.0)                                # the empty band
    inb = _in_bands(nwav, begin, end)
    sscale = mu[:, None] * ssi[None, :]
    for name, a, b in (("surf direct", sdir, d[:, -1]), ("surf dn", sdn, d[:, -1] + dn[:, -1]), ("toa up", tup, up[:, 0])):
        err = np.max(np.abs(a - b)[:, inb] / sscale[:, inb])
        print(f"{what} nlay={nlay} nwav={nwav} nsza={nsza} spectral {name}: {err:.3e} of the incoming flux (allowed {tol_rel:.1e})")
        assert err <= tol_rel, (what, name, err)
        assert np.all(a[:, ~inb] == 0.0)                             # zero outside the bands


SHAPES = [(1, 37, 1), (3, 256, 5), (8, 257, 8), (3, 600, 1), (8, 37, 5), (1, 600, 8), (54, 300, 5)]


@pytest.mark.parametrize("nlay,nwav,nsza", SHAPES)
def test_against_the_restatement(ctx, nlay, nwav, nsza):
    _check_against(_closed(nlay, nwav, nsza), _run(ctx, nlay, nwav, nsza), nlay, nwav, nsza, 1e-9, "closed")


@functools.lru_cache(maxsize=None)
def _exact(nlay, nwav, nsza):
    ta, tr, ssi, albedo = _case(nlay, nwav)
    out = np.empty((3, nsza, nlay + 1, nwav))
    for s, mu in enumerate(_angles(nsza)):
        for j in range(nwav):
            out[:, s, :, j] = rr.two_stream_exact(ta[:, j], tr[:, j], mu, albedo[j], ssi[j])
    return out[0], out[1], out[2]


@pytest.mark.parametrize("nlay,nwav,nsza", [(1, 37, 1), (3, 257, 5), (8, 37, 8), (54, 300, 1)])
def test_against_the_exact_solve(ctx, nlay, nwav, nsza):
    _check_against(_exact(nlay, nwav, nsza), _run(ctx, nlay, nwav, nsza), nlay, nwav, nsza, rr.EXACT_BOUND, "exact")


@pytest.mark.parametrize("f32", [(False, False), (True, False), (False, True), (True, True)])
def test_optical_depth_types(ctx, f32):
    nlay, nwav, nsza = 3, 257, 5
    _check_against(_closed(nlay, nwav, nsza, True, f32), _run(ctx, nlay, nwav, nsza, f32=f32), nlay, nwav, nsza, 1e-9, f"closed f32={f32}")


def test_no_albedo_is_albedo_zero(ctx):
    nlay, nwav, nsza = 3, 257, 5
    got = _run(ctx, nlay, nwav, nsza, with_albedo=False)
    _check_against(_closed(nlay, nwav, nsza, False), got, nlay, nwav, nsza, 1e-9, "closed, no albedo")
    assert np.all(got[2][:, :, -1] == 0.0)                           # nothing leaves a black surface


def test_direct_beam_has_the_bits_of_the_no_scattering_kernel(ctx):
    """The direct flux is today's chain on tau = tau_abs + tau_ray formed in float64."""
    import torch
    from ecckd_amd import api
    nlay, nwav, nsza = 8, 600, 5
    ta, tr, ssi, albedo = _case(nlay, nwav)
    begin, end = _bands(nwav)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)
    bdir, _, _, sdir, _, _ = _run(ctx, nlay, nwav, nsza)
    for s, mu in enumerate(_angles(nsza)):
        rdn, _, rsdn, _ = api.lbl_band_fluxes_sw(ctx, mu, dev(ssi), dev(ta + tr), begin, end, albedo=dev(albedo), boundary=True)
        assert np.array_equal(sdir[s], rsdn.cpu().numpy())
        np.testing.assert_allclose(bdir[s], rdn, rtol=1e-13, atol=0.0)


def test_without_rayleigh_it_is_the_no_scattering_kernel(ctx):
    import torch
    from ecckd_amd import api
    nlay, nwav = 8, 600
    ta, _, ssi, albedo = _case(nlay, nwav)
    ta = np.maximum(ta, 1e-3)                                        # (tau_abs = 0 too would leave nothing to attenuate)
    begin, end = _bands(nwav)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)
    mu = np.array([0.5, 0.3, 0.9])
    bdir, bdn, bup, sdir, sdn, tup = api.lbl_band_fluxes_sw_rayleigh(ctx, mu, dev(ssi), dev(ta), dev(np.zeros_like(ta)), begin, end,
                                                                     albedo=dev(albedo), boundary=True)
    sdn, sdir = sdn.cpu().numpy(), sdir.cpu().numpy()
    print(f"tau_ray = 0: max |dn - direct| band {np.max(np.abs(bdn - bdir)):.3e} at {np.argwhere(bdn != bdir)[:4].tolist()}, "
          f"spectral {np.max(np.abs(sdn - sdir)):.3e} ({int(np.sum(sdn != sdir))} differ), nan {int(np.isnan(bdn).sum())}")
    assert np.array_equal(bdn, bdir) and np.array_equal(sdn, sdir)
    for s, m in enumerate(mu):
        _, rup, _, rtup = api.lbl_band_fluxes_sw(ctx, m, dev(ssi), dev(ta), begin, end, albedo=dev(albedo), boundary=True)
        np.testing.assert_allclose(bup[s], rup, rtol=1e-14, atol=0.0)
        np.testing.assert_allclose(tup[s].cpu().numpy(), rtup.cpu().numpy(), rtol=1e-14, atol=0.0)


def test_an_angle_among_eight_has_the_bits_of_the_angle_alone(ctx):
    nlay, nwav = 8, 257
    all8 = _run(ctx, nlay, nwav, 8)
    for s in (0, 2, 7):
        one = _run(ctx, nlay, nwav, 1, angles=_angles(8)[s:s + 1])
        for a, b in zip(all8, one):
            assert np.array_equal(a[s], b[0])


_GRID_SCRIPT = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from ecckd_amd import api
import test_lbl_fluxes_sw_rayleigh_gpu as t
with api.Context(0) as ctx:
    out = t._run(ctx, 3, 1100, 5)
np.savez(sys.argv[1], *out)
"""


def test_blocks_loop_over_chunks_when_the_grid_is_capped(ctx, tmp_path):
    """Five chunks on two blocks (ECCKD_RAYLEIGH_GRID=2, read when the library launches: a process of its own): the bits of
    the run with a block per chunk, and the restatement's values."""
    nlay, nwav, nsza = 3, 1100, 5
    begin, end = _bands(nwav)
    assert sum(-(-(e - b + 1) // 256) for b, e in zip(begin, end) if e >= b) == 5
    ref = _run(ctx, nlay, nwav, nsza)
    _check_against(_closed(nlay, nwav, nsza), ref, nlay, nwav, nsza, 1e-9, "closed")
    script = tmp_path / "grid.py"
    script.write_text(_GRID_SCRIPT % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, ECCKD_RAYLEIGH_GRID="2")
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    got = np.load(tmp_path / "out.npz")
    for i, a in enumerate(ref):
        assert np.array_equal(a, got[f"arr_{i}"]), i


def test_bad_arguments(ctx):
    import torch
    from ecckd_amd import _lib
    nlay, nwav = 3, 37
    ta, tr, ssi, _ = _case(nlay, nwav)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)
    d_ta, d_tr, d_ssi = dev(ta), dev(tr), dev(ssi)
    b0, b1 = np.array([0], dtype=np.int64), np.array([nwav - 1], dtype=np.int64)
    out = [np.empty((8, 1, nlay + 1)) for _ in range(3)]
    hp = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))

    def call(nsza=1, mu=(0.5,), abs_type=_lib.F64, abs_stride=nwav, ray_type=_lib.F64, ray_stride=nwav):
        m = np.array(list(mu) + [0.5] * 9, dtype=np.float64)
        return ctx.lib.ecckd_lbl_band_fluxes_sw_rayleigh(ctx.handle, nlay, nwav, nsza, hp(m), C.c_void_p(d_ssi.data_ptr()), None,
                                                         C.c_void_p(d_ta.data_ptr()), abs_type, abs_stride, C.c_void_p(d_tr.data_ptr()),
                                                         ray_type, ray_stride, 1, hp(b0, C.c_int64), hp(b1, C.c_int64), hp(out[0]),
                                                         hp(out[1]), hp(out[2]), None, None, None)
    assert call() == 0
    for kw in (dict(nsza=0), dict(nsza=9), dict(mu=(0.0,)), dict(mu=(1.5,)), dict(abs_stride=nwav - 1), dict(ray_stride=nwav - 1),
               dict(abs_type=3), dict(ray_type=3)):
        assert call(**kw) == _lib.PARAMETER_ERROR, kw
    z, one = np.zeros((1, nlay, 2)), np.ones((1, 2))
    f = [np.empty((1, nlay + 1, 2)) for _ in range(3)]
    g = lambda mu: ctx.lib.ecckd_rt_sw_gpoints_rayleigh(ctx.handle, 1, nlay, 2, mu, 0.15, hp(one), hp(z), hp(z), hp(f[0]), hp(f[1]), hp(f[2]))
    assert g(0.5) == 0 and g(0.0) == _lib.PARAMETER_ERROR and g(1.5) == _lib.PARAMETER_ERROR


@pytest.mark.parametrize("ncol,nlay,ng", [(2, 3, 5), (1, 8, 70)])
def test_rt_sw_gpoints_rayleigh(ctx, ncol, nlay, ng):
    from ecckd_amd import api
    rng = np.random.default_rng(ng)
    od = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), (ncol, nlay, ng)))
    ray = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), (ncol, nlay, ng)))
    kind = rng.random((ncol, nlay, ng))
    ray[kind < 0.2] = 0.0
    od[(kind >= 0.2) & (kind < 0.4)] = 0.0
    sel = kind > 0.8
    ray[sel] = 0.3 * od[sel] / 0.7
    inc = rng.uniform(10.0, 300.0, (ncol, ng))
    for mu in (0.5, 1.0 / _k(0.3), 0.9):
        for albedo in (0.0, 0.15, 1.0):
            direct, dn, up = api.rt_sw_gpoints_rayleigh(ctx, mu, albedo, inc, od, ray)
            for c in range(ncol):
                rd, rdn, rup = rr.two_stream_closed(od[c], ray[c], mu, albedo, inc[c])
                tol = 1e-9 * mu * inc[c]
                assert np.all(np.abs(direct[c] - rd) <= tol) and np.all(np.abs(dn[c] - (rd + rdn)) <= tol) and np.all(np.abs(up[c] - rup) <= tol)
            ex = [rr.two_stream_exact(od[0, :, g], ray[0, :, g], mu, albedo, inc[0, g]) for g in range(min(ng, 5))]
            for g, (ed, edn, eup) in enumerate(ex):
                tol = rr.EXACT_BOUND * mu * inc[0, g]
                assert np.all(np.abs(dn[0, :, g] - (ed + edn)) <= tol) and np.all(np.abs(up[0, :, g] - eup) <= tol)
