"""GPU parity for the Rayleigh two-stream band fluxes of many scenarios from one read of the spectra
(ecckd_lbl_band_fluxes_sw_rayleigh_scenarios, csrc/lbl_scenarios_sw_rayleigh.hip).  The reference of every comparison is the
parent's single-scenario path, which tests/test_lbl_fluxes_sw_rayleigh_gpu.py pins to tests/rayleigh_ref.py: api.merge_spectrum
gas after gas into a DOUBLE matrix, then api.lbl_band_fluxes_sw_rayleigh.  The fused call is its own reference only in the
bit-equality properties; one small case goes straight to rayleigh_ref.two_stream_closed, against an error shared with the parent.

Bounds.  Against the parent path and against two_stream_closed: 1e-9 x mu0 x sum(ssi) of the band (mu0 x ssi for a spectral
array), the absolute bound this transfer is held to on the device.  The direct beam and the no-scattering upwelling flux against
api.lbl_band_fluxes_sw_scenarios: rtol 1e-12, atol 1e-15 x the largest flux, the bound of tests/test_lbl_scenarios_gpu.py
(identical merged optical depths; only the contraction of the recurrence may differ).  Run with -s for the observed figures;
DESIGN.md records them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rayleigh_ref as rr
import test_lbl_fluxes_sw_rayleigh_gpu as tr1
import test_lbl_scenarios_gpu as ts

pytestmark = pytest.mark.gpu

NSCEN = 5                                            # _scales: as is; first gas at 0; a profile; the same profile; a factor per gas
SHAPES = [(1, 37, 1), (3, 600, 5), (8, 257, 8), (54, 300, 5)]
# (the absorbers' types, the Rayleigh row's type, a per-wavenumber albedo or None)
VARIANTS = {
    "f32-ray32": (("float32",), "float32", True),
    "f64-ray64": (("float64",), "float64", True),
    "mixed-ray32-noalbedo": (("float32", "float64", "float32"), "float32", False),
    "mixed-ray64": (("float32", "float64", "float32"), "float64", True),
}
CASES = [(s, v) for s in SHAPES for v in VARIANTS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{v}" for s, v in CASES]


def _bands(nwav):
    """BEGIN / END of tests/test_lbl_scenarios_gpu.py cut to nwav (at nwav = 1000: [0, 599], [600, 639], empty, [640, 997]): the
    first band ends inside a chunk, the second is narrower than a wave, the third is empty, and the last two wavenumbers
    belong to no band."""
    e0 = (3 * nwav) // 5 - 1
    w = max(1, min(40, (nwav - e0 - 1) // 3))
    return np.array([0, e0 + 1, 0, e0 + w + 1]), np.array([e0, e0 + w, -1, nwav - 3])


def _nchunk(nwav):
    return int(sum(-(-(e - b + 1) // 256) for b, e in zip(*_bands(nwav)) if e >= b))


@functools.lru_cache(maxsize=None)
def _inputs(nlay, nwav, variant):
    """(absorbers, Rayleigh row, ssi, albedo or None, scales) as numpy arrays, read-only.  The absorbers are _spectra of the
    scenarios test; the Rayleigh row is built like _case of the Rayleigh test on the merged optical depth of scenario 0."""
    dtypes, ray_dtype, with_albedo = VARIANTS[variant]
    rng = np.random.default_rng(100 * nlay + nwav)
    kind = rng.random((nlay, nwav))
    ods = [np.ascontiguousarray(o[:, :nwav]) for o in ts._spectra(nlay, dtypes, seed=17)]
    for o in ods:
        o[(kind >= 0.2) & (kind < 0.4)] = 0.0                        # a fifth do not absorb
    ta = np.zeros((nlay, nwav))
    for o in ods:
        ta = ta + o.astype(np.float64)
    ray = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), (nlay, nwav)))
    ray[kind < 0.2] = 0.0                                            # a fifth do not scatter
    sel = (kind >= 0.4) & (kind < 0.5)
    ray[sel] = 0.3 * ta[sel] / 0.7                                   # w = 0.3: an angle of _angles sits on their resonance
    sel = (kind >= 0.5) & (kind < 0.6)
    ray[sel] = ta[sel] * 10.0 ** rng.uniform(-12, -4, int(sel.sum()))   # weakly scattering: next to the resonance of mu0 = 0.5
    ray = ray.astype(ray_dtype)
    ssi = rng.uniform(0.5, 2.0, nwav)
    albedo = rng.choice([0.0, 0.15, 1.0], nwav) if with_albedo else None
    scales = ts._scales(NSCEN, len(dtypes), nlay, seed=5)
    for a in ods + [ray, ssi, scales] + ([albedo] if with_albedo else []):
        a.setflags(write=False)
    return tuple(ods), ray, ssi, albedo, scales


def _dev(ctx, a):
    return None if a is None else torch.as_tensor(np.array(a), device=ctx.device)        # (a copy: the inputs are read-only)


def _call(ctx, nlay, nwav, nsza, variant, scales=None, angles=None, ray=None):
    """The fused call with boundary arrays, everything on the host: (direct, dn, up, surf_direct, surf_dn, toa_up)."""
    from ecckd_amd import api
    ods, ray0, ssi, albedo, sc = _inputs(nlay, nwav, variant)
    b0, b1 = _bands(nwav)
    out = api.lbl_band_fluxes_sw_rayleigh_scenarios(ctx, tr1._angles(nsza) if angles is None else angles, _dev(ctx, ssi),
                                                    [_dev(ctx, o) for o in ods], _dev(ctx, ray0 if ray is None else ray),
                                                    sc if scales is None else scales, b0, b1, albedo=_dev(ctx, albedo), boundary=True)
    return out[:3] + tuple(t.cpu().numpy() for t in out[3:])


_FUSED = {}


def _fused(ctx, nlay, nwav, nsza, variant):
    """The unforced call of a case, computed once and shared (never written to)."""
    key = (nlay, nwav, nsza, variant)
    if key not in _FUSED:
        _FUSED[key] = _call(ctx, nlay, nwav, nsza, variant)
        for a in _FUSED[key]:
            a.setflags(write=False)
    return _FUSED[key]


def _incoming(nwav, nsza, ssi):
    """mu0 x sum(ssi) per (angle, band), and mu0 x ssi per (angle, wavenumber)"""
    mu = tr1._angles(nsza)
    band = np.array([ssi[b:e + 1].sum() if e >= b else 0.0 for b, e in zip(*_bands(nwav))])
    return mu[:, None] * band[None, :], mu[:, None] * ssi[None, :]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape,variant", CASES, ids=IDS)
def test_against_the_parent_path(ctx, shape, variant):
    """Assertions 1 and 6: every scenario and angle against merge_spectrum + lbl_band_fluxes_sw_rayleigh; the empty band, the
    wavenumbers outside the bands, a real flux in the first band."""
    from ecckd_amd import api
    nlay, nwav, nsza = shape
    ods, ray, ssi, albedo, sc = _inputs(nlay, nwav, variant)
    b0, b1 = _bands(nwav)
    got = _fused(ctx, nlay, nwav, nsza, variant)
    assert all(g.shape == (NSCEN, nsza, 4, nlay + 1) for g in got[:3]) and all(g.shape == (NSCEN, nsza, nwav) for g in got[3:])
    d_ods, d_ray, d_ssi, d_alb = [_dev(ctx, o) for o in ods], _dev(ctx, ray), _dev(ctx, ssi), _dev(ctx, albedo)
    band_in, spec_in = _incoming(nwav, nsza, ssi)
    inb = tr1._in_bands(nwav, b0, b1)
    worst, bitwise = 0.0, True
    for s in range(NSCEN):
        ref = api.lbl_band_fluxes_sw_rayleigh(ctx, tr1._angles(nsza), d_ssi, ts._merged(ctx, d_ods, sc[s]), d_ray, b0, b1, albedo=d_alb,
                                              boundary=True)
        ref = ref[:3] + tuple(t.cpu().numpy() for t in ref[3:])
        for k in range(3):
            err = np.abs(got[k][s] - ref[k]) / np.maximum(band_in[:, :, None], 1e-300) * (band_in[:, :, None] > 0)
            worst = max(worst, float(err.max()))
            assert np.all(np.abs(got[k][s] - ref[k]) <= 1e-9 * band_in[:, :, None]), (s, k, float(err.max()))
        for k in range(3, 6):
            err = np.abs(got[k][s] - ref[k])[:, inb] / spec_in[:, inb]
            worst = max(worst, float(err.max()))
            assert np.all(np.abs(got[k][s] - ref[k]) <= 1e-9 * spec_in), (s, k, float(err.max()))
        bitwise &= _same([g[s] for g in got], ref)
    print(f"\nrayleigh scenarios {shape} {variant}: largest difference to the parent path {worst:.3e} of the incoming flux, bitwise: {bitwise}")
    for g in got[:3]:
        assert np.all(g[:, :, 2] == 0.0)                             # the empty band
    for g in got[3:]:
        assert np.all(g[:, :, ~inb] == 0.0)                          # outside the bands
    assert np.all(got[0][:, :, 0, 0] > 0) and np.all(got[1][:, :, 0, 0] > 0)
    assert np.all(np.isfinite(np.concatenate([g.ravel() for g in got])))


@pytest.mark.parametrize("shape,variant", CASES, ids=IDS)
def test_direct_beam_against_the_no_scattering_scenarios(ctx, shape, variant):
    """Assertion 2: the Rayleigh row as one more gas at scale 1 gives the same merged optical depth, bit for bit."""
    from ecckd_amd import api
    nlay, nwav, nsza = shape
    ods, ray, ssi, albedo, sc = _inputs(nlay, nwav, variant)
    got = _fused(ctx, nlay, nwav, nsza, variant)
    sc1 = np.concatenate([sc, np.ones((NSCEN, 1, nlay))], axis=1)
    rdn, _, rsdn, _ = api.lbl_band_fluxes_sw_scenarios(ctx, tr1._angles(nsza), _dev(ctx, ssi), [_dev(ctx, o) for o in ods + (ray,)], sc1,
                                                       *_bands(nwav), albedo=_dev(ctx, albedo), boundary=True)
    bitwise = True
    for s in range(NSCEN):
        bitwise &= ts._close(got[0][s], rdn[s], f"flux_dn_direct of scenario {s}")
        bitwise &= ts._close(got[3][s], rsdn.cpu().numpy()[s], f"direct surface spectrum of scenario {s}")
    print(f"\nrayleigh scenarios {shape} {variant}: direct beam bitwise equal to the no-scattering scenarios: {bitwise}")


@pytest.mark.parametrize("shape,variant", CASES, ids=IDS)
def test_without_scattering(ctx, shape, variant):
    """Assertion 3: a Rayleigh row of zeros."""
    from ecckd_amd import api
    nlay, nwav, nsza = shape
    ods, ray, ssi, albedo, sc = _inputs(nlay, nwav, variant)
    direct, dn, up, sdir, sdn, tup = _call(ctx, nlay, nwav, nsza, variant, ray=np.zeros_like(ray))
    assert np.array_equal(dn, direct) and np.array_equal(sdn, sdir)
    _, rup, _, rtup = api.lbl_band_fluxes_sw_scenarios(ctx, tr1._angles(nsza), _dev(ctx, ssi), [_dev(ctx, o) for o in ods], sc, *_bands(nwav),
                                                       albedo=_dev(ctx, albedo), boundary=True)
    for s in range(NSCEN):
        ts._close(up[s], rup[s], f"flux_up of scenario {s}")
        ts._close(tup[s], rtup.cpu().numpy()[s], f"TOA spectrum of scenario {s}")


@pytest.mark.parametrize("shape,variant", CASES, ids=IDS)
def test_bit_equality(ctx, shape, variant, monkeypatch):
    """Assertion 4: a scenario alone, an angle alone, the identical scenarios, a forced grid (two blocks loop over the chunks
    and reuse the workspace), a forced budget (three launches: 2 + 2 + 1 scenarios), one factor per gas."""
    from ecckd_amd import api
    nlay, nwav, nsza = shape
    sc = _inputs(nlay, nwav, variant)[4]
    got = _fused(ctx, nlay, nwav, nsza, variant)
    assert _same([g[2] for g in got], [g[3] for g in got])
    for s in range(NSCEN):
        alone = _call(ctx, nlay, nwav, nsza, variant, scales=sc[s:s + 1])
        assert _same([a[0] for a in alone], [g[s] for g in got]), s
    for a in sorted({0, nsza // 2, nsza - 1}) if nsza > 1 else []:
        one = _call(ctx, nlay, nwav, 1, variant, angles=tr1._angles(nsza)[a:a + 1])
        assert _same([o[:, 0] for o in one], [g[:, a] for g in got]), a
    flat = _call(ctx, nlay, nwav, nsza, variant, scales=sc[[0, 1, 4]][:, :, 0])
    assert _same(flat, [g[[0, 1, 4]] for g in got])
    nchunk = _nchunk(nwav)
    assert nchunk >= 3
    assert api.lbl_rayleigh_scenarios_per_launch(nlay, nsza, nchunk) >= NSCEN          # unforced: one launch
    monkeypatch.setenv("ECCKD_RAYLEIGH_GRID", "2")
    assert _same(_call(ctx, nlay, nwav, nsza, variant), got)
    monkeypatch.delenv("ECCKD_RAYLEIGH_GRID")
    monkeypatch.setenv("ECCKD_RAYLEIGH_SCENARIO_BYTES", str(2 * nchunk * nsza * 3 * (nlay + 1) * 8))
    assert api.lbl_rayleigh_scenarios_per_launch(nlay, nsza, nchunk) == 2
    assert _same(_call(ctx, nlay, nwav, nsza, variant), got)
    monkeypatch.setenv("ECCKD_RAYLEIGH_GRID", "2")                                    # both at once
    assert _same(_call(ctx, nlay, nwav, nsza, variant), got)


def test_against_the_restatement(ctx):
    """Assertion 5: (3, 37, 5) against rayleigh_ref.two_stream_closed on the merged optical depths formed in numpy (product and
    sum rounded separately, in gas order)."""
    nlay, nwav, nsza, variant = 3, 37, 5, "mixed-ray64"
    ods, ray, ssi, albedo, sc = _inputs(nlay, nwav, variant)
    b0, b1 = _bands(nwav)
    got = _call(ctx, nlay, nwav, nsza, variant)
    band_in, spec_in = _incoming(nwav, nsza, ssi)
    inb = tr1._in_bands(nwav, b0, b1)
    worst = 0.0
    for s in range(NSCEN):
        tau = None
        for g, o in enumerate(ods):
            v = o.astype(np.float64) * sc[s, g][:, None]
            tau = v if tau is None else tau + v
        out = [rr.two_stream_closed(tau, ray.astype(np.float64), mu, albedo, ssi) for mu in tr1._angles(nsza)]
        d, dn, up = (np.stack([o[i] for o in out]) for i in range(3))             # (nsza, nlay+1, nwav)
        for k, want in enumerate((d, d + dn, up)):
            diff = np.abs(got[k][s] - tr1._band_sums(want, b0, b1))
            worst = max(worst, float(np.max(diff / np.maximum(band_in[:, :, None], 1e-300) * (band_in[:, :, None] > 0))))
            assert np.all(diff <= 1e-9 * band_in[:, :, None]), (s, k)
        for k, want in ((3, d[:, -1]), (4, d[:, -1] + dn[:, -1]), (5, up[:, 0])):
            diff = np.abs(got[k][s] - want * inb)
            worst = max(worst, float(np.max(diff[:, inb] / spec_in[:, inb])))
            assert np.all(diff <= 1e-9 * spec_in), (s, k)
    print(f"\nrayleigh scenarios against two_stream_closed: {worst:.3e} of the incoming flux (allowed 1e-9)")


def test_refusals(ctx):
    """Assertion 7: every PARAMETER_ERROR of the entry, the library called directly with one wrong argument; the outputs keep
    what they held."""
    from ecckd_amd import _lib, api
    nlay, nwav, nsza, variant = 3, 37, 5, "mixed-ray64"
    ods, ray, ssi, albedo, sc = _inputs(nlay, nwav, variant)
    d_ods, d_ray, d_ssi = [_dev(ctx, o) for o in ods], _dev(ctx, ray), _dev(ctx, ssi)
    hp = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
    b0, b1 = (np.ascontiguousarray(b, dtype=np.int64) for b in _bands(nwav))
    scale = np.ones(2 * 17 * nlay)
    out = [np.full(2 * 8 * 4 * (nlay + 1), -7.0) for _ in range(3)]
    d_out = [torch.full((2 * 8 * nwav,), -7.0, dtype=torch.float64, device=ctx.device) for _ in range(3)]
    ptrs = (C.c_void_p * 17)(*[d_ods[g % 3].data_ptr() for g in range(17)])
    types = (C.c_int * 17)(*[_lib.F32 if o.dtype == np.float32 else _lib.F64 for o in [ods[g % 3] for g in range(17)]])
    strides = (C.c_size_t * 17)(*([nwav] * 17))
    mu = np.ascontiguousarray(np.linspace(0.1, 0.9, 9))
    ctx.fence_from_torch()
    ok = dict(nsza=2, mu=hp(mu), ngas=3, od=ptrs, ty=types, st=strides, ray=C.c_void_p(d_ray.data_ptr()), ray_type=_lib.F64,
              ray_stride=nwav, nscen=2)

    def call(**kw):
        a = dict(ok, **kw)
        r = ctx.lib.ecckd_lbl_band_fluxes_sw_rayleigh_scenarios(ctx.handle, nlay, nwav, a["nsza"], a["mu"], C.c_void_p(d_ssi.data_ptr()), None,
                                                                a["ngas"], a["od"], a["ty"], a["st"], a["ray"], a["ray_type"],
                                                                a["ray_stride"], a["nscen"], hp(scale), 4, hp(b0, C.c_int64),
                                                                hp(b1, C.c_int64), hp(out[0]), hp(out[1]), hp(out[2]),
                                                                *[C.c_void_p(d.data_ptr()) for d in d_out])
        ctx.synchronize()
        return r

    bad_types = (C.c_int * 17)(*([_lib.F32, 2] + [_lib.F32] * 15))
    short = (C.c_size_t * 17)(*([nwav - 1] * 17))
    refused = [dict(ngas=0), dict(ngas=17), dict(nscen=0), dict(nsza=0), dict(nsza=9), dict(nsza=1, mu=hp(np.array([0.0]))),
               dict(st=short), dict(ray_stride=nwav - 1), dict(ty=bad_types), dict(ray_type=3), dict(ray=None)]
    for kw in refused:
        assert call(**kw) == _lib.PARAMETER_ERROR, kw
        assert all(np.all(o == -7.0) for o in out) and all(bool(torch.all(d == -7.0)) for d in d_out), kw
        assert b"ecckd_lbl_band_fluxes_sw_rayleigh_scenarios" in ctx.lib.ecckd_last_error(), kw
    assert call() == 0 and call(ngas=16) == 0 and call(nsza=8) == 0
    assert not np.any(out[0][:2 * 8 * 4 * (nlay + 1)] == -7.0)
    with pytest.raises(ValueError):
        api.lbl_band_fluxes_sw_rayleigh_scenarios(ctx, 0.5, d_ssi, d_ods, d_ray[:, :-1], sc, *_bands(nwav))
    with pytest.raises(ValueError):
        api.lbl_band_fluxes_sw_rayleigh_scenarios(ctx, 0.5, d_ssi, d_ods, d_ray[:-1], sc, *_bands(nwav))
    with pytest.raises(api.EcckdError) as e:
        api.lbl_band_fluxes_sw_rayleigh_scenarios(ctx, [0.5, 0.0], d_ssi, d_ods, d_ray, sc, *_bands(nwav))
    assert e.value.code == _lib.PARAMETER_ERROR
