"""The closed-form two-stream transfer under clouds (allsky_ref.two_stream_closed, the restatement of cloud_layer in
csrc/lbl_rt.hpp and of the sky kernel's dispatch) against the formula-free solve (allsky_ref.two_stream_exact), its clear
limit, the delta-Eddington identities and the energy budget of conservative scattering.  CPU only.

Every tolerance against the exact solve is absolute and per unit incoming flux mu0 * ssi, as in test_rayleigh_ref.py."""
import numpy as np

import allsky_ref as ar
import rayleigh_ref as rr

SSA = (0.5, 0.9, 0.999, 0.999999, 1.0)
ALBEDO = (0.0, 0.15, 0.6, 1.0)


def _worst(tau_abs, tau_ray, t, w, a, mu0, albedo, scale):
    """max |closed - exact| over the three fluxes and all levels, per unit mu0 * ssi (ssi = 1).  scale: the closed form scales
    the triple itself (delta_eddington = 1); otherwise it is handed the scaled triple (delta_eddington = 0: "already scaled").
    Either way the asymmetry that reaches the layer is a / (1 + a) < 0.5, so g3 = 0.5 - 0.75 gg mu0 stays positive: with an
    unscaled asymmetry beyond 2 / (3 mu0) Rdir of the closed form turns negative and its clamp at 0 leaves the two-stream
    equations (2e-3 per unit incoming flux on these columns), which is the clamp's doing and not what this test measures."""
    ts, ws, as_ = ar.delta_eddington(t, w, a)
    ex = ar.two_stream_exact(*ar.mix(tau_abs, tau_ray, ts, ws, as_), mu0, albedo)
    cl = ar.two_stream_closed(tau_abs, tau_ray, t, w, a, mu0, albedo, scale=True) if scale else \
        ar.two_stream_closed(tau_abs, tau_ray, ts, ws, as_, mu0, albedo, scale=False)
    return max(float(np.max(np.abs(c - e))) for c, e in zip(cl, ex)) / mu0


def _random_columns(n=400, seed=17):
    """tau_abs in 1e-6..5, tau_ray in 1e-6..2, a cloud of od 1e-3..50 in half the layers, w of SSA, a in 0..0.9, mu0 in 0.05..1"""
    rng = np.random.default_rng(seed)
    for i in range(n):
        nlay = int(rng.integers(1, 9))
        tau_abs = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), nlay))
        tau_ray = np.exp(rng.uniform(np.log(1e-6), np.log(2.0), nlay))
        t = np.where(rng.random(nlay) < 0.5, np.exp(rng.uniform(np.log(1e-3), np.log(50.0), nlay)), 0.0)
        w, a = rng.choice(SSA, nlay), rng.uniform(0.0, 0.9, nlay)
        yield tau_abs, tau_ray, t, w, a, float(rng.uniform(0.05, 1.0)), float(rng.choice(ALBEDO)), bool(i % 2)


def _k(ssa, gg):
    g1, g2 = 2.0 - ssa * (1.25 + 0.75 * gg), ssa * (0.75 - 0.75 * gg)
    return np.sqrt(max((g1 - g2) * (g1 + g2), 1e-12))


def _resonance_cases():
    """single layers of total (ssa, gg, tau), a quarter of the scattering Rayleigh and the rest a particulate of half the
    optical depth, with mu0 = (1 + e) / k on both sides of the window's edge h and inside it"""
    eps = [0.0, 1e-3]
    for e in (1e-15, 1e-12, 1e-9, 1e-6, 0.9e-4, 1.1e-4):
        eps += [e, -e]
    for ssa, gg in ((1e-6, 0.0), (0.3, 0.5), (0.5, 0.6), (0.6, 0.0), (0.65, 0.2)):
        assert 1.0 / _k(ssa, gg) <= 1.0 / 1.001
        for tau in (1e-3, 0.7, 5.0):
            tau_ray, t = 0.25 * ssa * tau, 0.5 * tau
            w, a = 1.5 * ssa, gg / 0.75
            tau_abs = tau - tau_ray - t
            m_tau, m_ssa, m_gg = (float(v) for v in ar.mix(tau_abs, tau_ray, t, w, a))
            assert abs(m_ssa - ssa) < 1e-12 and abs(m_gg - gg) < 1e-12 and abs(m_tau - tau) < 1e-12
            for e in eps:
                yield tau_abs, tau_ray, t, w, a, (1.0 + e) / _k(m_ssa, m_gg)


def test_closed_against_exact_random_columns():
    worst = max(_worst(*case) for case in _random_columns())
    print(f"random columns: worst |closed - exact| per unit incoming flux = {worst:.3e}")
    assert worst <= ar.EXACT_BOUND


def test_closed_against_exact_across_the_resonance():
    worst, inside = 0.0, 0
    for tau_abs, tau_ray, t, w, a, mu0 in _resonance_cases():
        k = _k(*(float(v) for v in ar.mix(tau_abs, tau_ray, t, w, a)[1:]))
        inside += abs(1.0 - k * mu0) < ar.RESONANCE_H
        for albedo in (0.0, 0.15):
            worst = max(worst, _worst(*(np.array([v]) for v in (tau_abs, tau_ray, t, w, a)), mu0, albedo, False))
    print(f"resonance: worst |closed - exact| per unit incoming flux = {worst:.3e} ({inside} cases inside the window)")
    assert inside >= 100
    assert worst <= ar.EXACT_BOUND


def test_recorded_bound_is_ten_times_the_measured_difference():
    assert ar.EXACT_BOUND == 10.0 * ar.MEASURED_CLOSED_VS_EXACT
    assert ar.MEASURED_CLOSED_VS_EXACT <= 1e-7       # beyond that the resonance treatment is not good enough


def test_without_cloud_it_is_the_rayleigh_closed_form():
    """cloud_od = 0 (and negative, and NaN: not > 0) in every layer: rayleigh_ref.two_stream_closed to 1e-15 relative"""
    rng = np.random.default_rng(3)
    for mu0 in (0.1, 0.5, 0.9):
        tau_abs = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), (8, 60)))
        tau_ray = np.exp(rng.uniform(np.log(1e-6), np.log(2.0), (8, 60)))
        albedo = rng.choice(ALBEDO, 60)
        want = rr.two_stream_closed(tau_abs, tau_ray, mu0, albedo, incoming=1.7)
        for none in (0.0, -1.0, np.nan):
            got = ar.two_stream_closed(tau_abs, tau_ray, np.full((8, 60), none), np.full((8, 60), 0.9), np.full((8, 60), 0.8), mu0,
                                       albedo, incoming=1.7)
            for g, w in zip(got, want):
                np.testing.assert_allclose(g, w, rtol=1e-15, atol=0.0)


def test_general_layer_without_particulate_is_the_rayleigh_layer():
    """the general closed form at t = 0 (not the dispatch): gg = 0 gives g3 = g4 = 0.5 and rayleigh_layer's terms"""
    rng = np.random.default_rng(4)
    tau_abs = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), 200))
    tau_ray = np.exp(rng.uniform(np.log(1e-6), np.log(2.0), 200))
    zero = np.zeros(200)
    for mu0 in (0.2, 0.5, 1.0):
        for g, w in zip(ar.general_layer(tau_abs, tau_ray, zero, zero, zero, mu0), rr.rayleigh_layer(tau_abs, tau_ray, mu0)):
            np.testing.assert_allclose(g, w, rtol=1e-13, atol=1e-16)


def test_delta_eddington_identities():
    rng = np.random.default_rng(8)
    t, w, a = np.exp(rng.uniform(-6, 4, 100)), rng.uniform(0.0, 1.0, 100), rng.uniform(0.0, 0.95, 100)
    ts, ws, as_ = ar.delta_eddington(t, w, np.zeros(100))           # a = 0 leaves the triple alone
    assert np.array_equal(ts, t) and np.array_equal(ws, w) and not as_.any()
    ts, ws, as_ = ar.delta_eddington(t, np.ones(100), a)            # conservative scattering stays conservative
    np.testing.assert_allclose(ws, 1.0, rtol=4e-16, atol=0.0)
    np.testing.assert_allclose(ts, t * (1.0 - a * a), rtol=1e-15)
    np.testing.assert_allclose(as_, a / (1.0 + a), rtol=1e-15)
    ts, ws, as_ = ar.delta_eddington(t, w, a)                       # the scattering that is left: w' t' = w t (1 - f)
    np.testing.assert_allclose(ws * ts, w * t * (1.0 - a * a), rtol=1e-14)


def test_conservative_scattering_keeps_the_net_flux():
    """ssa = 1 in every layer (no gas absorption, w = 1): the net flux at the top is the net flux at the bottom"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        nlay = int(rng.integers(1, 9))
        tau_ray = np.exp(rng.uniform(np.log(1e-6), np.log(2.0), nlay))
        t = np.where(rng.random(nlay) < 0.5, np.exp(rng.uniform(np.log(1e-3), np.log(50.0), nlay)), 0.0)
        mu0, albedo = float(rng.uniform(0.05, 1.0)), float(rng.choice(ALBEDO))
        d, dn, up = ar.two_stream_closed(np.zeros(nlay), tau_ray, t, np.ones(nlay), rng.uniform(0.0, 0.9, nlay), mu0, albedo)
        worst = max(worst, abs((d[0] + dn[0] - up[0]) - (d[-1] + dn[-1] - up[-1])) / mu0)
    print(f"conservation: worst net-flux difference per unit incoming flux = {worst:.3e}")
    assert worst <= ar.EXACT_BOUND


def test_longwave_restatement_at_a_black_surface_and_its_surface_line():
    """emissivity 1 and no skin temperature: the up sweep starts from planck_hl[nlay] exactly; emissivity 0: from dn[nlay]"""
    rng = np.random.default_rng(9)
    pl, tau = rng.uniform(1.0, 5.0, (8, 12)), np.exp(rng.uniform(np.log(1e-7), np.log(20.0), (7, 12)))
    for sec, wgt in (([1.66], [1.0]), ([1.2, 2.5, 7.0], [0.5, 0.3, 0.2])):
        dn, up = ar.lw_fluxes(pl, tau, sec, wgt)
        np.testing.assert_allclose(up[7], pl[7], rtol=4e-16)
        dn0, up0 = ar.lw_fluxes(pl, tau, sec, wgt, emissivity=0.0, planck_skin=3.0 * pl[7])
        assert np.array_equal(dn0, dn)
        np.testing.assert_allclose(up0[7], dn[7], rtol=4e-16)
        dn1, up1 = ar.lw_fluxes(pl, tau, sec, wgt, emissivity=0.7, planck_skin=1.5 * pl[7])
        np.testing.assert_allclose(up1[7], 0.7 * 1.5 * pl[7] + (1.0 - 0.7) * dn[7], rtol=1e-15)
        assert (up1 > 0).all() and not np.array_equal(up1, up)
