"""The closed-form Rayleigh two-stream transfer (rayleigh_ref.two_stream_closed, the restatement of csrc/lbl_rt.hpp) against
the formula-free solve (two_stream_exact), its energy budget and its no-scattering limit.  CPU only.

Every tolerance is absolute and per unit incoming flux mu0 * ssi: the direct-to-diffuse terms are O(w), so a relative
tolerance on them asks for digits no flux has."""
import numpy as np
import pytest

import rayleigh_ref as rr

MU0 = (0.1, 0.3, 0.5, 0.7, 0.9, 1.0)
ALBEDO = (0.0, 0.15, 1.0)


def _worst(tau_abs, tau_ray, mu0, albedo):
    """max |closed - exact| over the three fluxes and all levels, per unit mu0 * ssi (ssi = 1)."""
    ex = rr.two_stream_exact(tau_abs, tau_ray, mu0, albedo)
    cl = rr.two_stream_closed(tau_abs, tau_ray, mu0, albedo)
    return max(float(np.max(np.abs(c - e))) for c, e in zip(cl, ex)) / mu0


def _random_columns(n=400, seed=11):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        nlay = int(rng.integers(1, 9))
        tau = [np.where(rng.random(nlay) < 0.2, 0.0, np.exp(rng.uniform(np.log(1e-6), np.log(5.0), nlay))) for _ in range(2)]
        yield tau[0], tau[1], float(rng.choice(MU0)), float(rng.choice(ALBEDO))


def _k(w):
    g1, g2 = 2.0 - 1.25 * w, 0.75 * w
    return np.sqrt(max((g1 - g2) * (g1 + g2), 1e-12))


def _resonance_cases():
    eps = [0.0, 1e-3]
    for e in (1e-15, 1e-12, 1e-9, 1e-6, 0.9e-4, 1.1e-4):     # both sides of h: the treatment is continuous there
        eps += [e, -e]
    for w in (1e-6, 0.3, 0.9, 0.99):
        for tau in (1e-3, 0.7, 5.0):
            for e in eps:
                yield w, tau, (1.0 + e) / _k(w)


def test_closed_against_exact_random_columns():
    worst = max(_worst(*case) for case in _random_columns())
    print(f"random columns: worst |closed - exact| per unit incoming flux = {worst:.3e}")
    assert worst <= rr.EXACT_BOUND


def test_closed_against_exact_across_the_resonance():
    worst = 0.0
    for w, tau, mu0 in _resonance_cases():
        for albedo in (0.0, 0.15):
            worst = max(worst, _worst(np.array([tau * (1.0 - w)]), np.array([tau * w]), mu0, albedo))
    print(f"resonance: worst |closed - exact| per unit incoming flux = {worst:.3e}")
    assert worst <= rr.EXACT_BOUND


@pytest.mark.parametrize("w", [1e-300, 1e-16, 1e-12, 1e-8])
def test_closed_against_exact_tiny_w_at_default_sun_angle(w):
    """k mu0 = 1 lies at w = 0, mu0 = 0.5: every weakly scattering layer at the default angle is next to the resonance."""
    worst = max(_worst(np.array([tau]), np.array([tau * w]), 0.5, 0.15) for tau in (1e-3, 0.7, 5.0))
    print(f"w = {w:g}: worst |closed - exact| per unit incoming flux = {worst:.3e}")
    assert worst <= rr.EXACT_BOUND


def test_recorded_bound_is_ten_times_the_measured_difference():
    assert rr.EXACT_BOUND == 10.0 * rr.MEASURED_CLOSED_VS_EXACT
    assert rr.MEASURED_CLOSED_VS_EXACT <= 1e-7       # beyond that the resonance treatment is not good enough


def test_energy_conservation_without_absorption():
    """tau_abs = 0: what the surface absorbs plus what leaves at the top is what came in."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        nlay = int(rng.integers(1, 9))
        tau_ray = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), nlay))
        mu0, albedo = float(rng.choice(MU0)), float(rng.choice(ALBEDO))
        d, dn, up = rr.two_stream_closed(np.zeros(nlay), tau_ray, mu0, albedo)
        worst = max(worst, abs((1.0 - albedo) * (dn[-1] + d[-1]) + up[0] - mu0) / mu0)
    print(f"energy: worst imbalance per unit incoming flux = {worst:.3e}")
    assert worst <= rr.EXACT_BOUND


def test_no_scattering_limit():
    """tau_ray = 0: no diffuse downwelling flux, and the upwelling one is the reflected beam attenuated by exp(-2 tau)."""
    rng = np.random.default_rng(6)
    for mu0 in MU0:
        nlay = 8
        tau = np.exp(rng.uniform(np.log(1e-6), np.log(5.0), (nlay, 50)))
        albedo = rng.choice(ALBEDO[1:], 50)
        d, dn, up = rr.two_stream_closed(tau, np.zeros_like(tau), mu0, albedo, incoming=2.0)
        assert np.all(dn == 0.0)
        ref = albedo * d[nlay]
        np.testing.assert_allclose(up[nlay], ref, rtol=1e-14)
        for l in range(nlay - 1, -1, -1):
            ref = ref * np.exp(-2.0 * tau[l])
            np.testing.assert_allclose(up[l], ref, rtol=1e-14)
