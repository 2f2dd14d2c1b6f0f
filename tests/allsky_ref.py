"""numpy float64 references of the resident fluxes under clouds and over a real surface (a helper module, not a conftest):
the formulas of ecckd_gas_optics_fluxes_{lw,sw}_sky_dev restated, and the exact two-stream solver of rayleigh_ref.py
generalised to a layer of single-scattering albedo ssa and asymmetry gg.

Shortwave, per layer: the gas (tau_abs, tau_ray) and a particulate (t, w, a), delta-Eddington scaled where asked
    f = a a,  t' = t (1 - w f),  w' = w (1 - f) / (1 - w f),  a' = a / (1 + a)
mix to  tau = tau_abs + tau_ray + t',  sc = tau_ray + w' t',  ssa = sc / tau,  gg = w' t' a' / sc,  and with t the optical
depth increasing downwards, U up, V diffuse down, D direct through a horizontal plane
    dU/dt =  g1 U - g2 V - ssa g3 D / mu0      g1 = 2 - ssa (1.25 + 0.75 gg),  g2 = ssa (0.75 - 0.75 gg)
    dV/dt =  g2 U - g1 V + ssa g4 D / mu0      g3 = 0.5 - 0.75 gg mu0,  g4 = 1 - g3
    dD/dt = -D / mu0                           V(0) = 0, D(0) = mu0 * ssi, surface: U = albedo (V + D)
A layer whose particulate optical depth is not > 0 is rayleigh_ref.rayleigh_layer itself.

two_stream_exact   rayleigh_ref.two_stream_exact with -ssa g3 / mu0 and +ssa g4 / mu0 in the source column
cloud_layer        restates cloud_layer of csrc/lbl_rt.hpp: Meador & Weaver's closed form with the k clamp, the ssa = 0 branch,
                   the clamps of Rdir and Tdd and the resonance treatment, the shifted angle in every place mu0 occurs
two_stream_closed  the adding sweeps of rayleigh_ref.two_stream_closed over such layers
lw_fluxes          the longwave sweeps of the kernel: every angle down, then every angle up from the Lambertian surface
"""
import numpy as np

import rayleigh_ref
from rayleigh_ref import RESONANCE_H, _expm

# Worst absolute difference of two_stream_closed against two_stream_exact per unit mu0 * ssi on the inputs of
# tests/test_allsky_ref.py, times 10 for a device build that contracts and orders sums differently.  Measured: 2.6e-13 on the
# 400 random columns (delta-Eddington scaled, in the kernel or before it), 2.7e-9 on the single layers swept across the
# resonance (the curvature the linear interpolation over 4h leaves), 5.3e-10 as the largest difference of the net fluxes at
# top and bottom under ssa = 1 (the k clamp at 1e-6, where 1 - exp(-2 k tau) cancels).  Not in the figure, because it is the
# clamp of Rdir at 0 and not the closed form: an UNSCALED asymmetry with 0.75 gg mu0 > 0.5 makes g3 negative, and the clamped
# layer then departs from the two-stream equations by up to 2e-3 on the same columns.
MEASURED_CLOSED_VS_EXACT = 2.7e-9
EXACT_BOUND = 10.0 * MEASURED_CLOSED_VS_EXACT


def delta_eddington(t, w, a):
    """(od, ssa, asymmetry) -> the delta-Eddington scaled triple"""
    t, w, a = (np.asarray(v, dtype=np.float64) for v in (t, w, a))
    f = a * a
    return t * (1.0 - w * f), w * (1.0 - f) / (1.0 - w * f), a / (1.0 + a)


def mix(tau_abs, tau_ray, t, w, a):
    """gas and (scaled) particulate -> (tau, ssa, gg) of the layer; ssa = gg = 0 where nothing scatters"""
    tau_abs, tau_ray, t, w, a = (np.asarray(v, dtype=np.float64) for v in (tau_abs, tau_ray, t, w, a))
    on = t > 0.0
    t = np.where(on, t, 0.0)
    tau = np.where(on, tau_abs + tau_ray + t, tau_abs + tau_ray)
    sc_cloud = np.where(on, w * t, 0.0)
    sc = tau_ray + sc_cloud
    scat = (sc > 0.0) & (tau > 0.0)
    with np.errstate(all="ignore"):
        ssa = np.where(scat, sc / np.where(scat, tau, 1.0), 0.0)
        gg = np.where(scat, sc_cloud * np.where(on, a, 0.0) / np.where(scat, sc, 1.0), 0.0)
    return tau, ssa, gg


# ---------------------------------------------------------------------------------------------------------------- exact
def two_stream_exact(tau, ssa, gg, mu0, albedo, incoming=1.0):
    """One column: tau, ssa, gg (nlay,), scalars mu0, albedo, incoming (= ssi) -> (direct, diffuse_dn, up), each (nlay+1,)."""
    tau, ssa, gg = (np.asarray(v, dtype=np.float64) for v in (tau, ssa, gg))
    nlay = tau.size
    nsub = np.maximum(1, np.ceil(tau)).astype(int)
    layer = np.repeat(np.arange(nlay), nsub)              # the layer of every sublayer
    t = (tau / nsub)[layer]
    ws, fac = ssa[layer], 0.75 * gg[layer]
    n = layer.size
    g1, g2 = 2.0 - ws * (1.25 + fac), ws * (0.75 - fac)
    g3 = 0.5 - mu0 * fac
    g4 = 1.0 - g3
    a = np.zeros((n, 3, 3))
    a[:, 0, 0], a[:, 0, 1], a[:, 0, 2] = g1, -g2, -ws * g3 / mu0
    a[:, 1, 0], a[:, 1, 1], a[:, 1, 2] = g2, -g1, ws * g4 / mu0
    a[:, 2, 2] = -1.0 / mu0
    p = _expm(a * t[:, None, None])
    d = np.empty(n + 1)
    d[0] = mu0 * incoming
    for i in range(n):
        d[i + 1] = d[i] * p[i, 2, 2]
    # unknowns U_0, V_0, U_1, V_1, ...: x_{i+1} = P_i x_i per sublayer, V_0 = 0, U_n = albedo (V_n + D_n)
    m = np.zeros((2 * n + 2, 2 * n + 2))
    rhs = np.zeros(2 * n + 2)
    for i in range(n):
        for r in range(2):
            m[2 * i + r, 2 * (i + 1) + r] = 1.0
            m[2 * i + r, 2 * i] = -p[i, r, 0]
            m[2 * i + r, 2 * i + 1] = -p[i, r, 1]
            rhs[2 * i + r] = p[i, r, 2] * d[i]
    m[2 * n, 1] = 1.0
    m[2 * n + 1, 2 * n], m[2 * n + 1, 2 * n + 1], rhs[2 * n + 1] = 1.0, -albedo, albedo * d[n]
    x = np.linalg.solve(m, rhs)
    at = np.concatenate([[0], np.cumsum(nsub)])            # interface index of every level
    return d[at], x[1::2][at], x[0::2][at]


# --------------------------------------------------------------------------------------------------------------- closed
def _direct_terms(w, k, e, e2, f, g1, g2, fac, tau, mu0):
    """Rdir and Tdd of the closed form with mu0 in every place it occurs: g3, g4, a1, a2 and Tdir (before the clamps)."""
    g3 = 0.5 - mu0 * fac
    g4 = 1.0 - g3
    a1 = g1 * g4 + g2 * g3
    a2 = g1 * g3 + g2 * g4
    km = k * mu0
    tdir = np.exp((-1.0 / mu0) * tau)
    f2 = w * f / (1.0 - km * km)
    rdir = f2 * ((1.0 - km) * (a2 + k * g3) - (1.0 + km) * (a2 - k * g3) * e2 - 2.0 * k * e * (g3 - a2 * mu0) * tdir)
    tdd = f2 * (2.0 * k * e * (g4 + a1 * mu0) - tdir * ((1.0 + km) * (a1 + k * g4) - (1.0 - km) * (a1 - k * g4) * e2))
    return rdir, tdd


def general_layer(tau_abs, tau_ray, t, ws, a, mu0):
    """cloud_layer of lbl_rt.hpp for arrays of one shape (the particulate already scaled, t taken as it is) ->
    (R, T, Tdir, Rdir, Tdd) per unit direct flux at the layer top"""
    tau_abs, tau_ray, t, ws, a = (np.asarray(v, dtype=np.float64) for v in (tau_abs, tau_ray, t, ws, a))
    tau = tau_abs + tau_ray + t
    sc_cloud = ws * t
    sc = tau_ray + sc_cloud
    scat = (sc > 0.0) & (tau > 0.0)
    with np.errstate(all="ignore"):
        w = np.where(scat, sc / np.where(scat, tau, 1.0), 0.5)          # (0.5: a harmless stand-in where the ssa = 0 branch is taken)
        gg = np.where(scat, sc_cloud * a / np.where(scat, sc, 1.0), 0.0)
        fac = 0.75 * gg
        g1, g2 = 2.0 - w * (1.25 + fac), w * (0.75 - fac)
        k = np.sqrt(np.maximum((g1 - g2) * (g1 + g2), 1e-12))
        e = np.exp(-k * tau)
        e2 = e * e
        f = 1.0 / (k + g1 + (k - g1) * e2)
        tdir = np.exp((-1.0 / mu0) * tau)
        r = g2 * (1.0 - e2) * f
        tr = 2.0 * k * e * f
        mu = np.full(tau.shape, float(mu0))
        rdir, tdd = _direct_terms(w, k, e, e2, f, g1, g2, fac, tau, mu)
        near = np.abs(1.0 - k * mu0) < RESONANCE_H
        if np.any(near):
            mu_a, mu_b = (1.0 - 2.0 * RESONANCE_H) / k, (1.0 + 2.0 * RESONANCE_H) / k
            ra, ta = _direct_terms(w, k, e, e2, f, g1, g2, fac, tau, mu_a)
            rb, tb = _direct_terms(w, k, e, e2, f, g1, g2, fac, tau, mu_b)
            x = (mu0 - mu_a) / (mu_b - mu_a)
            rdir = np.where(near, ra + (rb - ra) * x, rdir)
            tdd = np.where(near, ta + (tb - ta) * x, tdd)
        rdir = np.minimum(np.maximum(rdir, 0.0), 1.0 - tdir)
        tdd = np.minimum(np.maximum(tdd, 0.0), 1.0 - tdir - rdir)
        zero = np.zeros(tau.shape)
        return (np.where(scat, r, zero), np.where(scat, tr, np.exp(-2.0 * tau)), tdir, np.where(scat, rdir, zero),
                np.where(scat, tdd, zero))


def cloud_layer(tau_abs, tau_ray, t, w, a, mu0, scale=True):
    """The layer as the kernel dispatches it: rayleigh_ref.rayleigh_layer where the particulate optical depth is not > 0, else
    general_layer on the (scale: delta-Eddington scaled) triple.  -> (R, T, Tdir, Rdir, Tdd, tau), tau what the beam sees."""
    tau_abs, tau_ray, t, w, a = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (tau_abs, tau_ray, t, w, a)))
    on = t > 0.0
    clear = rayleigh_ref.rayleigh_layer(tau_abs, tau_ray, mu0)
    with np.errstate(all="ignore"):
        ts, ws, as_ = delta_eddington(t, w, a) if scale else (t, w, a)
    ts, ws, as_ = np.where(on, ts, 1.0), np.where(on, ws, 0.5), np.where(on, as_, 0.0)   # (stand-ins where the clear layer is taken)
    cloudy = general_layer(tau_abs, tau_ray, ts, ws, as_, mu0)
    return tuple(np.where(on, c, r) for c, r in zip(cloudy, clear)) + (np.where(on, tau_abs + tau_ray + ts, tau_abs + tau_ray),)


def two_stream_closed(tau_abs, tau_ray, cloud_od, cloud_ssa, cloud_asymmetry, mu0, albedo, incoming=1.0, scale=True):
    """tau_abs, tau_ray and the cloud triple (nlay,) or (nlay, n); mu0 a scalar; albedo and incoming (= ssi) scalars or (n,) ->
    (direct, dn, up), each (nlay+1,) or (nlay+1, n), dn the DIFFUSE downwelling flux (rayleigh_ref.two_stream_closed's)."""
    arrs = [np.asarray(v, dtype=np.float64) for v in (tau_abs, tau_ray, cloud_od, cloud_ssa, cloud_asymmetry)]
    one = arrs[0].ndim == 1
    if one:
        arrs = [v[:, None] for v in arrs]
    nlay, n = arrs[0].shape
    albedo = np.broadcast_to(np.asarray(albedo, dtype=np.float64), (n,))
    incoming = np.broadcast_to(np.asarray(incoming, dtype=np.float64), (n,))
    r, t, tdir, rdir, tdd, tau = cloud_layer(*arrs, mu0, scale=scale)
    minus_sec = -1.0 / mu0
    d = np.empty((nlay + 1, n))
    d[0] = mu0 * incoming
    for l in range(nlay):
        d[l + 1] = d[l] * np.exp(minus_sec * tau[l])
    a, s = np.empty((nlay + 1, n)), np.empty((nlay + 1, n))
    a[nlay] = albedo
    s[nlay] = albedo * d[nlay]
    for l in range(nlay - 1, -1, -1):
        inv = 1.0 / (1.0 - a[l + 1] * r[l])
        a[l] = r[l] + t[l] * t[l] * a[l + 1] * inv
        s[l] = rdir[l] * d[l] + t[l] * (s[l + 1] + a[l + 1] * tdd[l] * d[l]) * inv
    dn, up = np.zeros((nlay + 1, n)), np.empty((nlay + 1, n))
    up[0] = s[0]
    for l in range(nlay):
        inv = 1.0 / (1.0 - a[l + 1] * r[l])
        dn[l + 1] = (t[l] * dn[l] + r[l] * s[l + 1] + tdd[l] * d[l]) * inv
        up[l + 1] = a[l + 1] * dn[l + 1] + s[l + 1]
    if one:
        return d[:, 0], dn[:, 0], up[:, 0]
    return d, dn, up


# ------------------------------------------------------------------------------------------------------------- longwave
def lw_fluxes(planck_hl, tau, sec, weight, emissivity=1.0, planck_skin=None):
    """planck_hl (nlay+1, n), tau (nlay, n) (the cloud already added), sec and weight (nsec,) (lw_angle_table: 1.66 and 1, or
    1 / mu and 2 w mu of the Gauss-Legendre nodes), emissivity and planck_skin scalars or (n,) (None: planck_hl[nlay]) ->
    (dn, up), each (nlay+1, n): all angles down, then all angles up from emissivity * planck_skin + (1 - emissivity) * dn[nlay]."""
    pl, tau = np.asarray(planck_hl, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    nlay, n = tau.shape
    dn, up = np.zeros((nlay + 1, n)), np.zeros((nlay + 1, n))
    terms = []
    for s in sec:
        with np.errstate(all="ignore"):
            e = 1.0 - np.exp(-s * tau)
            fac = np.where(e > 1.0e-5, 1.0 - e * (1.0 / s) / np.where(tau > 0.0, tau, 1.0), 0.5 * e)
        terms.append((e, fac))
    for (e, fac), w in zip(terms, weight):
        f = np.zeros(n)
        for l in range(nlay):
            f = f * (1.0 - e[l]) + pl[l] * (e[l] - fac[l]) + pl[l + 1] * fac[l]
            dn[l + 1] += w * f
    skin = pl[nlay] if planck_skin is None else planck_skin
    surface = emissivity * skin + (1.0 - emissivity) * dn[nlay]
    for (e, fac), w in zip(terms, weight):
        f = surface
        up[nlay] += w * f
        for l in range(nlay - 1, -1, -1):
            f = f * (1.0 - e[l]) + pl[l + 1] * (e[l] - fac[l]) + pl[l] * fac[l]
            up[l] += w * f
    return dn, up
