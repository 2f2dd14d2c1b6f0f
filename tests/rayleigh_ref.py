"""Two numpy float64 references of the Rayleigh-scattering two-stream shortwave transfer (a helper module, not a conftest).

Levels 0..nlay from the top down; per layer tau = tau_abs + tau_ray, w = tau_ray / tau (0 where tau_ray <= 0 or tau <= 0);
with t the optical depth increasing downwards, U up, V diffuse down, D direct through a horizontal plane:
    dU/dt =  g1 U - g2 V - w g3 D / mu0        g1 = 2 - 1.25 w, g2 = 0.75 w, g3 = g4 = 0.5
    dV/dt =  g2 U - g1 V + w g4 D / mu0        V(0) = 0, D(0) = mu0 * ssi
    dD/dt = -D / mu0                           surface: U = albedo (V + D)

two_stream_exact   holds no closed form: the 3x3 transfer matrix expm(A t) of every sublayer (tau <= 1) from a Taylor series with
                   scaling and squaring, then ONE linear system for U and V at all interfaces with the two boundary conditions
                   (chaining the matrices is unstable).
two_stream_closed  restates the arithmetic of csrc/lbl_rt.hpp (rayleigh_layer, rayleigh_up, rayleigh_down): Meador & Weaver's
                   closed form per layer, the w = 0 branch, the resonance treatment and the two adding sweeps.
"""
import numpy as np

RESONANCE_H = 1.0e-4     # |1 - k mu0| below which the direct-beam terms are interpolated between mu0 = (1 -+ 2h) / k

# Worst absolute difference of two_stream_closed against two_stream_exact per unit mu0 * ssi on the inputs of
# tests/test_rayleigh_ref.py (random columns, the sweep across the resonance, tiny w at mu0 = 0.5), times 10 for a device
# build that contracts and orders sums differently.  Measured: 2.5e-10 on the random columns, 6.2e-9 across the resonance
# (the curvature the linear interpolation over 4h leaves, largest at w = 0.99, tau = 5, where 4h / k is widest in mu0),
# 1.2e-16 at tiny w.
MEASURED_CLOSED_VS_EXACT = 6.2e-9
EXACT_BOUND = 10.0 * MEASURED_CLOSED_VS_EXACT


# ---------------------------------------------------------------------------------------------------------------- exact
def _expm(a):
    """exp of a batch of small matrices (n, 3, 3): Taylor series of a / 2^s, squared s times."""
    a = np.asarray(a, dtype=np.float64)
    norm = np.max(np.sum(np.abs(a), axis=2), axis=1)
    s = np.maximum(0, np.ceil(np.log2(np.maximum(norm, 1e-300) / 0.25))).astype(int)
    x = a / (2.0 ** s)[:, None, None]
    eye = np.broadcast_to(np.eye(a.shape[1]), a.shape)
    out, term = eye.copy(), eye.copy()
    for n in range(1, 20):
        term = term @ x / n
        out = out + term
    for i in range(int(s.max()) if s.size else 0):
        sq = out @ out
        out = np.where((s > i)[:, None, None], sq, out)
    return out


def two_stream_exact(tau_abs, tau_ray, mu0, albedo, incoming=1.0):
    """One column: tau_abs, tau_ray (nlay,), scalars mu0, albedo, incoming (= ssi) -> (direct, diffuse_dn, up), each (nlay+1,)."""
    tau_abs = np.asarray(tau_abs, dtype=np.float64)
    tau_ray = np.asarray(tau_ray, dtype=np.float64)
    nlay = tau_abs.size
    tau = tau_abs + tau_ray
    w = np.where((tau_ray > 0.0) & (tau > 0.0), tau_ray / np.where(tau > 0.0, tau, 1.0), 0.0)
    nsub = np.maximum(1, np.ceil(tau)).astype(int)
    layer = np.repeat(np.arange(nlay), nsub)              # the layer of every sublayer
    t = (tau / nsub)[layer]
    ws = w[layer]
    n = layer.size
    g1, g2 = 2.0 - 1.25 * ws, 0.75 * ws
    a = np.zeros((n, 3, 3))
    a[:, 0, 0], a[:, 0, 1], a[:, 0, 2] = g1, -g2, -ws * 0.5 / mu0
    a[:, 1, 0], a[:, 1, 1], a[:, 1, 2] = g2, -g1, ws * 0.5 / mu0
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
def _direct_terms(w, k, e, e2, f, a1, a2, tau, mu0):
    """Rdir and Tdd of the closed form with mu0 in every place it occurs, Tdir included (before the clamps)."""
    g3 = g4 = 0.5
    km = k * mu0
    tdir = np.exp((-1.0 / mu0) * tau)
    f2 = w * f / (1.0 - km * km)
    rdir = f2 * ((1.0 - km) * (a2 + k * g3) - (1.0 + km) * (a2 - k * g3) * e2 - 2.0 * k * e * (g3 - a2 * mu0) * tdir)
    tdd = f2 * (2.0 * k * e * (g4 + a1 * mu0) - tdir * ((1.0 + km) * (a1 + k * g4) - (1.0 - km) * (a1 - k * g4) * e2))
    return rdir, tdd


def rayleigh_layer(tau_abs, tau_ray, mu0):
    """The layer terms (R, T, Tdir, Rdir, Tdd) per unit direct flux at the layer top; arrays of one shape, mu0 a scalar."""
    tau_abs = np.asarray(tau_abs, dtype=np.float64)
    tau_ray = np.asarray(tau_ray, dtype=np.float64)
    tau = tau_abs + tau_ray
    scat = (tau_ray > 0.0) & (tau > 0.0)
    with np.errstate(all="ignore"):
        w = np.where(scat, tau_ray / np.where(scat, tau, 1.0), 0.5)     # (0.5: a harmless stand-in where the w = 0 branch is taken)
        g3 = g4 = 0.5
        g1, g2 = 2.0 - 1.25 * w, 0.75 * w
        a1 = g1 * g4 + g2 * g3
        a2 = g1 * g3 + g2 * g4
        k = np.sqrt(np.maximum((g1 - g2) * (g1 + g2), 1e-12))
        e = np.exp(-k * tau)
        e2 = e * e
        f = 1.0 / (k + g1 + (k - g1) * e2)
        tdir = np.exp((-1.0 / mu0) * tau)
        r = g2 * (1.0 - e2) * f
        t = 2.0 * k * e * f
        mu = np.full(tau.shape, float(mu0))
        rdir, tdd = _direct_terms(w, k, e, e2, f, a1, a2, tau, mu)
        near = np.abs(1.0 - k * mu0) < RESONANCE_H
        if np.any(near):
            mu_a, mu_b = (1.0 - 2.0 * RESONANCE_H) / k, (1.0 + 2.0 * RESONANCE_H) / k
            ra, ta = _direct_terms(w, k, e, e2, f, a1, a2, tau, mu_a)
            rb, tb = _direct_terms(w, k, e, e2, f, a1, a2, tau, mu_b)
            x = (mu0 - mu_a) / (mu_b - mu_a)
            rdir = np.where(near, ra + (rb - ra) * x, rdir)
            tdd = np.where(near, ta + (tb - ta) * x, tdd)
        rdir = np.minimum(np.maximum(rdir, 0.0), 1.0 - tdir)
        tdd = np.minimum(np.maximum(tdd, 0.0), 1.0 - tdir - rdir)
        zero = np.zeros(tau.shape)
        return (np.where(scat, r, zero), np.where(scat, t, np.exp(-2.0 * tau)), tdir, np.where(scat, rdir, zero),
                np.where(scat, tdd, zero))


def two_stream_closed(tau_abs, tau_ray, mu0, albedo, incoming=1.0):
    """tau_abs, tau_ray (nlay,) or (nlay, n); mu0 a scalar; albedo and incoming (= ssi) scalars or (n,) ->
    (direct, diffuse_dn, up), each (nlay+1,) or (nlay+1, n)."""
    tau_abs = np.asarray(tau_abs, dtype=np.float64)
    tau_ray = np.asarray(tau_ray, dtype=np.float64)
    one = tau_abs.ndim == 1
    if one:
        tau_abs, tau_ray = tau_abs[:, None], tau_ray[:, None]
    nlay, n = tau_abs.shape
    albedo = np.broadcast_to(np.asarray(albedo, dtype=np.float64), (n,))
    incoming = np.broadcast_to(np.asarray(incoming, dtype=np.float64), (n,))
    r, t, tdir, rdir, tdd = rayleigh_layer(tau_abs, tau_ray, mu0)
    minus_sec = -1.0 / mu0
    d = np.empty((nlay + 1, n))
    d[0] = mu0 * incoming
    for l in range(nlay):
        d[l + 1] = d[l] * np.exp(minus_sec * (tau_abs[l] + tau_ray[l]))
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
