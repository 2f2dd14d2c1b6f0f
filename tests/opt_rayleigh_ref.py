"""The numpy float64 reference of the optimiser's Rayleigh-scattering shortwave cost (a helper module, not a conftest).

OracleRayleigh subclasses ckd_synth.OracleSW: the look-up of the gas optical depth stays the C oracle's, everything after it is
numpy.  tau_abs is that optical depth after the clamp at zero, tau_ray = moles_per_layer * rayleigh_molar_scattering, the
transfer is rayleigh_ref.two_stream_closed and the cost is calc_cost_function_sw.cpp:116-277 written out, fed with the total
downwelling D + V and the upwelling U.  `hr_from_net` switches the heating rate between the direct-beam one of the reference
(False: flux_dn alone, the truth's from the scene's flux_dn alone) and the net-flux one of a scattering handle (True: dn - up
on both sides).  With rayleigh_molar_scattering = 0 and hr_from_net=False the whole is the reference's no-scattering cost, which
pins the restated cost against the C oracle's (tests/test_opt_rayleigh_ref.py).
"""
import numpy as np

import ckd_synth
import rayleigh_ref

MOLES_PER_PA = 1.0 / (9.80665 * 0.001 * 28.970)            # ckd_model.h:246-247
HR_WEIGHT = 3600.0 * 24.0

# The cost of tests/test_optimize_rayleigh_gpu.py is held to the rel = 1e-10 of test_sw_cost_and_gradient: the scattering
# arithmetic keeps it (the device differed from this reference by 1.0e-13 ... 1.2e-12, relative, over the problems of that
# file on an MI355X).  For the record, this reference's own sensitivity - `cost_sensitivity` below, the cost with band sums,
# residuals and weights in float64 against np.longdouble on the same fluxes - is at most 3.8e-13 over the same problems.
COST_REL_TOL = 1.0e-10
MEASURED_COST_F64_VS_LONGDOUBLE = 3.8e-13


def heating_rate(p, dn, up=None):
    """heating_rate.h:30-50 per band: p (nhl,), dn / up (nhl, nband) -> (nlay, nband)"""
    conv = -(9.80665 / 1004.0) / (p[1:] - p[:-1])
    net = dn if up is None else dn - up
    return conv[:, None] * (net[1:] - net[:-1])


def profile_cost(cfg, p, lw, ib, nband, albedo, fdn_g, fup_g, flux_dn, flux_up, hr_true, hr_from_net, sfd=None, sbw=None,
                 rel_dn=None, rel_up=None, dtype=np.float64):
    """calc_cost_function_sw.cpp:116-277 for one profile from its per-g fluxes (nhl, ng)"""
    fdn_g = np.asarray(fdn_g, dtype=dtype)
    fup_g = np.asarray(fup_g, dtype=dtype)
    if rel_dn is not None:                                           # :160-163
        fdn_g = fdn_g - rel_dn
        fup_g = fup_g - rel_up
    nhl = fdn_g.shape[0]
    nlay = nhl - 1
    fdn = np.zeros((nhl, nband), dtype=dtype)
    fup = np.zeros((nhl, nband), dtype=dtype)
    for g in range(fdn_g.shape[1]):                                  # g order, as the device sums
        fdn[:, ib[g]] += fdn_g[:, g]
        fup[:, ib[g]] += fup_g[:, g]
    hrf = heating_rate(p.astype(dtype), fdn, fup if hr_from_net else None)
    all_pos = bool(np.all(albedo > 0.0))
    fw, fpw, bbw = cfg["flux_weight"], cfg["flux_profile_weight"], cfg["broadband_weight"]
    iw = fpw * 0.5 * (lw[:-1] + lw[1:]) if nlay > 1 else np.zeros(0)
    dres = hrf - hr_true
    dd, du = fdn - flux_dn, fup - flux_up
    cost = dtype(0.0)
    for b in range(nband):
        local = HR_WEIGHT * HR_WEIGHT * np.sum(lw * dres[:, b] ** 2) + fw * (dd[nlay, b] ** 2 + 20.0 * du[0, b] ** 2)   # :214
        if fpw > 0.0:
            local += np.sum(iw * (dd[1:nlay, b] ** 2 + du[1:nlay, b] ** 2))
        cost += local
    if bbw > 0.0:                                                    # :243
        cost = (cost * (1.0 - bbw)) / nband + bbw * HR_WEIGHT * HR_WEIGHT * np.sum(lw * dres.sum(axis=1) ** 2)
        cost += bbw * fw * dd[nlay].sum() ** 2
        if all_pos:                                                  # :252
            cost += bbw * fw * du[0].sum() ** 2
        if fpw > 0.0:
            cost += bbw * np.sum(iw * dd[1:nlay].sum(axis=1) ** 2)
            if all_pos:                                              # :264
                cost += bbw * np.sum(iw * du[1:nlay].sum(axis=1) ** 2)
    if sbw is not None and sfd is not None:                          # :271-274
        cost += np.sum(sbw * (fdn_g[nlay] - sfd) ** 2)
    return cost


class OracleRayleigh(ckd_synth.OracleSW):
    def __init__(self, pyoracle, model, scenes, cfg, hr_from_net=True):
        super().__init__(pyoracle, model, scenes, cfg)
        self.hr_from_net = hr_from_net

    def tau_abs_raw(self, x, scene):
        """the gas optical depth as it comes out of the tables (ncol, nlay, ng), negative cells included"""
        return ckd_synth.Oracle.optical_depth(self, x, scene)

    def tau_ray(self, scene):
        p = scene["pressure_hl"]
        moles = (p[:, 1:] - p[:, :-1]) * MOLES_PER_PA
        return moles[:, :, None] * np.asarray(self.m["rayleigh_molar_scattering"], dtype=np.float64)[None, None, :]

    def albedo_g(self, scene):
        return np.maximum(np.asarray(scene["albedo"], dtype=np.float64), 0.0)[self.m["iband_per_g"]]

    def fluxes3(self, x, scene):
        """(direct, diffuse dn, up), each (ncol, nhl, ng), of the scattering transfer on the clamped gas optical depth"""
        ta = np.maximum(self.tau_abs_raw(x, scene), 0.0)
        tr = self.tau_ray(scene)
        ncol, nlay, ng = ta.shape
        out = np.empty((3, ncol, nlay + 1, ng))
        alb, ssi = self.albedo_g(scene), self.ssi(scene)
        for c in range(ncol):
            out[0, c], out[1, c], out[2, c] = rayleigh_ref.two_stream_closed(ta[c], tr[c], float(scene["mu0"][c]), alb, ssi)
        return out

    def fluxes(self, x, scene):
        """(ncol, 2, nhl, ng): total downwelling and upwelling, what ecckd_opt_forward returns for a scattering handle"""
        d, v, u = self.fluxes3(x, scene)
        return np.ascontiguousarray(np.stack([d + v, u], axis=1))

    def layer_terms(self, x, scene, scale=1.0):
        """The quantities that decide rayleigh_layer's branches, per cell, at scale * tau_abs: dict of (ncol, nlay, ng) arrays
        scat (the scattering branch is taken), w, k, km = k mu0, and branch = (inside the resonance band, state of the Rdir
        clamp, state of the Tdd clamp), a clamp's state being -1 below 0, 0 unclamped, 1 at its upper bound"""
        ta = scale * np.maximum(self.tau_abs_raw(x, scene), 0.0)
        tr = self.tau_ray(scene)
        tau = ta + tr
        scat = (tr > 0.0) & (tau > 0.0)
        w = np.where(scat, tr / np.where(scat, tau, 1.0), 0.5)
        g1, g2 = 2.0 - 1.25 * w, 0.75 * w
        a1 = a2 = 0.5 * g1 + 0.5 * g2
        k = np.sqrt(np.maximum((g1 - g2) * (g1 + g2), 1e-12))
        e = np.exp(-k * tau)
        f = 1.0 / (k + g1 + (k - g1) * e * e)
        mu0 = np.broadcast_to(np.asarray(scene["mu0"], dtype=np.float64)[:, None, None], tau.shape)
        tdir = np.exp(-tau / mu0)
        rdir, tdd = rayleigh_ref._direct_terms(w, k, e, e * e, f, a1, a2, tau, mu0)
        inside = np.abs(1.0 - k * mu0) < rayleigh_ref.RESONANCE_H
        if np.any(inside):                                           # there the clamps act on the interpolated terms
            h = rayleigh_ref.RESONANCE_H
            mu_a, mu_b = (1.0 - 2.0 * h) / k, (1.0 + 2.0 * h) / k
            ra, ta_ = rayleigh_ref._direct_terms(w, k, e, e * e, f, a1, a2, tau, mu_a)
            rb, tb_ = rayleigh_ref._direct_terms(w, k, e, e * e, f, a1, a2, tau, mu_b)
            xi = (mu0 - mu_a) / (mu_b - mu_a)
            rdir = np.where(inside, ra + (rb - ra) * xi, rdir)
            tdd = np.where(inside, ta_ + (tb_ - ta_) * xi, tdd)
        state = lambda raw, hi: np.where(raw < 0.0, -1, np.where(raw > hi, 1, 0))
        s_r = state(rdir, 1.0 - tdir)
        r_c = np.minimum(np.maximum(rdir, 0.0), 1.0 - tdir)
        s_t = state(tdd, 1.0 - tdir - r_c)
        z = np.zeros(tau.shape, dtype=int)
        return dict(scat=scat, w=np.where(scat, w, 0.0), k=k, km=k * mu0,
                    branch=np.stack([np.where(scat, inside, z), np.where(scat, s_r, z), np.where(scat, s_t, z)]))

    def cost_rt(self, x, dtype=np.float64):
        cfg = self.cfg
        J = dtype(0.0)
        nband = self.m["nband"]
        ib = np.asarray(self.m["iband_per_g"])
        for scene in self.scenes:
            od = self.tau_abs_raw(x, scene)                          # the clamp acts on the gases alone, Rayleigh is added after it
            neg = od < 0.0
            if neg.any():                                            # solve_adept.cpp:107-116
                J += cfg["negative_od_penalty"] * np.sum(od[neg] ** 2)
            fl = self.fluxes(x, scene)
            p = scene["pressure_hl"]
            albedo = np.asarray(scene["albedo"], dtype=np.float64)
            sfd, sbw = scene.get("spectral_flux_dn_surf"), scene.get("spectral_boundary_weights")
            rd, ru = scene.get("relative_flux_dn"), scene.get("relative_flux_up")
            for c in range(p.shape[0]):
                pw = cfg["pressure_weight_power"]
                lw = (np.sqrt(p[c, 1:]) - np.sqrt(p[c, :-1])) if pw == 0.5 else (p[c, 1:] ** pw - p[c, :-1] ** pw)
                lw = lw / lw.sum()
                fd, fu = scene["flux_dn"][c], scene["flux_up"][c]
                hr_true = heating_rate(p[c], fd, fu if self.hr_from_net else None)
                J += profile_cost(cfg, p[c], lw, ib, nband, albedo, fl[c, 0], fl[c, 1], fd, fu, hr_true, self.hr_from_net,
                                  sfd[c] if (sfd is not None and sbw is not None) else None, sbw,
                                  rd[c] if rd is not None else None, ru[c] if ru is not None else None, dtype=dtype)
        return float(J) if dtype is np.float64 else J

    def cost_sensitivity(self, x):
        """relative difference of the float64 cost and the one whose band sums, residuals and weights run in np.longdouble"""
        a, b = self.cost_rt(x), self.cost_rt(x, dtype=np.longdouble)
        return float(abs(np.longdouble(a) - b) / abs(b))
