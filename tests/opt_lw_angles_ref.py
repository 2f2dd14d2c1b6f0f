"""The numpy float64 reference of the optimiser's longwave cost under the zenith-angle quadrature (a helper module, not a
conftest).

OracleLwAngles subclasses ckd_synth.Oracle: the look-up of the optical depth stays the C oracle's, everything after it is numpy.
The transfer is the one `optimize_lut nangle=N` trains under, written per angle from arrays sec / wgt:
    eps_k = 1 - exp(-sec_k tau),  fac_k = eps_k > 1e-5 ? 1 - eps_k / (sec_k tau) : eps_k / 2
    dn_k[l+1] = dn_k[l] (1 - eps_k) + B_l (eps_k - fac_k) + B_l+1 fac_k,  dn = sum_k wgt_k dn_k
    up_k[nlay] = es B_nlay + (1 - es) dn[nlay],  up_k[l] = up_k[l+1] (1 - eps_k) + B_l+1 (eps_k - fac_k) + B_l fac_k
and the cost is calc_cost_function_ckd_lw (calc_cost_function_lw.cpp:116-232) written out.  With the single angle sec = [1.66],
wgt = [1] the whole is the reference's two-stream cost, which pins the restatement against the C oracle's
(tests/test_opt_lw_angles_ref.py).
"""
import numpy as np

import ckd_synth
from opt_rayleigh_ref import COST_REL_TOL, HR_WEIGHT, heating_rate  # noqa: F401

THIN_EPS = 1.0e-5                                                    # radiative_transfer_lw.cpp:42


def nodes(nangle):
    """sec_k = 1 / mu_k, wgt_k = 2 w_k mu_k of the nangle-point Gauss-Legendre rule in mu on (0, 1), mu ascending"""
    x, w = np.polynomial.legendre.leggauss(int(nangle))
    mu, w = 0.5 * (x + 1.0), 0.5 * w
    return 1.0 / mu, 2.0 * w * mu


def layer_terms(od, sec):
    """eps, fac of every (angle, cell): od (..., ) -> two arrays (nang, ...)"""
    sec = np.asarray(sec, dtype=np.float64).reshape((-1,) + (1,) * od.ndim)
    path = sec * od[None]
    eps = 1.0 - np.exp(-path)
    thick = eps > THIN_EPS
    fac = np.where(thick, 1.0 - eps / np.where(thick, path, 1.0), 0.5 * eps)
    return eps, fac


def transfer(planck, od, es_g, sec, wgt):
    """planck (nhl, ng), od (nlay, ng), es_g (ng,) -> dn, up (nhl, ng), summed over the angles in angle order"""
    nlay, ng = od.shape
    eps, fac = layer_terms(od, sec)
    nang = eps.shape[0]
    dn_k = np.zeros((nang, nlay + 1, ng))
    for l in range(nlay):
        dn_k[:, l + 1] = dn_k[:, l] * (1.0 - eps[:, l]) + planck[l] * (eps[:, l] - fac[:, l]) + planck[l + 1] * fac[:, l]
    dn = np.zeros((nlay + 1, ng))
    for k in range(nang):
        dn += wgt[k] * dn_k[k]
    up_k = np.zeros((nang, nlay + 1, ng))
    up_k[:, nlay] = es_g * planck[nlay] + (1.0 - es_g) * dn[nlay]      # Lambertian: the angle-summed flux is reflected
    for l in range(nlay - 1, -1, -1):
        up_k[:, l] = up_k[:, l + 1] * (1.0 - eps[:, l]) + planck[l + 1] * (eps[:, l] - fac[:, l]) + planck[l] * fac[:, l]
    up = np.zeros((nlay + 1, ng))
    for k in range(nang):
        up += wgt[k] * up_k[k]
    return dn, up


def profile_cost(cfg, p, lw, ib, nband, fdn_g, fup_g, flux_dn, flux_up, hr_true, sfd=None, sfu=None, rel_dn=None, rel_up=None):
    """calc_cost_function_lw.cpp:161-231 for one profile from its per-g fluxes (nhl, ng)"""
    if rel_dn is not None:                                           # :162-165
        fdn_g = fdn_g - rel_dn
        fup_g = fup_g - rel_up
    nhl = fdn_g.shape[0]
    nlay = nhl - 1
    fdn = np.zeros((nhl, nband))
    fup = np.zeros((nhl, nband))
    for g in range(fdn_g.shape[1]):                                  # g order, as the device sums
        fdn[:, ib[g]] += fdn_g[:, g]
        fup[:, ib[g]] += fup_g[:, g]
    hrf = heating_rate(p, fdn, fup)
    fw, fpw, bbw, sbw = cfg["flux_weight"], cfg["flux_profile_weight"], cfg["broadband_weight"], cfg["spectral_boundary_weight"]
    iw = fpw * 0.5 * (lw[:-1] + lw[1:]) if nlay > 1 else np.zeros(0)   # :193
    dres = hrf - hr_true
    dd, du = fdn - flux_dn, fup - flux_up
    cost = 0.0
    for b in range(nband):                                           # :195-206
        cost += HR_WEIGHT * HR_WEIGHT * np.sum(lw * dres[:, b] ** 2) + fw * (dd[nlay, b] ** 2 + du[0, b] ** 2)
        if fpw > 0.0:
            cost += np.sum(iw * (dd[1:nlay, b] ** 2 + du[1:nlay, b] ** 2))
    cost = ((cost * (1.0 - bbw)) / nband + bbw * HR_WEIGHT * HR_WEIGHT * np.sum(lw * dres.sum(axis=1) ** 2)
            + bbw * fw * (dd[nlay].sum() ** 2 + du[0].sum() ** 2))   # :209-213
    if fpw > 0.0:                                                    # :216-221
        cost += bbw * np.sum(iw * (dd[1:nlay].sum(axis=1) ** 2 + du[1:nlay].sum(axis=1) ** 2))
    if sbw > 0.0 and sfd is not None and sfu is not None:            # :223-229
        cost += sbw * np.sum((fdn_g[nlay] - sfd) ** 2 + (fup_g[0] - sfu) ** 2)
    return cost


class OracleLwAngles(ckd_synth.Oracle):
    def __init__(self, pyoracle, model, scenes, cfg, sec, wgt):
        super().__init__(pyoracle, model, scenes, cfg)
        self.sec, self.wgt = np.asarray(sec, dtype=np.float64), np.asarray(wgt, dtype=np.float64)

    def emissivity_g(self, scene, c):
        es = scene.get("surf_emissivity")
        ng = self.m["planck_function"].shape[1]
        return np.ones(ng) if es is None else np.asarray(es, dtype=np.float64)[c][self.m["iband_per_g"]]

    def gas_optical_depths(self, x, scene):
        """(total, sum of the gases' absolute values), each (ncol, nlay, ng): how far a cell is from changing its sign"""
        total = abs_sum = None
        for i in range(len(self.m["gases"])):
            only = dict(self.m, gases=[g if j == i else dict(g, molar_abs=0.0 * g["molar_abs"]) for j, g in enumerate(self.m["gases"])])
            one = OracleLwAngles(self.o, only, self.scenes, self.cfg, self.sec, self.wgt)
            od = ckd_synth.Oracle.optical_depth(one, self._x_of(one, x, i), scene)
            total = od if total is None else total + od
            abs_sum = np.abs(od) if abs_sum is None else abs_sum + np.abs(od)
        return total, abs_sum

    def _x_of(self, other, x, keep):
        """the state of `other` (whose gases but `keep` are zero): x where the gas is `keep`, pinned elsewhere"""
        out = np.full_like(x, -1.0e20)
        off = 0
        for i, n in zip(self.active, self.sizes):
            if i == keep:
                out[off:off + n] = x[off:off + n]
            off += n
        return out

    def fluxes(self, x, scene, unclamped=False):
        od = self.optical_depth(x, scene)
        if not unclamped:
            od = np.maximum(od, 0.0)
        T = scene["temperature_hl"]
        ncol, nhl = T.shape
        out = np.empty((ncol, 2, nhl, od.shape[2]))
        for c in range(ncol):
            out[c, 0], out[c, 1] = transfer(self.planck(T[c]), od[c], self.emissivity_g(scene, c), self.sec, self.wgt)
        return out

    def band_fluxes(self, x, scene):
        f = self.fluxes(x, scene)
        ib = self.m["iband_per_g"]
        return np.stack([f[:, :, :, ib == b].sum(-1) for b in range(self.m["nband"])], axis=-1)

    def cost_rt(self, x):
        cfg = self.cfg
        J = 0.0
        nband = self.m["nband"]
        ib = np.asarray(self.m["iband_per_g"])
        for scene in self.scenes:
            od = self.optical_depth(x, scene)
            neg = od < 0.0
            if neg.any():                                            # solve_adept.cpp:107-116
                J += cfg["negative_od_penalty"] * np.sum(od[neg] ** 2)
            fl = self.fluxes(x, scene)
            p = scene["pressure_hl"]
            sfd, sfu = scene.get("spectral_flux_dn_surf"), scene.get("spectral_flux_up_toa")
            rd, ru = scene.get("relative_flux_dn"), scene.get("relative_flux_up")
            for c in range(p.shape[0]):
                pw = cfg["pressure_weight_power"]
                lw = (np.sqrt(p[c, 1:]) - np.sqrt(p[c, :-1])) if pw == 0.5 else (p[c, 1:] ** pw - p[c, :-1] ** pw)
                lw = lw / lw.sum()
                fd, fu = scene["flux_dn"][c], scene["flux_up"][c]
                J += profile_cost(cfg, p[c], lw, ib, nband, fl[c, 0], fl[c, 1], fd, fu, heating_rate(p[c], fd, fu),
                                  sfd[c] if sfd is not None else None, sfu[c] if sfu is not None else None,
                                  rd[c] if rd is not None else None, ru[c] if ru is not None else None)
        return float(J)
