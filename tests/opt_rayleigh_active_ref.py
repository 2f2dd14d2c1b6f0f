"""The references of the optimiser with optimised Rayleigh coefficients (ECCKD_OPT_RAYLEIGH_ACTIVE; a helper module, not a
conftest).

The state carries ng more elements x = ln(rayleigh_molar_scattering[g]) behind the active gases' elements.  Both references
take the Rayleigh coefficients from that tail, carry it in x0 and add 0.5 sum d^2 / sigma^2 (d = x - x0 on the unpinned tail
elements, sigma = ray_sigma > 0) in cost_prior:

  PlainActive      ckd_synth.OracleSW: the C oracle's cost, Rayleigh one more absorber added before the clamp
  ScatteringActive opt_rayleigh_ref.OracleRayleigh: the numpy two-stream cost, tau_ray beside tau_abs after the clamp

Neither has a gradient of its own for the tail: the tests difference these costs.
"""
import numpy as np

import ckd_synth
import opt_rayleigh_ref as orr

MIN_X = -1.0e20


class _Tail:
    """What both references share: the tail of the state and its prior."""

    def _init_base(self, cls, pyoracle, model, scenes, cfg, **kw):
        if any(g.get("active", True) for g in model["gases"]):
            cls.__init__(self, pyoracle, model, scenes, cfg, **kw)
            return
        # Rayleigh alone.  Oracle.__init__ concatenates the active gases' states and needs one for that: it is given the
        # first gas, and what it derived from it is emptied again
        cls.__init__(self, pyoracle, dict(model, gases=[dict(g, active=i == 0) for i, g in enumerate(model["gases"])]), scenes, cfg, **kw)
        self.m = dict(self.m, gases=model["gases"])
        self.active, self.sizes, self.x0, self._prior = [], [], np.zeros(0), None

    def _init_tail(self, ray_sigma):
        self.ray_sigma = float(ray_sigma)
        self.ng = int(self.m["ng"])
        self.ngas_x = int(sum(self.sizes))                       # the gases' part of the state
        k = np.asarray(self.m["rayleigh_molar_scattering"], dtype=np.float64)
        self.x0 = np.concatenate([self.x0, ckd_synth.Oracle._logk(k)])
        self.ray_scale = 1.0                                     # layer_terms: tau_ray scaled, for the branch-edge check

    def k_ray(self, x):
        t = np.asarray(x[self.ngas_x:self.ngas_x + self.ng], dtype=np.float64)
        return np.where(t > MIN_X, np.exp(np.minimum(t, 700.0)), 0.0)

    def moles(self, scene):
        p = scene["pressure_hl"]
        return (p[:, 1:] - p[:, :-1]) * orr.MOLES_PER_PA

    def cost_prior(self, x, sigma):
        """the gases' prior (calc_background_cost_function) plus the tail's 0.5 sum d^2 / ray_sigma^2; returns (J, grad)"""
        J, grad = ckd_synth.Oracle.cost_prior(self, x, sigma) if self.ngas_x else (0.0, np.zeros_like(x))
        if self.ray_sigma > 0.0:
            sl = slice(self.ngas_x, self.ngas_x + self.ng)
            d = np.where(self.x0[sl] > MIN_X, x[sl] - self.x0[sl], 0.0)
            J += 0.5 * np.sum(d * d) / self.ray_sigma ** 2
            grad[sl] = d / self.ray_sigma ** 2
        return J, grad


class PlainActive(_Tail, ckd_synth.OracleSW):
    def __init__(self, pyoracle, model, scenes, cfg, ray_sigma=0.0):
        self._init_base(ckd_synth.OracleSW, pyoracle, model, scenes, cfg)
        self._init_tail(ray_sigma)

    def optical_depth(self, x, scene):
        od = ckd_synth.Oracle.optical_depth(self, x, scene)      # the gases alone
        return od + self.moles(scene)[:, :, None] * self.k_ray(x)[None, None, :]


class ScatteringActive(_Tail, orr.OracleRayleigh):
    def __init__(self, pyoracle, model, scenes, cfg, ray_sigma=0.0, hr_from_net=True):
        self._init_base(orr.OracleRayleigh, pyoracle, model, scenes, cfg, hr_from_net=hr_from_net)
        self._init_tail(ray_sigma)
        self._k_now = np.asarray(self.m["rayleigh_molar_scattering"], dtype=np.float64)

    def tau_abs_raw(self, x, scene):
        # every method of OracleRayleigh that needs tau_ray(scene) asks for tau_abs_raw(x, scene) first: the state's
        # coefficients are noted here
        self._k_now = self.k_ray(x)
        return ckd_synth.Oracle.optical_depth(self, x, scene)

    def tau_ray(self, scene):
        return self.ray_scale * self.moles(scene)[:, :, None] * self._k_now[None, None, :]
