"""L-BFGS iterations per second of a scattering optimiser handle (api.Optimizer(rayleigh_scattering=True),
k_opt_forward_adjoint_rayleigh) and of a plain shortwave handle on the same machine and in the same run, at the shortwave
optimiser shape of bench.py --full: ng = 64, 6 x 53 (T, p) grid, 12 mole fractions, 13 bands, 8 scenarios x 50 columns x three
zenith angles x 54 layers.  Each handle is trained on the fluxes of a perturbed model through its own transfer.  Then both
again with the Rayleigh coefficients optimised too (optimize_rayleigh=True, prior error 1: 64 more state elements, two more
launches per evaluation).  Writes profiles/opt_rayleigh_probe.json and prints it.
usage: python tools/opt_rayleigh_probe.py [iterations]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ecckd_amd import api, synthetic as syn  # noqa: E402

iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 60
NBAND, MU0 = 13, (1.0, 0.5, 0.1)


def sw_model(seed):
    m = syn.ckd_model(ng=64, nt=6, np_=53, nband=NBAND, seed=seed, nconc=12)
    rs = np.random.RandomState(seed + 99)
    ssi = rs.uniform(0.5, 1.5, 64)
    m.update(solar_irradiance=1340.0 * ssi / ssi.sum(), rayleigh_molar_scattering=10.0 ** rs.uniform(-7.0, -5.5, 64),
             planck_function=None, temperature_planck=None)
    for g in m["gases"]:                                     # shortwave gases absorb less strongly
        for k in ("molar_abs", "min_molar_abs", "max_molar_abs"):
            g[k] = g[k] * 0.002
    return m


def problem():
    model, truth = sw_model(11), sw_model(11)
    rs = np.random.RandomState(12)
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    rep = lambda a: np.ascontiguousarray(np.repeat(a, len(MU0), axis=0))
    scenes = [dict(pressure_hl=rep(s["pressure_hl"]), temperature_hl=rep(s["temperature_hl"]), vmr_fl=rep(s["vmr_fl"]),
                   gas_present=s["gas_present"], mu0=np.tile(np.asarray(MU0), s["pressure_hl"].shape[0]), tsi=1361.0,
                   albedo=np.full(NBAND, 0.15)) for s in syn.ckd_scenes(model, nscene=8, ncol=50, nlay=54, seed=13)]
    return model, truth, scenes


def run(ctx, scattering, active=False):
    model, truth, scenes = problem()
    cfg = dict(flux_weight=0.2, flux_profile_weight=0.0, broadband_weight=0.5, prior_error=2.0, pressure_corr=0.8,
               temperature_corr=0.8, conc_corr=0.8)
    ib = model["iband_per_g"]
    for s in scenes:
        ncs, nhl = s["pressure_hl"].shape
        s["flux_dn"] = s["flux_up"] = np.zeros((ncs, nhl, NBAND))
    t_opt = api.Optimizer(ctx, truth, scenes, rayleigh_scattering=scattering, **cfg)
    _, fl = t_opt.forward(t_opt.initial_state())
    t_opt.close()
    band = np.stack([fl[..., ib == b].sum(-1) for b in range(NBAND)], axis=-1)
    c0 = 0
    for s in scenes:
        ncs = s["pressure_hl"].shape[0]
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(band[c0:c0 + ncs, 0]), np.ascontiguousarray(band[c0:c0 + ncs, 1])
        c0 += ncs
    extra = dict(optimize_rayleigh=True, rayleigh_prior_error=1.0) if active else {}
    opt = api.Optimizer(ctx, model, scenes, rayleigh_scattering=scattering, **extra, **cfg)
    x0 = opt.initial_state()
    J0, _ = opt.cost_grad(x0)                                # warm-up
    t0 = time.perf_counter()
    for _ in range(20):
        opt.cost_grad(x0)
    eval_ms = (time.perf_counter() - t0) / 20 * 1e3
    t0 = time.perf_counter()
    res = opt.minimize(max_iterations=iterations, convergence_criterion=0.0, bounded=True)
    dt = time.perf_counter() - t0
    out = dict(iters_per_s=res["iterations"] / dt, iterations=res["iterations"], cost_grad_ms=eval_ms, J0=J0, J_final=res["cost"],
               status=res["status"], nx=opt.nx, plan=opt.forward_plan())
    if active:
        out["rayleigh_plan"] = opt.rayleigh_plan()
    opt.close()
    return out


with api.Context(0) as ctx:
    result = {"shape": "ng 64, nlay 54, nband 13, 8 x 150 columns", "iterations_asked": iterations,
              "plain_shortwave": run(ctx, False), "rayleigh_scattering": run(ctx, True),
              "plain_shortwave_optimize_rayleigh": run(ctx, False, True), "rayleigh_scattering_optimize_rayleigh": run(ctx, True, True)}
result["ratio_scattering_to_plain"] = result["rayleigh_scattering"]["iters_per_s"] / result["plain_shortwave"]["iters_per_s"]
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "opt_rayleigh_probe.json"), "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
