"""SHA-256 of everything the optimiser entry points return (csrc/optimize.hip: ecckd_opt_*, ecckd_run_ckd, ecckd_scale_lut), at the
synthetic model's own small shapes: a change that is meant to leave their arithmetic alone is run once on the build before it and
once on the build after it, on the same GPU, and every digest has to be equal.  profiles/opt_digests.json holds the output of the
build it was committed with; a ROCm math-library update may change digests legitimately, which is why this is a tool and not a test.
Models and scenes of tests/ckd_synth.py with fixed seeds; the truth fluxes are fixed-seed arrays (no oracle).  Cases: longwave and
shortwave (Rayleigh on), with boundary terms, with relative-to fluxes, with 70 g points; longwave with an active gas absent from a
scene, with temperature_fl given, without min/max arrays, with the prior's sigma estimated from them, with cap_relative_linear
biting, and with pressure_weight_power 1.0 and 0.7 beside the base's 0.5; the shortwave on a scattering handle
(rayleigh_scattering=True: cost and gradient, both forward passes and the bounded minimiser): base, with boundary terms, with
relative-to fluxes, with 70 g points.  The two base cases also run under ECCKD_K8A_GENERIC=1, ECCKD_K8A_THREADS=128 and
ECCKD_K8B_PLAIN_ORDER=1, the scattering base case under ECCKD_K8A_THREADS=192.  Each setting runs in a child process of its own
(ECCKD_K8B_PLAIN_ORDER is read when a handle is created, the two K8a knobs at every forward launch: a child per setting keeps
the settings apart), one after another, each under its own time limit; a child that fails ends the run.  Prints one JSON object.
usage: python tools/opt_digest.py"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [("default", {}, "all"), ("ECCKD_K8A_GENERIC=1", {"ECCKD_K8A_GENERIC": "1"}, "base"),
            ("ECCKD_K8A_THREADS=128", {"ECCKD_K8A_THREADS": "128"}, "base"),
            ("ECCKD_K8B_PLAIN_ORDER=1", {"ECCKD_K8B_PLAIN_ORDER": "1"}, "base"),
            ("ECCKD_K8A_THREADS=192", {"ECCKD_K8A_THREADS": "192"}, "scattering base")]
SCATTERING = "sw scattering"            # cases whose name starts so run on a scattering handle
CHILD_TIMEOUT_S = 240
CFG = dict(flux_weight=0.2, flux_profile_weight=0.05, broadband_weight=0.4, spectral_boundary_weight=0.0,
           negative_od_penalty=1.0e4, pressure_weight_power=0.5, prior_error=4.0, pressure_corr=0.95,
           temperature_corr=0.95, conc_corr=0.9, cap_relative_linear=0.0)


def child(which):
    import numpy as np
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import ckd_synth
    from ecckd_amd import api

    # api.Optimizer does not pass a scene's temperature_fl on; the C entry takes one
    plain_scene = api._opt_scene

    def scene_with_temperature_fl(sc, s, keep):
        plain_scene(sc, s, keep)
        if s.get("temperature_fl") is not None:
            sc.temperature_fl = api._keep_ptr(keep, api._f64c(s["temperature_fl"]))
    api._opt_scene = scene_with_temperature_fl

    def digest(*items):
        h = hashlib.sha256()
        for a in items:
            h.update(np.ascontiguousarray(a, dtype=None if isinstance(a, np.ndarray) else np.float64).tobytes())
        return h.hexdigest()

    def problem(sw=False, ng=12, nband=3, boundary=False, relative=False, **cfg):
        model = (ckd_synth.make_model_sw if sw else ckd_synth.make_model)(seed=3, ng=ng, nband=nband)
        albedo = np.linspace(0.3, 0.06, nband)
        scenes = ckd_synth.make_scenes_sw(model, albedo, ch4_low=True) if sw else ckd_synth.make_scenes(model, ch4_low=True)
        rs = np.random.RandomState(17)
        for s in scenes:
            ncol, nhl = s["pressure_hl"].shape
            s["flux_dn"], s["flux_up"] = rs.uniform(50.0, 150.0, (ncol, nhl, nband)), rs.uniform(50.0, 150.0, (ncol, nhl, nband))
            if boundary:
                s["spectral_flux_dn_surf"] = rs.uniform(5.0, 15.0, (ncol, ng))
                if sw:
                    s["spectral_boundary_weights"] = 0.02 * rs.uniform(size=ng)
                else:
                    s["spectral_flux_up_toa"] = rs.uniform(5.0, 15.0, (ncol, ng))
            if relative:
                s["relative_flux_dn"], s["relative_flux_up"] = rs.uniform(1.0, 9.0, (ncol, nhl, ng)), rs.uniform(1.0, 9.0, (ncol, nhl, ng))
        return model, scenes, dict(CFG, **cfg)

    def lw_gas_absent():
        model, scenes, cfg = problem()
        scenes[0]["gas_present"][2] = 0
        return model, scenes, cfg

    def lw_temperature_fl():
        model, scenes, cfg = problem()
        for s in scenes:
            s["temperature_fl"] = 0.5 * (s["temperature_hl"][:, 1:] + s["temperature_hl"][:, :-1]) + 1.5
        return model, scenes, cfg

    def lw_unbounded():
        model, scenes, cfg = problem()
        for g in model["gases"]:
            g["min_molar_abs"] = g["max_molar_abs"] = None
        return model, scenes, cfg

    def lw_cap():
        model, scenes, cfg = problem(cap_relative_linear=0.8)
        for k in ("molar_abs", "min_molar_abs", "max_molar_abs"):      # strong enough for the cap to bite
            model["gases"][3][k] = model["gases"][3][k] * 10.0
        return model, scenes, cfg

    cases = {"lw": problem, "sw": lambda: problem(sw=True)}
    if which == "scattering base":
        cases = {SCATTERING: lambda: problem(sw=True)}
    if which == "all":
        cases.update({
            "lw boundary": lambda: problem(boundary=True, spectral_boundary_weight=0.3), "sw boundary": lambda: problem(sw=True, boundary=True),
            "lw relative": lambda: problem(relative=True), "sw relative": lambda: problem(sw=True, relative=True),
            "lw ng=70": lambda: problem(ng=70, nband=5), "sw ng=70": lambda: problem(sw=True, ng=70, nband=5),
            "lw gas absent": lw_gas_absent, "lw temperature_fl": lw_temperature_fl, "lw unbounded": lw_unbounded,
            "lw estimated sigma": lambda: problem(prior_error=-1.0, min_prior_error=0.5, max_prior_error=3.0, prior_error_scaling=1.0),
            "lw cap_relative_linear": lw_cap,
            "lw pressure_weight_power=1.0": lambda: problem(pressure_weight_power=1.0),
            "lw pressure_weight_power=0.7": lambda: problem(pressure_weight_power=0.7),
            SCATTERING: lambda: problem(sw=True), SCATTERING + " boundary": lambda: problem(sw=True, boundary=True),
            SCATTERING + " relative": lambda: problem(sw=True, relative=True),
            SCATTERING + " ng=70": lambda: problem(sw=True, ng=70, nband=5)})
    out = {}
    with api.Context(0) as ctx:
        for name, make in cases.items():
            model, scenes, cfg = make()
            d = out[name] = {}
            scattering = name.startswith(SCATTERING)
            opt = api.Optimizer(ctx, model, scenes, rayleigh_scattering=scattering, **cfg)
            x0, lo, hi = opt.initial_state(bounds=True)
            if not scattering:
                d["initial state and bounds"] = digest(x0, lo, hi)
            rs = np.random.RandomState(8)
            x = x0 + np.where(x0 > -1.0e20, 0.2 * rs.normal(size=x0.size), 0.0)
            sizes = np.cumsum([0] + [g["molar_abs"].size for g in model["gases"] if g["active"]])
            x[sizes[3]:sizes[4]] += 9.0                          # negative optical depths: penalty and clamp
            d["forward"] = digest(*opt.forward(x))
            d["forward unclamped"] = digest(*opt.forward(x, unclamped=True))
            d["cost and gradient"] = digest(*opt.cost_grad(x))
            if not scattering:
                d["coefficients"] = digest(*[opt.coefficients(x, i, g["molar_abs"].shape) for i, g in enumerate(model["gases"])])
            for bounded in ((True,) if scattering else (True, False)):
                r = opt.minimize(max_iterations=30, convergence_criterion=0.0, bounded=bounded)
                d[f"minimize bounded={bounded}"] = digest(r["x"], r["status"], r["iterations"], r["cost"], r["gradient_norm"])
                d[f"minimize bounded={bounded} (status, iterations)"] = [r["status"], r["iterations"]]
            opt.close()
            if scattering:                                       # what follows makes no scattering handle
                continue
            r = api.run_ckd(ctx, model, scenes[0])
            d["run_ckd"] = digest(*[r[k] for k in sorted(r)])
            s = scenes[0]
            nz, ng = s["pressure_hl"].shape[1] - 1, len(model["iband_per_g"])
            flux_sums = np.cumprod(np.random.RandomState(5).uniform(0.6, 1.0, (nz + 1, ng)), axis=0)
            flux_sums[-2:, 0] = 0.0                              # a g point that is dark at the surface
            coeffs, scaling = api.scale_lut(ctx, model, flux_sums, s["pressure_hl"][0], s["temperature_hl"][0], s["vmr_fl"][0],
                                            s["gas_present"], 0.6)
            d["scale_lut"] = digest(scaling, *coeffs)
    print(json.dumps(out))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    out = {}
    for name, env, which in SETTINGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], env=dict(os.environ, **env),
                           stdout=subprocess.PIPE, timeout=CHILD_TIMEOUT_S)
        if r.returncode != 0:
            sys.exit(f"opt_digest: the run under {name} ended with status {r.returncode}; nothing more is started")
        out[name] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
