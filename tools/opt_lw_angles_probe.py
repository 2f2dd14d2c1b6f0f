"""L-BFGS iterations per second and forward-kernel time of the longwave optimiser under the zenith-angle quadrature
(api.Optimizer(nangle=N), k_opt_forward_adjoint_lw_angles) against the two-stream handle, at the longwave optimiser shape of
bench.py --full: ng = 64, 6 x 53 (T, p) grid, 12 mole fractions (nx ~ 3e5), 13 bands, 8 scenarios x 50 columns x 54 layers.
Each handle is trained on the fluxes of a perturbed model through its own transfer.  Every configuration runs in a process of
its own, one at a time, the configurations alternating over `rounds` rounds, so that drift of the machine shows as spread
within a configuration and not as a difference between two.  In each process: one warm-up evaluation, 20 timed evaluations
(host clock), `repeats` minimisations of `iterations` L-BFGS iterations from the first guess, then 20 evaluations with the
handle's device events on: the time of the forward kernel alone.
--parent DIR: also time nangle = 0 with the package found under DIR (a checkout of the parent commit, built), in the same rounds.
Writes profiles/opt_lw_angles_probe.json and prints it.
usage: python tools/opt_lw_angles_probe.py [--iterations 100] [--rounds 3] [--repeats 3] [--parent DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBAND = 13


def child(args):
    sys.path.insert(0, args.root)
    import numpy as np
    from ecckd_amd import api, synthetic as syn
    kw = dict(nangle=args.nangle) if args.nangle > 0 else {}          # (the parent's Optimizer has no such argument)
    model = syn.ckd_model(ng=64, nt=6, np_=53, nband=NBAND, seed=11, nconc=12)
    truth = syn.ckd_model(ng=64, nt=6, np_=53, nband=NBAND, seed=11, nconc=12)
    rs = np.random.RandomState(12)
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    scenes = syn.ckd_scenes(model, nscene=8, ncol=50, nlay=54, seed=13)
    cfg = dict(flux_weight=0.2, flux_profile_weight=0.0, broadband_weight=0.5, prior_error=4.0, pressure_corr=0.95,
               temperature_corr=0.95, conc_corr=0.95)                 # the longwave leg of bench.py --full
    ib = model["iband_per_g"]
    for s in scenes:
        ncs, nhl = s["pressure_hl"].shape
        s["flux_dn"] = s["flux_up"] = np.zeros((ncs, nhl, NBAND))
    with api.Context(0) as ctx:
        t_opt = api.Optimizer(ctx, truth, scenes, **kw, **cfg)
        _, fl = t_opt.forward(t_opt.initial_state())
        t_opt.close()
        band = np.stack([fl[..., ib == b].sum(-1) for b in range(NBAND)], axis=-1)
        c0 = 0
        for s in scenes:
            ncs = s["pressure_hl"].shape[0]
            s["flux_dn"], s["flux_up"] = np.ascontiguousarray(band[c0:c0 + ncs, 0]), np.ascontiguousarray(band[c0:c0 + ncs, 1])
            c0 += ncs
        opt = api.Optimizer(ctx, model, scenes, **kw, **cfg)
        x0 = opt.initial_state()
        J0, _ = opt.cost_grad(x0)                                     # warm-up
        t0 = time.perf_counter()
        for _ in range(20):
            opt.cost_grad(x0)
        eval_ms = (time.perf_counter() - t0) / 20 * 1e3
        rates, res = [], None
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            res = opt.minimize(max_iterations=args.iterations, convergence_criterion=0.0, bounded=True)
            rates.append(res["iterations"] / (time.perf_counter() - t0))
        opt.set_progress(lambda *a: None)                             # starts the handle's device-event timers (an event wait per
        rt0 = opt.timings()["radiative transfer"]                     # evaluation: after the rates above, not during them)
        for _ in range(20):
            opt.cost_grad(x0)
        forward_ms = (opt.timings()["radiative transfer"] - rt0) / 20 * 1e3
        out = dict(iters_per_s=rates, iterations=res["iterations"], cost_grad_ms=eval_ms, forward_kernel_ms=forward_ms, J0=J0,
                   J_final=res["cost"], status=res["status"], nx=opt.nx, plan=opt.forward_plan())
        opt.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--nangle", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # (name, package root, nangle, ECCKD_K8A_THREADS or None)
    configs = [("nangle_0", ROOT, 0, None), ("nangle_1", ROOT, 1, None), ("nangle_4", ROOT, 4, None), ("nangle_8", ROOT, 8, None),
               ("nangle_4_threads_256", ROOT, 4, 256), ("nangle_4_threads_512", ROOT, 4, 512)]
    if args.parent:
        configs.insert(0, ("parent_nangle_0", os.path.abspath(args.parent), 0, None))
    runs = {name: [] for name, _, _, _ in configs}
    for _ in range(args.rounds):
        for name, root, nangle, threads in configs:
            env = dict(os.environ)
            env.pop("ECCKD_K8A_THREADS", None)
            if threads:
                env["ECCKD_K8A_THREADS"] = str(threads)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--nangle", str(nangle), "--iterations",
                   str(args.iterations), "--repeats", str(args.repeats)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:          # nothing more is started on the device after a process that failed there
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{name}: the child process ended with status {r.returncode}")
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[len("RESULT "):]))
    span = lambda name, key: [min(min(_list(x[key])) for x in runs[name]), max(max(_list(x[key])) for x in runs[name])]
    summary = {name: dict(iters_per_s=span(name, "iters_per_s"), forward_kernel_ms=span(name, "forward_kernel_ms"),
                          cost_grad_ms=span(name, "cost_grad_ms"), plan=runs[name][0]["plan"]) for name in runs}
    base = "parent_nangle_0" if args.parent else "nangle_0"
    mid = lambda name: sorted(x["forward_kernel_ms"] for x in runs[name])[len(runs[name]) // 2]
    result = {"shape": "ng 64, nlay 54, nband 13, 8 x 50 columns, nx ~ 3e5", "iterations_asked": args.iterations, "rounds": args.rounds,
              "repeats": args.repeats, "summary_min_max": summary,
              "forward_kernel_ratio_to_" + base: {name: mid(name) / mid(base) for name in runs}, "runs": runs}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "opt_lw_angles_probe.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))


def _list(v):
    return v if isinstance(v, list) else [v]


if __name__ == "__main__":
    main()
