"""Cost-and-gradient evaluations per second of the longwave optimiser with and without the per-g flux-profile term
(api.Optimizer.set_gpoint_truth), at the longwave optimiser shape of bench.py --full: ng = 64, 6 x 53 (T, p) grid, 12 mole
fractions (nx ~ 3e5), 13 bands, 8 scenarios x 50 columns x 54 layers.  Every handle is trained on the fluxes of a perturbed
model through its own transfer; the per-g truth is that model's per-g fluxes.  Every configuration runs in a process of its own,
one at a time, the configurations alternating over `rounds` rounds (at least five), so that drift of the machine shows as spread
within a configuration and not as a difference between two.  In each process: one warm-up evaluation, `evaluations` timed
evaluations (host clock), then 20 with the handle's device events on: the time of the forward kernel alone.
--parent DIR: also time the handle without the term with the package found under DIR (a checkout of the parent commit, built),
in the same rounds: the difference between it and this build's handle without the term has to lie within the parent's own spread.
Writes profiles/opt_gpoint_probe.json and prints it.
usage: python tools/opt_gpoint_probe.py [--rounds 5] [--evaluations 40] [--parent DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBAND, NG, NLAY, NSCENE, NCOL = 13, 64, 54, 8, 50
WEIGHT = 0.1


def child(args):
    sys.path.insert(0, args.root)
    import numpy as np
    from ecckd_amd import api, synthetic as syn
    kw = dict(nangle=args.nangle) if args.nangle > 0 else {}          # (a parent's Optimizer may lack the argument)
    model = syn.ckd_model(ng=NG, nt=6, np_=53, nband=NBAND, seed=11, nconc=12)
    truth = syn.ckd_model(ng=NG, nt=6, np_=53, nband=NBAND, seed=11, nconc=12)
    rs = np.random.RandomState(12)
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    scenes = syn.ckd_scenes(model, nscene=NSCENE, ncol=NCOL, nlay=NLAY, seed=13)
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
        if args.term:
            opt.set_gpoint_truth(WEIGHT, fl)
        x0 = opt.initial_state()
        J0, _ = opt.cost_grad(x0)                                     # warm-up
        t0 = time.perf_counter()
        for _ in range(args.evaluations):
            opt.cost_grad(x0)
        evals_per_s = args.evaluations / (time.perf_counter() - t0)
        opt.set_progress(lambda *a: None)                             # starts the handle's device-event timers
        rt0 = opt.timings()["radiative transfer"]
        for _ in range(20):
            opt.cost_grad(x0)
        forward_ms = (opt.timings()["radiative transfer"] - rt0) / 20 * 1e3
        out = dict(evals_per_s=evals_per_s, forward_kernel_ms=forward_ms, J0=J0, nx=opt.nx, plan=opt.forward_plan())
        opt.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--evaluations", type=int, default=40)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--nangle", type=int, default=0)
    ap.add_argument("--term", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.rounds < 5:
        raise SystemExit("opt_gpoint_probe: at least five rounds (the parent's own spread is the margin)")
    # (name, package root, nangle, with the term)
    configs = [("two_stream", ROOT, 0, 0), ("two_stream_term", ROOT, 0, 1), ("nangle_4", ROOT, 4, 0), ("nangle_4_term", ROOT, 4, 1)]
    if args.parent:
        configs[:0] = [("parent_two_stream", os.path.abspath(args.parent), 0, 0), ("parent_nangle_4", os.path.abspath(args.parent), 4, 0)]
    runs = {name: [] for name, _, _, _ in configs}
    for _ in range(args.rounds):
        for name, root, nangle, term in configs:
            env = dict(os.environ)
            env.pop("ECCKD_K8A_THREADS", None)
            env.pop("ECCKD_K8A_GENERIC", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--nangle", str(nangle), "--term", str(term),
                   "--evaluations", str(args.evaluations)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:          # nothing more is started on the device after a process that failed there
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{name}: the child process ended with status {r.returncode}")
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[len("RESULT "):]))
    span = lambda name, key: [min(x[key] for x in runs[name]), max(x[key] for x in runs[name])]
    mid = lambda name, key: sorted(x[key] for x in runs[name])[len(runs[name]) // 2]
    summary = {name: dict(evals_per_s_min_max=span(name, "evals_per_s"), evals_per_s_median=mid(name, "evals_per_s"),
                          forward_kernel_ms_min_max=span(name, "forward_kernel_ms"), forward_kernel_ms_median=mid(name, "forward_kernel_ms"),
                          plan=runs[name][0]["plan"]) for name in runs}
    result = {"shape": f"ng {NG}, nlay {NLAY}, nband {NBAND}, {NSCENE} x {NCOL} columns, nx ~ 3e5", "rounds": args.rounds,
              "evaluations": args.evaluations, "gpoint_profile_weight": WEIGHT,
              "extra_bytes_read_per_evaluation": 2 * (NLAY + 1) * NG * 8 * NSCENE * NCOL,
              "extra_doubles_read_per_column": 2 * (NLAY + 1) * NG, "summary": summary}
    if args.parent:
        for mine, parent in (("two_stream", "parent_two_stream"), ("nangle_4", "parent_nangle_4")):
            lo, hi = span(parent, "evals_per_s")
            diff = mid(mine, "evals_per_s") - mid(parent, "evals_per_s")
            result[mine + "_against_parent"] = dict(median_difference_evals_per_s=diff, parent_spread_evals_per_s=hi - lo,
                                                    within_parent_spread=abs(diff) <= hi - lo)
    result["runs"] = runs
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "opt_gpoint_probe.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))


if __name__ == "__main__":
    main()
