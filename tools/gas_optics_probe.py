"""Time of one ecckd_gas_optics_dev call (api.GasOptics) for the five-gas synthetic model (5 x 16 (T, p) grid, 4 mole
fractions, 24 table entries per cell) at the size of a model grid, 1e5 columns x 54 layers, at ng = 32 and 64, float64 and
float32 output, without per-gas outputs and with all five; and the parent's ecckd_run_ckd against the new call at 400 and 5 000
columns (ng = 64), host inputs to host output.
Large shape: the call sits between two device events on the context's stream (Context.timer_begin / timer_end); per process one
warm-up call and `calls` timed ones, of which the median counts.  The rate is OUTPUT bytes per second (what the call has to
store: 8 or 4 bytes per (cell, g) and array), given also as a fraction of the rate at which a device-to-device copy of the same
byte count runs in the same process (torch copy_ between torch events, same warm-up and median).
Small shapes: wall clock around everything either path needs from numpy inputs to a numpy optical depth: ecckd_run_ckd with the
optical depth as its only output; for the handle the upload of the three inputs, the call and the download - with the handle
already resident, and again with its creation counted.
Every configuration runs in a process of its own, one at a time, the configurations alternating over `rounds` rounds (at least
five): min, max and median over the rounds.  Writes profiles/gas_optics_probe.json and prints it.
usage: python tools/gas_optics_probe.py [--rounds 5] [--calls 5]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLAY, NCOL_LARGE = 54, 100000


def columns(np, syn, model, ncol):
    """ncol different columns from the four of synthetic.ckd_scenes: each repeat a little warmer and moister"""
    s = syn.ckd_scenes(model, nscene=1, ncol=4, nlay=NLAY, seed=3, ch4_low=True)[0]
    c = np.arange(ncol)
    rep = (c // 4) * (40.0 / max(ncol, 1))
    vmr = s["vmr_fl"][c % 4].copy()
    vmr[:, 1] *= (1.0 + 0.01 * rep)[:, None]
    return s["pressure_hl"][c % 4].copy(), s["temperature_hl"][c % 4] + 0.1 * rep[:, None], vmr


def median(v):
    return sorted(v)[len(v) // 2]


def child_large(args):
    import numpy as np
    import torch
    from ecckd_amd import api, synthetic as syn
    model = syn.ckd_model(ng=args.ng, seed=5)
    dtype = torch.float32 if args.f32 else torch.float64
    p, t, vmr = columns(np, syn, model, NCOL_LARGE)
    with api.Context(0) as ctx:
        go = api.GasOptics(ctx, model)
        dp, dt, dv = (torch.as_tensor(a, device=ctx.device) for a in (p, t, vmr))
        out = {}
        for per_gas in (False, True):
            narr = 1 + (go.ngas if per_gas else 0)
            nbytes = narr * NCOL_LARGE * NLAY * args.ng * (4 if args.f32 else 8)
            arrays = torch.empty((narr, NCOL_LARGE, NLAY, args.ng), dtype=dtype, device=ctx.device)
            ptrs = (C.c_void_p * go.ngas)(*[arrays[1 + i].data_ptr() if per_gas else None for i in range(go.ngas)])
            ms = []
            ctx.fence_from_torch()
            for _ in range(args.calls + 1):
                ctx.timer_begin()
                api.check(ctx.lib.ecckd_gas_optics_dev(go.handle, NCOL_LARGE, NLAY, C.c_void_p(dp.data_ptr()), C.c_void_p(dt.data_ptr()), None,
                                                       C.c_void_p(dv.data_ptr()), None, None, 0, api._lib.F32 if args.f32 else api._lib.F64,
                                                       C.c_void_p(arrays[0].data_ptr()), ptrs if per_gas else None, None))
                ms.append(ctx.timer_end())
            call_ms = median(ms[1:])
            dst = torch.empty_like(arrays)
            cms = []
            for _ in range(args.calls + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(arrays)
                e1.record()
                e1.synchronize()
                cms.append(e0.elapsed_time(e1))
            copy_ms = median(cms[1:])
            assert torch.isfinite(arrays).all()
            del dst, arrays
            out["per_gas" if per_gas else "total_only"] = dict(
                call_ms=call_ms, output_bytes=nbytes, output_GB_per_s=nbytes / call_ms * 1e-6, copy_ms=copy_ms,
                copy_GB_per_s=nbytes / copy_ms * 1e-6, fraction_of_copy_rate=copy_ms / call_ms)
        go.close()
    print("RESULT " + json.dumps(out))


def child_small(args):
    import numpy as np
    import torch
    from ecckd_amd import api, synthetic as syn
    model = syn.ckd_model(ng=64, seed=5)
    p, t, vmr = columns(np, syn, model, args.ncol)
    reps = 3
    with api.Context(0) as ctx:
        if args.run_ckd:
            keep = []
            m = api._opt_model(model, keep)
            sc = api._lib.OptScene()
            api._opt_scene(sc, dict(pressure_hl=p, temperature_hl=t, vmr_fl=vmr), keep)
            od = np.empty((args.ncol, NLAY, 64))
            s = []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                api.check(ctx.lib.ecckd_run_ckd(ctx.handle, C.byref(m), C.byref(sc), od.ctypes.data_as(C.POINTER(C.c_double)), None, None, None))
                s.append(time.perf_counter() - t0)
            out = dict(wall_ms=median(s[1:]) * 1e3, checksum=float(od.sum()))
        else:
            def once(go):
                dev = [torch.as_tensor(a, device=ctx.device) for a in (p, t, vmr)]
                return go.optical_depth(*dev)["optical_depth"].cpu().numpy()
            go = api.GasOptics(ctx, model)
            s, s_create = [], []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                od = once(go)
                s.append(time.perf_counter() - t0)
            go.close()
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                g2 = api.GasOptics(ctx, model)
                once(g2)
                g2.close()
                s_create.append(time.perf_counter() - t0)
            out = dict(wall_ms=median(s[1:]) * 1e3, wall_ms_with_create=median(s_create[1:]) * 1e3, checksum=float(od.sum()))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--ng", type=int, default=64)
    ap.add_argument("--f32", type=int, default=0)
    ap.add_argument("--ncol", type=int, default=400)
    ap.add_argument("--run_ckd", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.child:
        return child_large(args) if args.child == "large" else child_small(args)
    if args.rounds < 5:
        raise SystemExit("gas_optics_probe: at least five rounds")
    configs = [(f"ng{ng}_{'f32' if f32 else 'f64'}", ["--child", "large", "--ng", str(ng), "--f32", str(f32), "--calls", str(args.calls)])
               for ng in (32, 64) for f32 in (0, 1)]
    for ncol in (400, 5000):
        configs.append((f"run_ckd_{ncol}", ["--child", "small", "--ncol", str(ncol), "--run_ckd", "1"]))
        configs.append((f"gas_optics_{ncol}", ["--child", "small", "--ncol", str(ncol), "--run_ckd", "0"]))
    runs = {name: [] for name, _ in configs}
    for _ in range(args.rounds):
        for name, extra in configs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:          # nothing more is started on the device after a process that failed there
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{name}: the child process ended with status {r.returncode}")
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[len("RESULT "):]))

    def stats(values):
        return dict(min=min(values), max=max(values), median=median(values))

    summary = {}
    for name, _ in configs:
        if name.startswith("ng"):
            summary[name] = {part: {k: stats([r[part][k] for r in runs[name]]) for k in ("call_ms", "output_GB_per_s", "copy_GB_per_s", "fraction_of_copy_rate")}
                             for part in ("total_only", "per_gas")}
            for part in ("total_only", "per_gas"):
                summary[name][part]["output_bytes"] = runs[name][0][part]["output_bytes"]
        else:
            summary[name] = {k: stats([r[k] for r in runs[name]]) for k in runs[name][0] if k != "checksum"}
    for ncol in (400, 5000):
        a, b = runs[f"run_ckd_{ncol}"][0]["checksum"], runs[f"gas_optics_{ncol}"][0]["checksum"]
        summary[f"checksum_relative_difference_{ncol}"] = abs(a - b) / abs(a)
    result = {"shape": f"five-gas synthetic model, 24 entries per cell; large: {NCOL_LARGE} columns x {NLAY} layers; small: ng 64, {NLAY} layers",
              "rounds": args.rounds, "calls": args.calls, "summary": summary, "runs": runs}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gas_optics_probe.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}, indent=1))


if __name__ == "__main__":
    main()
