"""Time of the fused fluxes of the resident gas-optics handle (ecckd_gas_optics_fluxes_lw_dev / _sw_dev through api.GasOptics)
for the five-gas synthetic model (24 table entries per cell) at 1e5 columns x 54 layers, ng = 32 and 64: longwave nangle 0 and
4, shortwave direct beam and two-stream, each with the broadband fluxes and heating rates as the only outputs and again with
the per-g fluxes as well.  Beside them, in the same process and on the same inputs, what any unfused path pays before a transfer
can start: ecckd_gas_optics_dev (total only) and, longwave, ecckd_gas_optics_planck_dev on the half levels.
Each call sits between two device events on the context's stream (Context.timer_begin / timer_end); per process one warm-up call
and `calls` timed ones, of which the median counts.  The small shape (5 000 columns, ng 64, longwave) is wall clock from device
tensors to device fluxes, set against the composition run_ckd device_gas_optics=1 uses: optical depths and Planck function to
the host, ecckd_rt_lw_gpoints on host arrays, numpy sums.
Every configuration runs in a process of its own, one at a time, the configurations alternating over `rounds` rounds (at least
five): min, max and median over the rounds.  Writes profiles/gas_optics_fluxes_probe.json (or --out) and prints it.
usage: python tools/gas_optics_fluxes_probe.py [--rounds 5] [--calls 3] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLAY, NCOL_LARGE, NCOL_SMALL = 54, 100000, 5000
KINDS = ("lw0", "lw4", "sw_direct", "sw_twostream")


def make_model(np, syn, ng, sw):
    model = syn.ckd_model(ng=ng, seed=5)
    if sw:      # the same tables under a solar spectrum and Rayleigh coefficients
        rs = np.random.RandomState(11)
        model = dict(model, planck_function=None, temperature_planck=None, solar_irradiance=rs.uniform(0.5, 1.5, ng),
                     rayleigh_molar_scattering=10.0 ** rs.uniform(-7.0, -5.5, ng))
    return model


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


def timed(ctx, calls, fn):
    ms = []
    ctx.fence_from_torch()
    for _ in range(calls + 1):
        ctx.timer_begin()
        fn()
        ms.append(ctx.timer_end())
    return median(ms[1:])


def child_large(args):
    import ctypes as C
    import numpy as np
    import torch
    from ecckd_amd import api, synthetic as syn
    sw = args.kind.startswith("sw")
    model = make_model(np, syn, args.ng, sw)
    p, t, vmr = columns(np, syn, model, NCOL_LARGE)
    lib, F64 = api._lib, api._lib.F64
    ptr = lambda x: C.c_void_p(x.data_ptr())
    with api.Context(0) as ctx:
        go = api.GasOptics(ctx, model)
        dp, dt, dv = (torch.as_tensor(a, device=ctx.device) for a in (p, t, vmr))
        mu0 = torch.as_tensor(0.2 + 0.8 * (np.arange(NCOL_LARGE) % 97) / 96.0, device=ctx.device)
        albedo = torch.as_tensor(0.5 * (np.arange(NCOL_LARGE) % 13) / 12.0, device=ctx.device)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=ctx.device)
        nhl = NLAY + 1
        out = {}
        for spectral in (False, True):
            o = lib.FluxOutputs()
            keep = dict(flux_dn=new(NCOL_LARGE, nhl), flux_up=new(NCOL_LARGE, nhl), heating_rate=new(NCOL_LARGE, NLAY))
            if args.kind == "sw_twostream":
                keep["flux_dn_direct"] = new(NCOL_LARGE, nhl)
            if spectral:
                keep["spectral_flux_dn"], keep["spectral_flux_up"] = new(NCOL_LARGE, nhl, args.ng), new(NCOL_LARGE, nhl, args.ng)
                if args.kind == "sw_twostream":
                    keep["spectral_flux_dn_direct"] = new(NCOL_LARGE, nhl, args.ng)
            for k, v in keep.items():
                setattr(o, k, v.data_ptr())
            if sw:
                call = lambda: api.check(ctx.lib.ecckd_gas_optics_fluxes_sw_dev(go.handle, int(args.kind == "sw_twostream"), NCOL_LARGE, NLAY, ptr(dp),
                                                                                ptr(dt), None, ptr(dv), None, None, ptr(mu0), ptr(albedo), 1361.0, F64,
                                                                                C.byref(o)))
            else:
                call = lambda: api.check(ctx.lib.ecckd_gas_optics_fluxes_lw_dev(go.handle, int(args.kind[2:]), NCOL_LARGE, NLAY, ptr(dp), ptr(dt), None,
                                                                                ptr(dv), None, None, F64, C.byref(o)))
            ms = timed(ctx, args.calls, call)
            ctx.synchronize()
            assert all(bool(torch.isfinite(v).all()) for v in keep.values())
            out["with_spectral" if spectral else "broadband"] = dict(call_ms=ms, output_bytes=sum(v.numel() * 8 for v in keep.values()))
            del keep
        # the unfused path's first step on the same inputs: the optical depth (total only) and the Planck function
        od = new(NCOL_LARGE, NLAY, args.ng)
        out["optical_depth_ms"] = timed(ctx, args.calls, lambda: api.check(ctx.lib.ecckd_gas_optics_dev(
            go.handle, NCOL_LARGE, NLAY, ptr(dp), ptr(dt), None, ptr(dv), None, None, 0, F64, ptr(od), None, None)))
        del od
        if not sw:
            pl = new(NCOL_LARGE, nhl, args.ng)
            out["planck_ms"] = timed(ctx, args.calls, lambda: api.check(ctx.lib.ecckd_gas_optics_planck_dev(go.handle, NCOL_LARGE * nhl, ptr(dt), F64,
                                                                                                             ptr(pl))))
            del pl
        out["scratch_bytes"] = go.fluxes_geometry(NLAY, mode=KINDS.index(args.kind) - 1 if sw else 0)["scratch_bytes"]
        go.close()
    print("RESULT " + json.dumps(out))


def child_small(args):
    import numpy as np
    import torch
    from ecckd_amd import api, synthetic as syn
    model = make_model(np, syn, 64, False)
    p, t, vmr = columns(np, syn, model, NCOL_SMALL)
    reps = 3
    with api.Context(0) as ctx:
        go = api.GasOptics(ctx, model)
        dp, dt, dv = (torch.as_tensor(a, device=ctx.device) for a in (p, t, vmr))
        s = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            if args.fused:
                res = go.fluxes_lw(dp, dt, dv)                     # returns after the stream has drained
                dn = res["flux_dn_lw"]
            else:
                od = go.optical_depth(dp, dt, dv)["optical_depth"].cpu().numpy()
                pl = go.planck(dt).cpu().numpy()
                fd, fu = api.rt_lw_gpoints(ctx, pl, od, 0)
                dn = torch.as_tensor(fd.sum(-1), device=ctx.device)
                up = torch.as_tensor(fu.sum(-1), device=ctx.device)
                torch.cuda.synchronize()
            s.append(time.perf_counter() - t0)
        out = dict(wall_ms=median(s[1:]) * 1e3, checksum=float(dn.sum()))
        go.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gas_optics_fluxes_probe.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--ng", type=int, default=64)
    ap.add_argument("--kind", default="lw0")
    ap.add_argument("--fused", type=int, default=1)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.child:
        return child_large(args) if args.child == "large" else child_small(args)
    if args.rounds < 5:
        raise SystemExit("gas_optics_fluxes_probe: at least five rounds")
    configs = [(f"ng{ng}_{kind}", ["--child", "large", "--ng", str(ng), "--kind", kind, "--calls", str(args.calls)]) for ng in (32, 64) for kind in KINDS]
    configs += [(f"fused_{NCOL_SMALL}", ["--child", "small", "--fused", "1"]), (f"composed_{NCOL_SMALL}", ["--child", "small", "--fused", "0"])]
    runs = {name: [] for name, _ in configs}
    for _ in range(args.rounds):
        for name, extra in configs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:          # nothing more is started on the device after a process that failed there
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{name}: the child process ended with status {r.returncode}")
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[len("RESULT "):]))
            print(name, line, flush=True)

    def stats(values):
        return dict(min=min(values), max=max(values), median=median(values))

    summary = {}
    for name, _ in configs:
        first = runs[name][0]
        if name.startswith("ng"):
            summary[name] = {part: dict(call_ms=stats([r[part]["call_ms"] for r in runs[name]]), output_bytes=first[part]["output_bytes"])
                             for part in ("broadband", "with_spectral")}
            for k in ("optical_depth_ms", "planck_ms"):
                if k in first:
                    summary[name][k] = stats([r[k] for r in runs[name]])
            summary[name]["scratch_bytes"] = first["scratch_bytes"]
        else:
            summary[name] = dict(wall_ms=stats([r["wall_ms"] for r in runs[name]]))
    a, b = runs[f"fused_{NCOL_SMALL}"][0]["checksum"], runs[f"composed_{NCOL_SMALL}"][0]["checksum"]
    summary["checksum_relative_difference"] = abs(a - b) / abs(b)
    result = {"shape": f"five-gas synthetic model, 24 entries per cell; large: {NCOL_LARGE} columns x {NLAY} layers; small: ng 64, {NCOL_SMALL} columns",
              "rounds": args.rounds, "calls": args.calls, "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}, indent=1))


if __name__ == "__main__":
    main()
