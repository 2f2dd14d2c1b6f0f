"""Time of the resident fluxes under clouds (ecckd_gas_optics_fluxes_lw_sky_dev / _sw_sky_dev) beside the clear calls, by the
method of tools/gas_optics_fluxes_probe.py and on its inputs: the five-gas synthetic model (24 table entries per cell, three
bands) at 1e5 columns x 54 layers, ng = 32 and 64; longwave nangle 0 and 4 and the two-stream shortwave transfer, the broadband
fluxes and heating rates as the only outputs.  Per configuration, in ONE process and on the same inputs:
    clear      the clear call
    sky_null   the sky call with nothing given (the clear kernel instance: the same time)
    sky_zero   the sky kernel with cloud arrays of zeros (longwave: emissivity 1 and the air's temperature as skin temperature as
               well): what the sky instance costs before any cloud
    sky_cloud  the sky kernel with clouds in a third of the layers (every third layer, all bands; longwave with an emissivity
               below 1 and a skin temperature)
Each call sits between two device events on the context's stream (Context.timer_begin / timer_end); per process one warm-up call
and `calls` timed ones of each, of which the median counts.  Every configuration runs in a process of its own, one at a time,
the configurations alternating over `rounds` rounds (at least five): min, max and median over the rounds.
Writes profiles/gas_optics_sky_probe.json (or --out) and prints it.
usage: python tools/gas_optics_sky_probe.py [--rounds 5] [--calls 3] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gas_optics_fluxes_probe as base  # noqa: E402

NLAY, NCOL = base.NLAY, base.NCOL_LARGE
KINDS = ("lw0", "lw4", "sw_twostream")
VARIANTS = ("clear", "sky_null", "sky_zero", "sky_cloud")


def child(args):
    import ctypes as C
    import numpy as np
    import torch
    from ecckd_amd import api, synthetic as syn
    sw = args.kind.startswith("sw")
    model = base.make_model(np, syn, args.ng, sw)
    nband = int(np.max(model["iband_per_g"])) + 1
    p, t, vmr = base.columns(np, syn, model, NCOL)
    lib, F64 = api._lib, api._lib.F64
    ptr = lambda x: C.c_void_p(x.data_ptr())
    with api.Context(0) as ctx:
        go = api.GasOptics(ctx, model)
        dp, dt, dv = (torch.as_tensor(a, device=ctx.device) for a in (p, t, vmr))
        mu0 = torch.as_tensor(0.2 + 0.8 * (np.arange(NCOL) % 97) / 96.0, device=ctx.device)
        albedo = torch.as_tensor(0.5 * (np.arange(NCOL) % 13) / 12.0, device=ctx.device)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=ctx.device)
        nhl = NLAY + 1
        keep = dict(flux_dn=new(NCOL, nhl), flux_up=new(NCOL, nhl), heating_rate=new(NCOL, NLAY))
        if sw:
            keep["flux_dn_direct"] = new(NCOL, nhl)
        o = lib.FluxOutputs()
        for k, v in keep.items():
            setattr(o, k, v.data_ptr())
        # clouds in every third layer, the optical depth between 0.1 and 10 by column and band
        rs = np.random.RandomState(7)
        od = np.zeros((NCOL, NLAY, nband))
        od[:, 1::3] = 10.0 ** rs.uniform(-1.0, 1.0, (NCOL, 1, nband))
        tensors = dict(zero=torch.zeros((NCOL, NLAY, nband), dtype=torch.float64, device=ctx.device), cloud=torch.as_tensor(od, device=ctx.device),
                       ssa=torch.as_tensor(np.broadcast_to(rs.uniform(0.9, 1.0, (NCOL, 1, nband)), od.shape).copy(), device=ctx.device),
                       asym=torch.as_tensor(np.broadcast_to(rs.uniform(0.7, 0.9, (NCOL, 1, nband)), od.shape).copy(), device=ctx.device),
                       one=torch.ones((NCOL, nband), dtype=torch.float64, device=ctx.device),
                       emis=torch.as_tensor(rs.uniform(0.9, 1.0, (NCOL, nband)), device=ctx.device),
                       air=dt[:, -1].contiguous(), skin=(dt[:, -1] + 2.0).contiguous())

        def sky(variant):
            if variant == "sky_null":
                return None
            s = lib.FluxSky()
            s.cloud_od = tensors["zero" if variant == "sky_zero" else "cloud"].data_ptr()
            if sw:
                s.cloud_ssa, s.cloud_asymmetry, s.delta_eddington = tensors["ssa"].data_ptr(), tensors["asym"].data_ptr(), 1
            else:
                s.surface_emissivity = tensors["one" if variant == "sky_zero" else "emis"].data_ptr()
                s.skin_temperature = tensors["air" if variant == "sky_zero" else "skin"].data_ptr()
            return s

        def call_of(variant):
            if variant == "clear":
                if sw:
                    return lambda: api.check(ctx.lib.ecckd_gas_optics_fluxes_sw_dev(go.handle, 1, NCOL, NLAY, ptr(dp), ptr(dt), None, ptr(dv), None, None,
                                                                                    ptr(mu0), ptr(albedo), 1361.0, F64, C.byref(o)))
                return lambda: api.check(ctx.lib.ecckd_gas_optics_fluxes_lw_dev(go.handle, int(args.kind[2:]), NCOL, NLAY, ptr(dp), ptr(dt), None, ptr(dv),
                                                                                None, None, F64, C.byref(o)))
            s = sky(variant)
            sp = None if s is None else C.addressof(s)
            if sw:
                return lambda s=s: api.check(ctx.lib.ecckd_gas_optics_fluxes_sw_sky_dev(go.handle, NCOL, NLAY, ptr(dp), ptr(dt), None, ptr(dv), None, None,
                                                                                        ptr(mu0), ptr(albedo), 1361.0, F64, C.byref(o), sp))
            return lambda s=s: api.check(ctx.lib.ecckd_gas_optics_fluxes_lw_sky_dev(go.handle, int(args.kind[2:]), NCOL, NLAY, ptr(dp), ptr(dt), None,
                                                                                    ptr(dv), None, None, F64, C.byref(o), sp))

        out = {}
        for variant in VARIANTS:
            ms = base.timed(ctx, args.calls, call_of(variant))
            ctx.synchronize()
            assert all(bool(torch.isfinite(v).all()) for v in keep.values())
            out[variant] = dict(call_ms=ms, checksum=float(keep["flux_up"].sum()))
        out["sky_input_bytes"] = int(od.nbytes * (3 if sw else 1) + (0 if sw else NCOL * (nband + 1) * 8))
        go.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gas_optics_sky_probe.json"))
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--ng", type=int, default=64)
    ap.add_argument("--kind", default="lw0")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.child:
        return child(args)
    if args.rounds < 5:
        raise SystemExit("gas_optics_sky_probe: at least five rounds")
    configs = [(f"ng{ng}_{kind}", ["--child", "1", "--ng", str(ng), "--kind", kind, "--calls", str(args.calls)]) for ng in (32, 64) for kind in KINDS]
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
        return dict(min=min(values), max=max(values), median=base.median(values))

    summary = {}
    for name, _ in configs:
        first = runs[name][0]
        summary[name] = {v: dict(call_ms=stats([r[v]["call_ms"] for r in runs[name]])) for v in VARIANTS}
        clear_ms = summary[name]["clear"]["call_ms"]["median"]
        for v in VARIANTS[1:]:
            summary[name][v]["over_clear"] = summary[name][v]["call_ms"]["median"] / clear_ms
        summary[name]["null_is_clear_bit_for_bit"] = all(r["sky_null"]["checksum"] == r["clear"]["checksum"] for r in runs[name])
        summary[name]["sky_input_bytes"] = first["sky_input_bytes"]
    result = {"shape": f"five-gas synthetic model, 24 entries per cell, 3 bands; {NCOL} columns x {NLAY} layers; broadband fluxes and heating rates",
              "rounds": args.rounds, "calls": args.calls, "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}, indent=1))


if __name__ == "__main__":
    main()
