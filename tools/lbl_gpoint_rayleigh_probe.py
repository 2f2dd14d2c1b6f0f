"""Time per column of the Rayleigh two-stream line-by-line fluxes per g point against the band entry that does the same transfer:
  gpoint ng=16 / 32 / 96   ecckd_lbl_gpoint_fluxes_sw_rayleigh, five angles in one call (one launch per angle and column range:
                            1, 1 and 3 ranges at 54 layers);
  band                     ecckd_lbl_band_fluxes_sw_rayleigh on the same column with 13 bands: the same transfer arithmetic per
                            wavenumber, five angles in one launch, no binning - the yardstick;
  no_scattering            the pair of tools/lbl_gpoint_sw_probe.py on the same column: ecckd_lbl_gpoint_fluxes_sw (ng = 32)
                            and five calls of ecckd_lbl_band_fluxes_sw - what binning costs where nothing scatters.
One synthetic column of 7.2e6 points x 54 layers, FLOAT optical depths, with albedo.  Every measurement runs in a process of its
own under its own time limit; after one that fails nothing more is started.  Prints one JSON object (and writes it with --out).
usage: python tools/lbl_gpoint_rayleigh_probe.py [nwav] [--out FILE]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NWAV = 7200000
NLAY, NBAND, NREP, NG_NO_SCATTERING = 54, 13, 10, 32
MU = (0.1, 0.3, 0.5, 0.7, 0.9)
MEASUREMENTS = ("band", "gpoint:16", "gpoint:32", "gpoint:96", "no_scattering")
LIMIT_S = 240


def one(name, nwav):
    """a single measurement -> dict"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from ecckd_amd import api, synthetic as syn

    def median_ms(ctx, fn):
        fn()
        ts = []
        for _ in range(NREP):
            ctx.timer_begin(); fn(); ts.append(ctx.timer_end())
        return float(np.median(ts))

    with api.Context(0) as ctx:
        dev = ctx.device
        p = syn.pressure_grid(NLAY)
        wn_h, dwn_h = syn.wavenumber_grid(nwav, 250.0, 50000.0)
        wn, dwn = torch.as_tensor(wn_h, device=dev), torch.as_tensor(dwn_h, device=dev)
        od = syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1, device=dev)
        assert od.dtype == torch.float32
        # Rayleigh: ~ wavenumber^4, a column total of 1 at 50 000 cm-1 shared among the layers by their pressure thickness
        dp = torch.as_tensor(np.diff(p) / (p[-1] - p[0]), device=dev, dtype=torch.float64)
        ray = (dp[:, None] * (wn[None, :] / 50000.0) ** 4).to(torch.float32)
        ssi = torch.as_tensor(syn.solar_spectral_irradiance(wn_h, dwn_h), device=dev)
        albedo = torch.as_tensor(np.where(wn_h < 12000.0, 0.2, 0.05), device=dev)
        edges = np.linspace(0, nwav, NBAND + 1).astype(np.int64)
        begin, end = edges[:-1], edges[1:] - 1
        g_map = lambda ng: api.GPointMap(ctx, torch.as_tensor(np.random.default_rng(3).integers(0, ng, size=nwav).astype(np.int32),
                                                              device=dev), ng, wn, dwn)            # scattered
        if name == "band":
            ms = median_ms(ctx, lambda: api.lbl_band_fluxes_sw_rayleigh(ctx, MU, ssi, od, ray, begin, end, albedo=albedo))
            up = api.lbl_band_fluxes_sw_rayleigh(ctx, MU, ssi, od, ray, begin, end, albedo=albedo)[2]
            return {"band_rayleigh_5_angles_ms": ms, "band_toa_up": up[:, :, 0].sum(1).tolist()}
        if name.startswith("gpoint:"):
            ng = int(name.split(":")[1])
            gm = g_map(ng)
            ms = median_ms(ctx, lambda: gm.lbl_fluxes_sw_rayleigh(MU, ssi, od, ray, albedo))
            ms1 = median_ms(ctx, lambda: gm.lbl_fluxes_sw_rayleigh(MU[2], ssi, od, ray, albedo))
            bup = gm.lbl_fluxes_sw_rayleigh(MU, ssi, od, ray, albedo)[5]
            gm.close()
            cap = (80 * 1024 - 22528) // (24 * (NLAY + 1))                                         # the file header's formula
            return {"ng": ng, "gpoint_rayleigh_5_angles_ms": ms, "gpoint_rayleigh_1_angle_ms": ms1,
                    "launches": len(MU) * -(-(ng + 1) // cap), "gpoint_toa_up": bup[:, 0].tolist()}
        assert name == "no_scattering"
        total = (od.double() + ray.double()).to(torch.float32)
        gm = g_map(NG_NO_SCATTERING)
        a = median_ms(ctx, lambda: gm.lbl_fluxes_sw(MU, ssi, total, albedo))
        b = median_ms(ctx, lambda: [api.lbl_band_fluxes_sw(ctx, m, ssi, total, begin, end, albedo=albedo) for m in MU])
        gm.close()
        return {"gpoint_no_scattering_5_angles_ms": a, "band_no_scattering_5_calls_ms": b}


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if len(argv) > 1 and argv[0] == "--one":
        print("RESULT " + json.dumps(one(argv[1], int(argv[2]))))
        return 0
    nwav = int(argv[0]) if argv else NWAV
    res = {"nwav": nwav, "nlay": NLAY, "nsza": len(MU), "nband": NBAND, "gpoint": {}}
    for name in MEASUREMENTS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, str(nwav)], capture_output=True, text=True,
                               timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            res["stopped_at"] = name + ": time limit"
            break
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res["stopped_at"] = "%s: exit code %d: %s" % (name, r.returncode, r.stderr[-400:])
            break
        d = json.loads(line[-1][7:])
        if name.startswith("gpoint:"):
            res["gpoint"][str(d.pop("ng"))] = d
        else:
            res.update(d)
    if "band_rayleigh_5_angles_ms" in res:
        for d in res["gpoint"].values():
            d["over_band"] = d["gpoint_rayleigh_5_angles_ms"] / res["band_rayleigh_5_angles_ms"]
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return 1 if "stopped_at" in res else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
