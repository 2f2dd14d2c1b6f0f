"""Time per column of the fused multi-angle shortwave line-by-line fluxes per g point against the band kernel:
  (a) ecckd_lbl_gpoint_fluxes_sw, five angles in one call (fused; its launches repeat the transfer, see the file header);
  (b) five calls of ecckd_lbl_band_fluxes_sw with one band covering the spectrum: the radiative transfer alone, one angle per
      pass over the optical depths, no binning.
nlay 54, nwav 2^22, ng 32, FLOAT optical depths, with albedo.  Prints one JSON object.
usage: python tools/lbl_gpoint_sw_probe.py [nwav]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecckd_amd import api, synthetic as syn  # noqa: E402

nwav = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 22
nlay, ng, nrep = 54, 32, 10
mu = (0.1, 0.3, 0.5, 0.7, 0.9)
nsza = len(mu)


def median_ms(ctx, fn):
    fn()
    ts = []
    for _ in range(nrep):
        ctx.timer_begin(); fn(); ts.append(ctx.timer_end())
    return float(np.median(ts))


with api.Context(0) as ctx:
    dev = ctx.device
    p = syn.pressure_grid(nlay)
    wn_h, dwn_h = syn.wavenumber_grid(nwav, 250.0, 50000.0)
    wn, dwn = torch.as_tensor(wn_h, device=dev), torch.as_tensor(dwn_h, device=dev)
    od = syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1, device=dev)
    assert od.dtype == torch.float32
    ssi = torch.as_tensor(syn.solar_spectral_irradiance(wn_h, dwn_h), device=dev)
    albedo = torch.as_tensor(np.where(wn_h < 12000.0, 0.2, 0.05), device=dev)
    g_point = torch.as_tensor(np.random.default_rng(3).integers(0, ng, size=nwav).astype(np.int32), device=dev)   # scattered
    gm = api.GPointMap(ctx, g_point, ng, wn, dwn)
    begin, end = np.array([0]), np.array([nwav - 1])

    a = median_ms(ctx, lambda: gm.lbl_fluxes_sw(mu, ssi, od, albedo))
    a1 = median_ms(ctx, lambda: gm.lbl_fluxes_sw(mu[2], ssi, od, albedo))
    b = median_ms(ctx, lambda: [api.lbl_band_fluxes_sw(ctx, m, ssi, od, begin, end, albedo=albedo) for m in mu])
    dn, up, bdn, bup = gm.lbl_fluxes_sw(mu, ssi, od, albedo)
    band = [api.lbl_band_fluxes_sw(ctx, m, ssi, od, begin, end, albedo=albedo) for m in mu]
    gm.close()
    # the split of csrc/lbl_gpoint_fluxes_sw.hip (its header): SF_ACC_BYTES = 80 KB - 22 528 B of static LDS
    cap = (80 * 1024 - 22528) // (16 * (nlay + 1))           # column-angles per launch
    if cap >= ng + 1:
        amax = min(nsza, cap // (ng + 1))
        launches_a, launches_c = -(-nsza // amax), 1         # angle groups, every column in each
    else:
        launches_a, launches_c = nsza, -(-(ng + 1) // cap)    # one angle per launch, column ranges per angle
    launches = launches_a * launches_c
    bytes_pt = launches * (2 * nlay * 4 + 8 + 8 + 4)      # per launch: the optical depths once per sweep, ssi, albedo, g point
    exps_pt = nlay * (nsza * launches_c + launches)
    out = {"nwav": nwav, "nlay": nlay, "ng": ng, "nsza": nsza, "a_fused_5_angles_ms": a, "a1_fused_1_angle_ms": a1,
           "five_single_angle_calls_ms": nsza * a1, "b_band_kernel_5_calls_ms": b, "a_over_b": a / b, "fused_launches": launches,
           "fused_algorithmic_bytes_per_point": bytes_pt, "fused_exponentials_per_point": exps_pt,
           "fused_TBs": nwav * bytes_pt / (a * 1e-3) / 1e12, "fused_Gexp_per_s": nwav * exps_pt / (a * 1e-3) / 1e9,
           "band_Gexp_per_s": nwav * 2 * nlay * nsza / (b * 1e-3) / 1e9,
           "bb_vs_band_max_rel_diff": float(max(np.max(np.abs(bdn[s] - band[s][0][0]) / band[s][0][0]) for s in range(nsza)))}
print(json.dumps(out, indent=1))
