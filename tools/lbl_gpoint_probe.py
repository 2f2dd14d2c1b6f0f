"""Timing of the fused per-g-point line-by-line longwave fluxes against the composed path and the band kernel, one column of
nwav = 7.2e6, nlay = 54, ng = 32 (FLOAT optical depths), HIP events on the library's stream, median of 10 after a warm-up:
  (a) ecckd_lbl_gpoint_fluxes_lw (fused);
  (b) ecckd_lbl_spectral_fluxes_lw + ecckd_gmap_sum_rows over 2 x 55 FLOAT rows (composed);
  (c) ecckd_lbl_band_fluxes_lw with 13 bands (the same arithmetic, contiguous reduction).
Each call includes its small host parts (tables up, results down).  Prints one JSON object.
Usage: python tools/lbl_gpoint_probe.py [nwav]"""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecckd_amd import api, synthetic as syn

nwav = int(float(sys.argv[1])) if len(sys.argv) > 1 else 7_200_000
nlay, ng, nband, nrep = 54, 32, 13, 10
out = {"nwav": nwav, "nlay": nlay, "ng": ng, "nband": nband}


def median_ms(ctx, fn):
    fn()
    ts = []
    for _ in range(nrep):
        ctx.timer_begin(); fn(); ts.append(ctx.timer_end())
    return float(np.median(ts))


with api.Context(0) as ctx:
    dev = ctx.device
    p = syn.pressure_grid(nlay)
    t_hl = syn.temperature_profile(p)
    wn_h, dwn_h = syn.wavenumber_grid(nwav)
    wn, dwn = torch.as_tensor(wn_h, device=dev), torch.as_tensor(dwn_h, device=dev)
    od = syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1, device=dev)
    assert od.dtype == torch.float32
    # g points as find_g_points makes them: ranges of the rank under the longwave sorting key - scattered sets of wavenumbers
    k, _ = api.reorder_key_lw(ctx, p, api.idealised_temperature(p), wn, dwn, od, 0.5)
    rank, _ = api.stable_argsort_bands(ctx, k, [0], [nwav - 1], want_ordered=False)
    edges = (nwav * (np.linspace(0.0, 1.0, ng + 1) ** 0.35)).astype(np.int64)
    edges[-1] = nwav
    g_point = torch.bucketize(rank.long(), torch.as_tensor(edges[1:-1], device=dev), right=True).to(torch.int32)
    gm = api.GPointMap(ctx, g_point, ng, wn, dwn)
    bedges = np.linspace(0, nwav, nband + 1).astype(np.int64)
    begin, end = bedges[:-1], bedges[1:] - 1

    a = median_ms(ctx, lambda: gm.lbl_fluxes_lw(t_hl, od))
    c = median_ms(ctx, lambda: api.lbl_band_fluxes_lw(ctx, t_hl, wn, dwn, od, begin, end))
    rows = {}

    def composed():
        sdn, sup, _, _ = api.lbl_spectral_fluxes_lw(ctx, t_hl, wn, dwn, od)
        rows["dn"], rows["up"] = gm.sum_rows(sdn), gm.sum_rows(sup)
    b = median_ms(ctx, composed)
    spec = median_ms(ctx, lambda: api.lbl_spectral_fluxes_lw(ctx, t_hl, wn, dwn, od))
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_hl, od)
    out["fused_vs_composed_max_rel_diff"] = float(np.max(np.abs(rows["up"] - up) / np.maximum(np.abs(up), 1e-300)))
    gm.close()
    bytes_pt = 2 * nlay * 4 + 16 + 4            # the optical depths once per sweep, wavenumber, d_wavenumber, g point
    out.update({"a_fused_ms": a, "b_composed_ms": b, "b_spectral_mode_only_ms": spec, "c_band_kernel_ms": c,
                "a_over_c": a / c, "b_over_a": b / a, "fused_algorithmic_bytes_per_point": bytes_pt,
                "fused_TBs": nwav * bytes_pt / (a * 1e-3) / 1e12, "fused_fraction_of_8TBs": nwav * bytes_pt / (a * 1e-3) / 8e12,
                "composed_extra_bytes_per_point": 2 * (nlay + 1) * 4 * 2})
print(json.dumps(out, indent=1))
