"""Time per column of the band fluxes of 16 scenarios from one read of the spectra against the single-scenario sequence, in one
process on synthetic spectra (nwav 7.2e6, nlay 54, 5 FLOAT gases, one band over the spectrum):
  (a) one call of ecckd_lbl_band_fluxes_lw_scenarios (nangle 0) / ecckd_lbl_band_fluxes_sw_scenarios (5 angles, with albedo);
  (b) per scenario: ecckd_merge_spectrum_dev x ngas into a DOUBLE matrix, then ecckd_lbl_band_fluxes_lw (longwave), or
      ecckd_lbl_band_fluxes_sw once per angle (shortwave).
HIP events on the context's stream, one warm-up and 5 timed repeats each.  Prints one JSON object.
usage: python tools/lbl_scenarios_probe.py [nwav]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecckd_amd import api, synthetic as syn  # noqa: E402

nwav = int(sys.argv[1]) if len(sys.argv) > 1 else 7200000
nlay, ngas, nscen, nrep = 54, 5, 16, 5
mu = (0.1, 0.3, 0.5, 0.7, 0.9)


def times_ms(ctx, fn):
    fn()
    ts = []
    for _ in range(nrep):
        ctx.timer_begin(); fn(); ts.append(ctx.timer_end())
    return {"ms": [round(t, 3) for t in ts], "median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def spectra(dev, p, wn):
    ods = [syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1 + g, device=dev) for g in range(ngas)]
    assert all(od.dtype == torch.float32 for od in ods)
    return ods


def compare(a, b):
    """fused against parent: median, min-max, ratio, and whether (a) is slower than (b) by more than (b)'s own spread."""
    return {"fused_over_parent": a["median_ms"] / b["median_ms"], "parent_spread_ms": b["max_ms"] - b["min_ms"],
            "fused_not_slower_beyond_parent_spread": bool(a["median_ms"] <= b["median_ms"] + (b["max_ms"] - b["min_ms"]))}


with api.Context(0) as ctx:
    dev = ctx.device
    p = syn.pressure_grid(nlay)
    scales = np.random.default_rng(7).uniform(0.25, 4.0, (nscen, ngas))
    scales[0] = 1.0
    profile = np.ascontiguousarray(np.repeat(scales[:, :, None], nlay, axis=2))
    begin, end = np.array([0]), np.array([nwav - 1])
    merged = torch.empty((nlay, nwav), dtype=torch.float64, device=dev)
    out = {"nwav": nwav, "nlay": nlay, "ngas": ngas, "nscen": nscen, "repeats": nrep}

    # ---- longwave ----
    wn_h, dwn_h = syn.wavenumber_grid(nwav)
    wn, dwn = torch.as_tensor(wn_h, device=dev), torch.as_tensor(dwn_h, device=dev)
    t_hl = syn.temperature_profile(p)
    ods = spectra(dev, p, wn)

    def merge_scenario(s):
        """The parent's merged DOUBLE matrix of scenario s, gas after gas into the one resident buffer (as bin/ckdmip_lw does)."""
        for g in range(ngas):
            api.check(ctx.lib.ecckd_merge_spectrum_dev(ctx.handle, nlay, nwav, ods[g].data_ptr(), 4, nwav,
                                                       profile[s, g].ctypes.data_as(C.POINTER(C.c_double)), int(g == 0), merged.data_ptr(), nwav))

    def lw_parent():
        res = []
        for s in range(nscen):
            merge_scenario(s)
            res.append(api.lbl_band_fluxes_lw(ctx, t_hl, wn, dwn, merged, begin, end))
        return res

    ctx.fence_from_torch()
    a = times_ms(ctx, lambda: api.lbl_band_fluxes_lw_scenarios(ctx, t_hl, wn, dwn, ods, scales, begin, end))
    b = times_ms(ctx, lw_parent)
    fdn, fup = api.lbl_band_fluxes_lw_scenarios(ctx, t_hl, wn, dwn, ods, scales, begin, end)
    ref = lw_parent()
    T = api.lbl_scenarios_slots(False, nlay)
    launches = -(-nscen // T)
    bytes_pl = ngas * 4 * 2 * launches                   # per point and layer: the gas rows once per sweep and launch (derived)
    out["lw"] = {"fused": a, "parent_sequence": b, **compare(a, b), "slots_per_launch": T, "launches": launches,
                 "derived_bytes_per_point_layer": bytes_pl, "fused_TBs_at_derived_bytes": nwav * nlay * bytes_pl / (a["median_ms"] * 1e-3) / 1e12,
                 "fused_point_layer_scenarios_per_s": nwav * nlay * nscen / (a["median_ms"] * 1e-3),
                 "max_rel_diff_vs_parent": float(max(np.max(np.abs(fdn[s] - ref[s][0]) / ref[s][0].max()) for s in range(nscen)))}
    del ods, wn, dwn
    torch.cuda.empty_cache()

    # ---- shortwave ----
    wn_h, dwn_h = syn.wavenumber_grid(nwav, 250.0, 50000.0)
    wn = torch.as_tensor(wn_h, device=dev)
    ssi = torch.as_tensor(syn.solar_spectral_irradiance(wn_h, dwn_h), device=dev)
    albedo = torch.as_tensor(np.where(wn_h < 12000.0, 0.2, 0.05), device=dev)
    ods = spectra(dev, p, wn)

    def sw_parent():
        res = []
        for s in range(nscen):
            merge_scenario(s)
            res.append([api.lbl_band_fluxes_sw(ctx, c, ssi, merged, begin, end, albedo=albedo) for c in mu])
        return res

    ctx.fence_from_torch()
    a = times_ms(ctx, lambda: api.lbl_band_fluxes_sw_scenarios(ctx, mu, ssi, ods, scales, begin, end, albedo=albedo))
    b = times_ms(ctx, sw_parent)
    fdn, fup = api.lbl_band_fluxes_sw_scenarios(ctx, mu, ssi, ods, scales, begin, end, albedo=albedo)
    ref = sw_parent()
    T = api.lbl_scenarios_slots(True, nlay)
    per = min(T // len(mu), 16 // len(mu))
    launches = -(-nscen // per)
    bytes_pl = ngas * 4 * 2 * launches
    out["sw"] = {"nsza": len(mu), "fused": a, "parent_sequence": b, **compare(a, b), "slots_per_launch": T, "scenarios_per_launch": per,
                 "launches": launches, "derived_bytes_per_point_layer": bytes_pl,
                 "fused_TBs_at_derived_bytes": nwav * nlay * bytes_pl / (a["median_ms"] * 1e-3) / 1e12,
                 "fused_point_layer_slots_per_s": nwav * nlay * nscen * len(mu) / (a["median_ms"] * 1e-3),
                 "max_rel_diff_vs_parent": float(max(np.max(np.abs(fdn[s, k] - ref[s][k][0]) / ref[s][k][0].max())
                                                     for s in range(nscen) for k in range(len(mu))))}
print(json.dumps(out, indent=1))
