"""Time per column of the Rayleigh-scattering two-stream shortwave band fluxes against the no-scattering kernel:
  (a) ecckd_lbl_band_fluxes_sw_rayleigh, five angles in one call (absorption and Rayleigh optical depths apart);
  (b) five calls of ecckd_lbl_band_fluxes_sw_ex, one per angle, on the summed optical depth: today's treatment, Rayleigh as
      one more absorber.
nlay 54, nwav 2^22 (a shortwave job's size), FLOAT optical depths, with albedo, 13 bands.  Prints one JSON object.
usage: python tools/lbl_rayleigh_probe.py [nwav]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecckd_amd import api, synthetic as syn  # noqa: E402

nwav = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 22
nlay, nband, nrep = 54, 13, 10
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
    wn = torch.as_tensor(wn_h, device=dev)
    od = syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1, device=dev)
    assert od.dtype == torch.float32
    # Rayleigh: ~ wavenumber^4, a column total of 1 at 50 000 cm-1 shared among the layers by their pressure thickness
    dp = torch.as_tensor(np.diff(p) / (p[-1] - p[0]), device=dev, dtype=torch.float64)
    ray = (dp[:, None] * (wn[None, :] / 50000.0) ** 4).to(torch.float32)
    total = (od.double() + ray.double()).to(torch.float32)
    ssi = torch.as_tensor(syn.solar_spectral_irradiance(wn_h, dwn_h), device=dev)
    albedo = torch.as_tensor(np.where(wn_h < 12000.0, 0.2, 0.05), device=dev)
    edges = np.linspace(0, nwav, nband + 1).astype(np.int64)
    begin, end = edges[:-1], edges[1:] - 1

    a = median_ms(ctx, lambda: api.lbl_band_fluxes_sw_rayleigh(ctx, mu, ssi, od, ray, begin, end, albedo=albedo))
    a1 = median_ms(ctx, lambda: api.lbl_band_fluxes_sw_rayleigh(ctx, mu[2], ssi, od, ray, begin, end, albedo=albedo))
    b = median_ms(ctx, lambda: [api.lbl_band_fluxes_sw(ctx, m, ssi, total, begin, end, albedo=albedo) for m in mu])
    direct, dn, up = api.lbl_band_fluxes_sw_rayleigh(ctx, mu, ssi, od, ray, begin, end, albedo=albedo)
    total64 = od.double() + ray.double()                      # what the Rayleigh kernel forms per layer: the direct beams must agree
    band = [api.lbl_band_fluxes_sw(ctx, m, ssi, total64, begin, end, albedo=albedo) for m in mu]
    inc = np.array(mu)[:, None] * np.array([float(ssi[b0:b1 + 1].sum()) for b0, b1 in zip(begin, end)])[None, :]
    nchunk = int(sum(-(-(e - b0 + 1) // 256) for b0, e in zip(begin, end)))
    grid = min(nchunk, 3 * torch.cuda.get_device_properties(0).multi_processor_count)
    # per wavenumber, angle and layer: the direct chain (1 exp), and rayleigh_layer in each of the two adding sweeps (2 exp, 1 sqrt,
    # 4 divisions: w, f, f2, inv)
    out = {"nwav": nwav, "nlay": nlay, "nsza": nsza, "nband": nband, "a_rayleigh_5_angles_ms": a, "a1_rayleigh_1_angle_ms": a1,
           "b_no_scattering_5_calls_ms": b, "a_over_b": a / b, "blocks": grid, "chunks": nchunk,
           "workspace_bytes": grid * 3 * (nlay + 1) * 256 * 8,
           "rayleigh_exponentials_per_point": nsza * nlay * 5, "rayleigh_Gexp_per_s": nwav * nsza * nlay * 5 / (a * 1e-3) / 1e9,
           "no_scattering_Gexp_per_s": nwav * 2 * nlay * nsza / (b * 1e-3) / 1e9,
           "workspace_traffic_bytes_per_point": nsza * (nlay + 1) * 8 * (3 + 4),
           "toa_reflectance_rayleigh": (up[:, :, 0] / inc).tolist(),
           "toa_reflectance_no_scattering": [(band[s][1][:, 0] / inc[s]).tolist() for s in range(nsza)],
           "direct_vs_no_scattering_max_rel_diff": float(max(np.max(np.abs(direct[s] - band[s][0]) / np.maximum(band[s][0], 1e-300))
                                                             for s in range(nsza)))}
print(json.dumps(out, indent=1))
