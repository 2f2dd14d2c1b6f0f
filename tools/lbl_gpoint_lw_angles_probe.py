"""Timing of the zenith-angle quadrature in the fused per-g-point line-by-line longwave fluxes, one column of nwav = 7.2e6,
nlay = 54, ng = 32 (FLOAT optical depths), HIP events on the library's stream, warm, median of 10 with the spread (min, max):
  (a) ecckd_lbl_gpoint_fluxes_lw_angles (fused: one walk of the layers for all angles) at nangle = 0, 1, 4, 8, 16;
  (b) N calls of the two-stream entry ecckd_lbl_gpoint_fluxes_lw, N = 1, 4, 8, 16: what N sweeps of the existing kernel cost;
  (c) ecckd_lbl_band_fluxes_lw_angles with 13 bands on the same column at the same nangle (re-reads the rows per angle).
Each call includes its small host parts (tables up, results down).  Prints one JSON object.
Usage: python tools/lbl_gpoint_lw_angles_probe.py [nwav]"""
import ctypes as C
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecckd_amd import _lib, api, synthetic as syn

nwav = int(float(sys.argv[1])) if len(sys.argv) > 1 else 7_200_000
nlay, ng, nband, nrep = 54, 32, 13, 10
ANGLES = (0, 1, 4, 8, 16)
out = {"nwav": nwav, "nlay": nlay, "ng": ng, "nband": nband, "nrep": nrep}


def timed_ms(ctx, fn):
    fn()
    ts = []
    for _ in range(nrep):
        ctx.timer_begin(); fn(); ts.append(ctx.timer_end())
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


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

    # the two-stream C entry itself, as a caller without the key reaches it
    t = np.ascontiguousarray(t_hl, dtype=np.float64)
    h = [np.empty((nlay + 1, ng)), np.empty((nlay + 1, ng)), np.empty(nlay + 1), np.empty(nlay + 1)]
    hp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))

    def two_stream():
        _lib.check(ctx.lib.ecckd_lbl_gpoint_fluxes_lw(gm.handle, nlay, hp(t), C.c_void_p(od.data_ptr()), _lib.F32, od.stride(0),
                                                      hp(h[0]), hp(h[1]), hp(h[2]), hp(h[3])))

    def repeat(n):
        for _ in range(n):
            two_stream()

    ctx.fence_from_torch()
    fused, calls, band = {}, {}, {}
    for n in ANGLES:
        fused[n] = timed_ms(ctx, lambda: gm.lbl_fluxes_lw(t_hl, od, nangle=n))
        band[n] = timed_ms(ctx, lambda: api.lbl_band_fluxes_lw(ctx, t_hl, wn, dwn, od, begin, end, nangle=n))
        if n > 0:
            calls[n] = timed_ms(ctx, lambda: repeat(n))
    out["two_stream_entry_ms"] = timed_ms(ctx, two_stream)
    # the quadrature against the band kernel at 4 angles (chain bound, see the tests), so the timings are of right answers
    g_band = torch.as_tensor(np.repeat(np.arange(nband, dtype=np.int32), np.diff(bedges)), device=dev)
    gb = api.GPointMap(ctx, g_band, nband, wn, dwn)
    _, up, _, _ = gb.lbl_fluxes_lw(t_hl, od, nangle=4)
    _, up_k = api.lbl_band_fluxes_lw(ctx, t_hl, wn, dwn, od, begin, end, nangle=4)
    out["fused_vs_band_kernel_max_rel_diff_nangle4"] = float(np.max(np.abs(up - up_k.T) / np.abs(up_k.T)))
    gb.close()
    gm.close()
    bytes_pt = 2 * nlay * 4 + 16 + 4            # the optical depths once per sweep, wavenumber, d_wavenumber, g point
    out["a_fused_ms"] = {str(n): fused[n] for n in ANGLES}
    out["b_n_two_stream_calls_ms"] = {str(n): calls[n] for n in ANGLES if n > 0}
    out["c_band_kernel_ms"] = {str(n): band[n] for n in ANGLES}
    out["a_over_b"] = {str(n): fused[n]["median"] / calls[n]["median"] for n in ANGLES if n > 0}
    out["a_over_c"] = {str(n): fused[n]["median"] / band[n]["median"] for n in ANGLES}
    out["fused_algorithmic_bytes_per_point"] = bytes_pt
    out["fused_TBs"] = {str(n): nwav * bytes_pt / (fused[n]["median"] * 1e-3) / 1e12 for n in ANGLES}
    # fp64 work that grows with the angles: 2 nlay lw_layer + lw_step + weight per angle and point
    out["fused_ns_per_point_layer_sweep_angle"] = {str(n): fused[n]["median"] * 1e6 / (nwav * 2 * nlay * n) for n in ANGLES if n > 0}
print(json.dumps(out, indent=1))
