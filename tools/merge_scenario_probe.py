"""The merged matrix of one scenario, two ways, in one process on synthetic spectra (nwav 7.2e6, 54 layers, 5 FLOAT gases):
  (a) gas by gas, as the tools run it: ecckd_merge_spectrum_dev per gas, each call synchronous, every gas after the first a
      read-modify-write of the DOUBLE matrix - derived 4 + 8 bytes for the first gas and 4 + 16 for each later one per point and
      layer, 92 B for five gases (DESIGN counts about 100 B);
  (b) one ecckd_merge_scenario_dev - derived 4 ngas + 8 = 28 B per point and layer.
HIP events on the context's stream (they span the synchronous calls), one warm-up of each form, then 5 rounds that alternate
the two.  The two matrices are compared by digest (wrapping sums of their bit patterns, plain and position-weighted) and by
torch.equal.  Prints one JSON object and writes it to profiles/merge_scenario_probe.json.
usage: python tools/merge_scenario_probe.py [nwav]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ecckd_amd import api, synthetic as syn  # noqa: E402

nwav = int(sys.argv[1]) if len(sys.argv) > 1 else 7200000
nlay, ngas, rounds = 54, 5, 5
BYTES_ONE_PASS = 4 * ngas + 8
BYTES_SEQUENCE = (4 + 8) + (ngas - 1) * (4 + 16)
BYTES_SEQUENCE_DESIGN = 100


def digest(m):
    """(wrapping sum of the doubles' bit patterns, the same weighted by position) layer by layer, on the device"""
    bits = m.view(torch.int64)
    weight = (torch.arange(m.shape[1], device=m.device, dtype=torch.int64) % 65521) + 1
    plain = weighted = 0
    for l in range(m.shape[0]):
        plain = (plain + int(bits[l].sum())) & 0xFFFFFFFFFFFFFFFF
        weighted = (weighted + (l + 1) * int((bits[l] * weight).sum())) & 0xFFFFFFFFFFFFFFFF
    return "%016x%016x" % (plain, weighted)


def stats(ts, nbytes):
    med = float(np.median(ts))
    return {"ms": [round(t, 3) for t in ts], "median_ms": med, "min_ms": float(min(ts)), "max_ms": float(max(ts)),
            "derived_TB_per_s_at_median": {k: v * nlay * nwav / (med * 1e-3) / 1e12 for k, v in nbytes.items()}}


with api.Context(0) as ctx:
    dev = ctx.device
    p = syn.pressure_grid(nlay)
    wn_h, _ = syn.wavenumber_grid(nwav)
    wn = torch.as_tensor(wn_h, device=dev)
    ods = [syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1 + g, device=dev) for g in range(ngas)]
    assert all(od.dtype == torch.float32 and od.is_contiguous() for od in ods)
    scale = np.ascontiguousarray(np.repeat(np.random.default_rng(7).uniform(0.25, 4.0, ngas)[:, None], nlay, axis=1))
    seq = torch.empty((nlay, nwav), dtype=torch.float64, device=dev)
    one = torch.empty((nlay, nwav), dtype=torch.float64, device=dev)
    ptrs = (C.c_void_p * ngas)(*[od.data_ptr() for od in ods])
    types = (C.c_int * ngas)(*[4] * ngas)
    strides = (C.c_size_t * ngas)(*[nwav] * ngas)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def gas_by_gas():
        for g in range(ngas):
            api.check(ctx.lib.ecckd_merge_spectrum_dev(ctx.handle, nlay, nwav, C.c_void_p(ods[g].data_ptr()), 4, nwav, dp(scale[g]),
                                                       int(g == 0), C.c_void_p(seq.data_ptr()), nwav))
            ctx.synchronize()

    def one_pass():
        api.check(ctx.lib.ecckd_merge_scenario_dev(ctx.handle, nlay, nwav, ngas, ptrs, types, strides, dp(scale), C.c_void_p(one.data_ptr()), nwav))

    ctx.fence_from_torch()
    gas_by_gas(); one_pass()                      # warm
    t_seq, t_one = [], []
    for _ in range(rounds):                       # alternating
        ctx.timer_begin(); gas_by_gas(); t_seq.append(ctx.timer_end())
        ctx.timer_begin(); one_pass(); t_one.append(ctx.timer_end())
    a = stats(t_seq, {"derived_92B": BYTES_SEQUENCE, "design_100B": BYTES_SEQUENCE_DESIGN})
    b = stats(t_one, {"derived_28B": BYTES_ONE_PASS})
    d_seq, d_one = digest(seq), digest(one)
    spread = a["max_ms"] - a["min_ms"]
    out = {"nwav": nwav, "nlay": nlay, "ngas": ngas, "rounds": rounds, "geometry": api.merge_scenario_geometry(),
           "gas_by_gas": a, "one_pass": b, "sequence_over_one_pass": a["median_ms"] / b["median_ms"],
           "sequence_spread_ms": spread, "one_pass_faster_beyond_sequence_spread": bool(b["median_ms"] < a["median_ms"] - spread),
           "digest_gas_by_gas": d_seq, "digest_one_pass": d_one, "digests_equal": d_seq == d_one, "torch_equal": bool(torch.equal(seq, one))}
print(json.dumps(out))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "merge_scenario_probe.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
