"""Timing probe for the longwave sweep kernel alone: a fixed whole-partition batch (38 intervals over the 7.2e6 points) and a
few single intervals, timed by the library's HIP events around every launch (ECCKD_BG64=1: with DOUBLE background rows;
ECCKD_RT_PERSISTENT=1: one resident round of blocks walking the chunks; ECCKD_RT_UNALIGNED=1: chunks counted from the
interval's first point instead of the 128-byte line below it).
usage: python tools/sweep_probe.py [nwav] [--i1-mod R] [--only SUBSTRING] [--rowmajor | --blocked]
  --rowmajor   make the gas with ECCKD_RT_ROWMAJOR=1: row-major Planck and background matrices and the row-major sweep
  --blocked    make it without: the sweep's operands line-blocked (csrc/sweep_layout.hpp), whatever the environment says
  --i1-mod R   move every interval, keeping its length (the spectrum's end cuts it), so that its first sorted index is R
               modulo 16 (16 doubles = one 128-byte line): R = 0 starts every row load of every tile on a line, R = 1 is the
               same batch one point on
  --only S     run only the batches whose label contains S (for a counter pass over one kind of launch)"""
import os, sys, json
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecckd_amd import api, synthetic as syn

os.environ["ECCKD_NO_ERROR_MEMO"] = "1"
argv = sys.argv[1:]
i1_mod = only = None
if "--i1-mod" in argv:
    k = argv.index("--i1-mod")
    i1_mod = int(argv[k + 1]) % 16
    del argv[k:k + 2]
if "--only" in argv:
    k = argv.index("--only")
    only = argv[k + 1]
    del argv[k:k + 2]
if "--rowmajor" in argv:
    argv.remove("--rowmajor")
    os.environ["ECCKD_RT_ROWMAJOR"] = "1"
if "--blocked" in argv:
    argv.remove("--blocked")
    os.environ.pop("ECCKD_RT_ROWMAJOR", None)
nwav, nlay = int(argv[0]) if argv else 7200000, 54


def place(b1, b2):
    """The bounds of the same intervals with their first indices at i1_mod modulo 16.  The library takes ceil(b1 (n-1)) and
    floor(b2 (n-1)) as the first and the last index (make_interval): bounds half a point outside them give exactly those."""
    b1, b2 = np.asarray(b1, dtype=np.float64), np.asarray(b2, dtype=np.float64)
    if i1_mod is None:
        return b1, b2
    i1 = np.ceil(b1 * (nwav - 1)).astype(np.int64)
    i2 = np.maximum(np.floor(b2 * (nwav - 1)).astype(np.int64), i1)
    j1 = i1 // 16 * 16 + i1_mod
    j2 = np.minimum(j1 + (i2 - i1), nwav - 1)      # an interval that would leave the spectrum loses its last points
    assert np.all(j1 <= j2) and np.all(j1 % 16 == i1_mod)
    return np.maximum((j1 - 0.5) / (nwav - 1), 0.0), np.minimum((j2 + 0.5) / (nwav - 1), 1.0)


ctx = api.Context(0)
dev = ctx.device
p = syn.pressure_grid(nlay)
wn_h, dwn_h = syn.wavenumber_grid(nwav)
wn, dwn = torch.as_tensor(wn_h, device=dev), torch.as_tensor(dwn_h, device=dev)
od = syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1, device=dev)
bg = syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1001, column_scale=3.0, device=dev)
key, col = api.reorder_key_lw(ctx, p, api.idealised_temperature(p), wn, dwn, od, 0.5)
rank, _ = api.stable_argsort_bands(ctx, key, [0], [nwav - 1], want_ordered=False)
gas = api.GasLW(ctx, p, syn.temperature_profile(p), wn, dwn, rank, od, bg, "transmission", flux_weight=0.0)
bpp = gas.sweep_bytes_per_point()
cuts = np.linspace(0.0, 1.0, 39) ** 1.5
try:
    gas.view_ptr("planck_hl_blocked")
    layout = "blocked"
except api.EcckdError:
    layout = "row-major"
out = {"bytes_per_point": bpp, "i1_mod_16": i1_mod, "layout": layout}
even = np.linspace(0.0, 1.0, 39)
for label, (b1, b2) in (("whole partition, 38 intervals", (cuts[:-1], cuts[1:])), ("whole partition, 38 equal intervals", (even[:-1], even[1:])),
                        ("whole partition, 1 interval", ([0.0], [1.0])), ("whole partition, 4 equal intervals", ([0.0, 0.25, 0.5, 0.75], [0.25, 0.5, 0.75, 1.0])),
                        ("one interval of 190 000 points", ([0.4], [0.4 + 190000.0 / nwav])),
                        ("one interval of 40 000 points", ([0.4], [0.4 + 40000.0 / nwav])),
                        ("one interval of 1 000 000 points", ([0.4], [0.4 + 1000000.0 / nwav]))):
    if only is not None and only not in label:
        continue
    b1, b2 = place(b1, b2)
    for _ in range(3):
        gas.calc_error_batch(0, nwav, b1, b2)
    ctx.profile_enable(1)
    for _ in range(20):
        gas.calc_error_batch(0, nwav, b1, b2)
    calls, ms, pts = ctx.profile_get("k_rt_lw_bb")
    ctx.profile_enable(0)
    out[label] = {"launches": calls, "us_per_launch": 1e3 * ms / calls, "points_per_launch": pts / calls, "TBs": pts * bpp / (ms * 1e-3) / 1e12}
print(json.dumps(out))
