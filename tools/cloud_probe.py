"""Timing probe for the cloud pseudo-gas at the shortwave probe size (tools/sw_probe.py): nwav = 3.3e6 on the 250-50000 cm-1 grid,
a seeded smooth synthetic Mie table of 400 knots (synthetic.mie_table).  Times, on the device (HIP events around each call):
the sorting variable (ecckd_cloud_sorting_variable_dev), the per-band stable sort of its keys, the cloud partition
(ecckd_cloud_partition_dev); then the wall time of bin/reorder_cloud_spectrum with a *.nc and a *.h5 output.  Prints one JSON
line.  Run under `rocprofv3 --kernel-trace --stats ... -- python tools/cloud_probe.py --no-tool` for the per-kernel times.
Usage: python tools/cloud_probe.py [--nwav N] [--no-tool] [--workdir DIR]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ecckd_amd import api, synthetic as syn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nwav", type=int, default=3300000)
ap.add_argument("--no-tool", action="store_true")
ap.add_argument("--workdir", default=None)
ap.add_argument("--repeat", type=int, default=5)
a = ap.parse_args()

import torch  # noqa: E402

nwav = a.nwav
ctx = api.Context(0)
dev = ctx.device
wn_h, dwn_h = syn.wavenumber_grid(nwav, 250.0, 50000.0)
ssi_h = syn.solar_spectral_irradiance(wn_h, dwn_h)
mwn, mssa, mg = syn.mie_table(11, nknot=400)
wn = torch.as_tensor(wn_h, device=dev)
ssi = torch.as_tensor(ssi_h, device=dev)
# the 32-band structure's bounds are not public here: 32 bands equally spaced in log wavenumber
edges = np.geomspace(250.0, 50000.0, 33)
_, bb, be = api.band_ranges(wn_h, edges[:-1], edges[1:])


def timed(fn):
    ms = []
    for _ in range(a.repeat):
        ctx.synchronize()
        ctx.timer_begin()
        out = fn()
        ms.append(ctx.timer_end())
    return out, float(np.median(ms)), float(np.min(ms))


key, t_key, t_key_min = timed(lambda: api.cloud_sorting_variable(ctx, mwn, mssa[0], mg[0], wn))
(rank, _), t_sort1, _ = timed(lambda: api.stable_argsort_bands(ctx, key, [0], [nwav - 1], want_ordered=False, sync=False))
(rank32, _), t_sort32, _ = timed(lambda: api.stable_argsort_bands(ctx, key, bb, be, want_ordered=False, sync=False))
part, t_part, t_part_min = timed(lambda: api.cloud_partition(ctx, ssi, rank32, key, bb, be, 0.05))
hbm = 8.0e12
bytes_key = 16.0 * nwav                            # wavenumber in, key out
# scatter (ssi, sorting variable, rank in; both in rank order out, after zeroing them) + tile reduce (16 B) + tile scan (16 B)
# + per-g-point statistics (8 B)
bytes_part = (8 + 8 + 4 + 16 + 16) * nwav + 16.0 * nwav + 16.0 * nwav + 8.0 * nwav
res = dict(nwav=nwav, nknot=int(mwn.size), nband=int(len(bb)),
           sorting_variable_ms=t_key, sorting_variable_min_ms=t_key_min, sorting_variable_bytes=bytes_key,
           sorting_variable_hbm_bound_ms=1e3 * bytes_key / hbm,
           sort_1band_ms=t_sort1, sort_32band_ms=t_sort32,
           partition_ms=t_part, partition_min_ms=t_part_min, partition_bytes=bytes_part, partition_hbm_bound_ms=1e3 * bytes_part / hbm,
           partition_ng=int(len(part["rank1"])))

if not a.no_tool:
    from scipy.io import netcdf_file
    d = a.workdir or tempfile.mkdtemp(prefix="cloud_probe_")
    os.makedirs(d, exist_ok=True)
    w = netcdf_file(os.path.join(d, "ssi.nc"), "w", version=2)
    w.createDimension("wavenumber", nwav)
    w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn_h
    w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = ssi_h
    w.close()
    w = netcdf_file(os.path.join(d, "mie.nc"), "w", version=2)
    w.createDimension("effective_radius", mssa.shape[0])
    w.createDimension("wavenumber", mwn.size)
    w.createVariable("wavenumber", "f", ("wavenumber",))[:] = mwn
    w.createVariable("single_scattering_albedo", "f", ("effective_radius", "wavenumber"))[:] = mssa
    w.createVariable("asymmetry_factor", "f", ("effective_radius", "wavenumber"))[:] = mg
    w.close()
    b1 = "wavenumber1=" + " ".join("%.6f" % v for v in edges[:-1])
    b2 = "wavenumber2=" + " ".join("%.6f" % v for v in edges[1:])
    for ext in ("nc", "h5"):
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "bin", "reorder_cloud_spectrum"), "input=mie.nc", "isize=0", "wavenumber_input=ssi.nc",
                                f"output=order_cloud.{ext}", b1, b2], cwd=d, capture_output=True, text=True, timeout=300,
                               env=dict(os.environ, ECCKD_LOG_TIMES="1"))
            walls.append(time.perf_counter() - t0)
            if r.returncode != 0:
                raise SystemExit(r.stderr)
        res[f"tool_{ext}_wall_s"] = float(np.median(walls))
        res[f"tool_{ext}_log"] = [ln for ln in r.stdout.splitlines() if ln.startswith("[")]
        res[f"tool_{ext}_bytes"] = os.path.getsize(os.path.join(d, f"order_cloud.{ext}"))
ctx.close()
print(json.dumps(res))
