"""Wall time of the per-g-point truth of a 16-scenario training set, two ways, on synthetic files (ecckd_amd/synthetic.py: 5 FLOAT
gas files of one column, 54 layers; a 32-g-point map):
  (a) one `lw_spectra gpoints= nangle=4 scenarios=TABLE` with a 16-line table;
  (b) the sixteen single runs `lw_spectra gpoints= nangle=4 scaling=... output=...`, one process each, as the scripts run them.
(b) is run with the tools of --baseline-bin DIR (the parent commit's build) when given, else with this tree's, whose single-run
path is the parent's.  Two rounds, alternating; every output of (a) is compared with its single run variable by variable.
Prints one JSON object and writes it to profiles/spectra_scenarios_probe.json.
usage: python tools/spectra_scenarios_probe.py [nwav] [--baseline-bin DIR]"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
from scipy.io import netcdf_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ecckd_amd import api, synthetic as syn  # noqa: E402
import e2e_bench  # noqa: E402

args = sys.argv[1:]
baseline_bin = os.path.join(ROOT, "bin")
if "--baseline-bin" in args:
    i = args.index("--baseline-bin")
    baseline_bin = os.path.abspath(args[i + 1])
    del args[i:i + 2]
nwav = int(args[0]) if args else 1000000
nlay, ngas, nscen, ng, rounds = 54, 5, 16, 32, 2
GASES = ("h2o", "co2", "o3", "ch4", "n2o")


def run(exe, *keys, cwd):
    t0 = time.perf_counter()
    r = subprocess.run([exe, *keys], cwd=cwd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{exe} {' '.join(keys)}: exit {r.returncode}\n{r.stderr}")
    return time.perf_counter() - t0


d = tempfile.mkdtemp(prefix="spectra_scenarios_probe_")
try:
    with api.Context(0) as ctx:                 # the files: written once, outside the timed windows
        p = syn.pressure_grid(nlay)
        t = syn.temperature_profile(p)
        wn_h, _ = syn.wavenumber_grid(nwav)
        wn = torch.as_tensor(wn_h, device=ctx.device)
        for g, name in enumerate(GASES):
            od = syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1 + g, device=ctx.device)
            e2e_bench._write_spectrum(os.path.join(d, name + ".nc"), name, p, [t], wn_h, od.cpu().numpy(), 1.0e-4 * (g + 1))
            del od
    rng = np.random.default_rng(3)
    w = netcdf_file(os.path.join(d, "gpoints.nc"), "w", version=2)
    w.createDimension("wavenumber", nwav)
    w.createVariable("g_point", "i", ("wavenumber",))[:] = rng.integers(0, ng, nwav).astype(np.int32)
    w.close()
    scales = rng.uniform(0.25, 4.0, (nscen, ngas)).round(3)
    scales[0] = 1.0
    with open(os.path.join(d, "table.txt"), "w") as f:
        for s in range(nscen):
            f.write(f"scen{s} table_{s}.nc " + " ".join("asis" if v == 1.0 else f"scale={v}" for v in scales[s]) + "\n")
    common = ("input=" + " ".join(g + ".nc" for g in GASES), "gpoints=gpoints.nc", "nangle=4", "log_level=warning")
    table_s, singles_s = [], []
    for _ in range(rounds):
        table_s.append(run(os.path.join(ROOT, "bin", "lw_spectra"), *common, "scenarios=table.txt", cwd=d))
        singles_s.append(sum(run(os.path.join(baseline_bin, "lw_spectra"), *common, "scaling=" + " ".join(str(v) for v in scales[s]),
                                 f"output=single_{s}.nc", cwd=d) for s in range(nscen)))
    equal = True
    for s in range(nscen):
        a, b = netcdf_file(os.path.join(d, f"table_{s}.nc"), "r", mmap=False), netcdf_file(os.path.join(d, f"single_{s}.nc"), "r", mmap=False)
        equal = equal and list(a.variables) == list(b.variables) and all(np.array_equal(a.variables[k][...], b.variables[k][...]) for k in a.variables)
    input_bytes = sum(os.path.getsize(os.path.join(d, g + ".nc")) for g in GASES)
    out = {"nwav": nwav, "nlay": nlay, "ngas": ngas, "nscen": nscen, "ng": ng, "nangle": 4, "rounds": rounds,
           "baseline_bin": "this tree" if baseline_bin == os.path.join(ROOT, "bin") else "given", "input_bytes": input_bytes,
           "table_run_s": [round(x, 3) for x in table_s], "sixteen_single_runs_s": [round(x, 3) for x in singles_s],
           "singles_over_table": min(singles_s) / min(table_s), "outputs_equal": bool(equal)}
finally:
    shutil.rmtree(d, ignore_errors=True)
print(json.dumps(out))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "spectra_scenarios_probe.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
