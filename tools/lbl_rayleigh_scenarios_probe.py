"""Time per column of the Rayleigh two-stream band fluxes of 16 scenarios from one read of the spectra against the
single-scenario sequence, in one process on synthetic spectra (nwav 2^22, nlay 54, 5 angles, 13 bands, 5 FLOAT gases, a FLOAT
Rayleigh row, with albedo):
  (a) one call of ecckd_lbl_band_fluxes_sw_rayleigh_scenarios;
  (b) per scenario: ecckd_merge_spectrum_dev x ngas into a DOUBLE matrix, then ecckd_lbl_band_fluxes_sw_rayleigh with the 5 angles.
HIP events on the context's stream, one warm-up and 5 timed repeats each.  Then the wall time of one
`bin/ckdmip_sw --scenarios ... --scenarios-rayleigh` run against the 16 `--rayleigh ... --scenario` runs on files of --cli-nwav
points (one column), written as tools/e2e_bench.py writes its spectra; that comparison depends on the page cache and is reported
only.  Prints one JSON object and writes it to profiles/lbl_rayleigh_scenarios_probe.json.
usage: python tools/lbl_rayleigh_scenarios_probe.py [nwav] [--cli-nwav N | --no-cli] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from ecckd_amd import api, synthetic as syn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("nwav", nargs="?", type=int, default=2 ** 22)
ap.add_argument("--cli-nwav", type=int, default=None)
ap.add_argument("--no-cli", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbl_rayleigh_scenarios_probe.json"))
args = ap.parse_args()
nwav = args.nwav
nlay, ngas, nscen, nband, nrep = 54, 5, 16, 13, 5
mu = (0.1, 0.3, 0.5, 0.7, 0.9)
nsza = len(mu)
LO, HI = 250.0, 50000.0


def times_ms(ctx, fn):
    fn()
    ts = []
    for _ in range(nrep):
        ctx.timer_begin(); fn(); ts.append(ctx.timer_end())
    return {"ms": [round(t, 3) for t in ts], "median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def rayleigh_row(p, wn):
    """~ wavenumber^4, a column total of 1 at 50 000 cm-1 shared among the layers by their pressure thickness"""
    dp = torch.as_tensor(np.diff(p) / (p[-1] - p[0]), device=wn.device, dtype=torch.float64)
    return (dp[:, None] * (wn[None, :] / HI) ** 4).to(torch.float32)


def device_part(ctx):
    dev = ctx.device
    p = syn.pressure_grid(nlay)
    wn_h, dwn_h = syn.wavenumber_grid(nwav, LO, HI)
    wn = torch.as_tensor(wn_h, device=dev)
    ods = [syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1 + g, device=dev) for g in range(ngas)]
    assert all(od.dtype == torch.float32 for od in ods)
    ray = rayleigh_row(p, wn)
    ssi = torch.as_tensor(syn.solar_spectral_irradiance(wn_h, dwn_h), device=dev)
    albedo = torch.as_tensor(np.where(wn_h < 12000.0, 0.2, 0.05), device=dev)
    edges = np.linspace(0, nwav, nband + 1).astype(np.int64)
    begin, end = edges[:-1], edges[1:] - 1
    scales = np.random.default_rng(7).uniform(0.25, 4.0, (nscen, ngas))
    scales[0] = 1.0
    profile = np.ascontiguousarray(np.repeat(scales[:, :, None], nlay, axis=2))
    merged = torch.empty((nlay, nwav), dtype=torch.float64, device=dev)

    def parent():
        res = []
        for s in range(nscen):
            for g in range(ngas):
                api.check(ctx.lib.ecckd_merge_spectrum_dev(ctx.handle, nlay, nwav, ods[g].data_ptr(), 4, nwav,
                                                           profile[s, g].ctypes.data_as(C.POINTER(C.c_double)), int(g == 0), merged.data_ptr(), nwav))
            res.append(api.lbl_band_fluxes_sw_rayleigh(ctx, mu, ssi, merged, ray, begin, end, albedo=albedo))
        return res

    fused = lambda: api.lbl_band_fluxes_sw_rayleigh_scenarios(ctx, mu, ssi, ods, ray, scales, begin, end, albedo=albedo)
    ctx.fence_from_torch()
    a = times_ms(ctx, fused)
    b = times_ms(ctx, parent)
    got, ref = fused(), parent()
    inc = np.array(mu)[:, None] * np.array([float(ssi[b0:b1 + 1].sum()) for b0, b1 in zip(begin, end)])[None, :]
    diff = max(float(np.max(np.abs(got[k][s] - ref[s][k]) / inc[:, :, None])) for s in range(nscen) for k in range(3))
    bitwise = all(np.array_equal(got[k][s], ref[s][k]) for s in range(nscen) for k in range(3))
    nchunk = int(sum(-(-(e - b0 + 1) // 256) for b0, e in zip(begin, end)))
    per = api.lbl_rayleigh_scenarios_per_launch(nlay, nsza, nchunk)
    env_grid = int(os.environ.get("ECCKD_RAYLEIGH_GRID", "0"))
    grid = min(nchunk, env_grid if env_grid >= 1 else 4 * torch.cuda.get_device_properties(0).multi_processor_count)
    spread = b["max_ms"] - b["min_ms"]
    return {"fused": a, "parent_sequence": b, "fused_over_parent": a["median_ms"] / b["median_ms"], "parent_spread_ms": spread,
            "fused_ms_per_scenario": a["median_ms"] / nscen, "parent_ms_per_scenario": b["median_ms"] / nscen,
            "fused_not_slower_than_parent": bool(a["median_ms"] < b["median_ms"]),
            "fused_not_slower_beyond_parent_spread": bool(a["median_ms"] <= b["median_ms"] + spread),
            "chunks": nchunk, "blocks": grid, "scenarios_per_launch": min(per, nscen), "launches": -(-nscen // min(per, nscen)),
            "workspace_bytes": grid * 4 * (nlay + 1) * 256 * 8,
            "partial_bytes_per_launch": nchunk * min(per, nscen) * nsza * 3 * (nlay + 1) * 8,
            "max_diff_vs_parent_per_incoming_flux": diff, "bitwise_equal_to_parent": bool(bitwise)}


def cli_part(n):
    """One column, ngas + 1 files of n points: the 16 single runs against the one --scenarios run, wall time of the processes."""
    from e2e_bench import _write_spectrum
    from scipy.io import netcdf_file
    exe = os.path.join(ROOT, "bin", "ckdmip_sw")
    with tempfile.TemporaryDirectory(prefix="rayleigh_scenarios_probe_") as d:
        with api.Context(0) as ctx:
            p = syn.pressure_grid(nlay)
            wn_h, dwn_h = syn.wavenumber_grid(n, LO, HI)
            wn = torch.as_tensor(wn_h, device=ctx.device)
            t0 = syn.temperature_profile(p)
            for g in range(ngas):
                od = syn.optical_depth_lines(torch, p, wn, syn.SEED_BASE + 1 + g, device=ctx.device).cpu().numpy()
                _write_spectrum(os.path.join(d, f"gas{g}.nc"), f"gas{g}", p, [t0], wn_h, od, 1e-4)
            _write_spectrum(os.path.join(d, "rayleigh.nc"), "rayleigh", p, [t0], wn_h, rayleigh_row(p, wn).cpu().numpy(), 1.0)
            w = netcdf_file(os.path.join(d, "ssi.nc"), "w", version=2)
            w.createDimension("wavenumber", n)
            w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = syn.solar_spectral_irradiance(wn_h, dwn_h)
            w.close()
        torch.cuda.empty_cache()
        edges = np.linspace(LO, HI, nband + 1)
        with open(os.path.join(d, "sw.nam"), "w") as f:
            f.write("&shortwave_config\noptical_depth_name = \"optical_depth\",\nsurf_albedo = 0.15,\nuse_mu0_dimension = true,\n"
                    f"cos_solar_zenith_angle(1:{nsza}) = {', '.join(str(m) for m in mu)},\nnspectralstride = 1,\n"
                    f"band_wavenumber1(1:{nband}) = {', '.join(f'{e:.6f}' for e in edges[:-1])},\n"
                    f"band_wavenumber2(1:{nband}) = {', '.join(f'{e:.6f}' for e in edges[1:])},\n/\n")
        scales = np.random.default_rng(7).uniform(0.25, 4.0, (nscen, ngas))
        scales[0] = 1.0
        files = [f"gas{g}.nc" for g in range(ngas)]
        with open(os.path.join(d, "table.txt"), "w") as f:
            for s in range(nscen):
                f.write(f"s{s} multi_{s}.nc " + " ".join(f"scale={float(scales[s, g])!r}" for g in range(ngas)) + "\n")
        common = [exe, "--config", "sw.nam", "--ssi", "ssi.nc"]

        def run(*words):
            t = time.perf_counter()
            subprocess.run([*common, *words], cwd=d, check=True, capture_output=True, timeout=1500)
            return time.perf_counter() - t
        run("--rayleigh", "rayleigh.nc", "--scenario", "warm", *files, "--output", "warm.nc")       # the files into the page cache
        t_multi = run("--scenarios", "table.txt", "--scenarios-rayleigh", "rayleigh.nc", *files)
        t_single = []
        for s in range(nscen):
            words = []
            for g in range(ngas):
                words += ["--scale", repr(float(scales[s, g])), files[g]]
            t_single.append(run("--rayleigh", "rayleigh.nc", "--scenario", f"s{s}", *words, "--output", f"single_{s}.nc"))
        a = netcdf_file(os.path.join(d, "multi_3.nc"), "r", mmap=False)
        b = netcdf_file(os.path.join(d, "single_3.nc"), "r", mmap=False)
        same = bool(np.allclose(a.variables["band_flux_up_sw"][...], b.variables["band_flux_up_sw"][...], rtol=2e-7, atol=1e-30))
        a.close(); b.close()
    return {"nwav": n, "columns": 1, "file_bytes": (ngas + 1) * nlay * n * 4, "scenarios_run_s": t_multi, "single_runs_s": float(sum(t_single)),
            "single_runs_over_scenarios_run": float(sum(t_single)) / t_multi, "page_cache": "warm (one run of the tool before the timed ones)",
            "outputs_agree": same}


out = {"nwav": nwav, "nlay": nlay, "nsza": nsza, "nband": nband, "ngas": ngas, "nscen": nscen, "repeats": nrep}
with api.Context(0) as ctx:
    out.update(device_part(ctx))
torch.cuda.empty_cache()


def report():
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return text


report()                                             # the device figures are kept whatever becomes of the tool runs
if not args.no_cli:
    out["cli"] = cli_part(args.cli_nwav or nwav)
print(report())
