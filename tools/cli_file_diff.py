#!/usr/bin/env python3
"""Compare what the flux tools of two checkouts write, byte for byte.  Needs an MI355X and both checkouts built.

  python tools/cli_file_diff.py <parent checkout> <this tree> [--work DIR]

The CLI tests compare the tools with the library at rtol ~ 3e-7, which cannot show that a rewrite of a tool moved nothing.
This writes the small inputs those tests use - make_do_all_inputs (3 columns), the shortwave files of
test_ckdmip_sw_stand_in (16 layers, 8000 points) with a Rayleigh spectrum, the od.nc / od_sw.nc of the --ckd tests, a
g-points file - once, then runs the command lines of RUNS with each checkout's bin/, from the same working directory and
with the same words, and compares every pair of output files:
  * classic files through scipy's reader: dimension names, sizes and order; variable names, order, types, dimensions and
    attributes; the raw bytes of every variable; every global attribute except `history` (the time and argv[0]) and the
    `0=<argv[0]>` entry that the spectra tools' `config` begins with;
  * every file, the NetCDF-4 ones (*.h5) included, through ecckd_amd.ncio.NcFile under the names of its classic twin: the
    dimensions' sizes, every variable's type and shape, its values and text attributes, the global text attributes.
REFUSED are command lines that must fail: their exit code and stderr are compared.  Each tool run has a time limit of its
own and the first failure ends the script.  Exit status 1 on any difference.  A tool, not a test: it needs a second checkout.

bin/find_g_points likewise (FIND_G_RUNS, FIND_G_REFUSED) on the inputs of its tool tests under find_g/: the 12 000-point
longwave files of tests/test_cli_gpu.py in two bands, the 16 000-point shortwave files of test_find_g_points_sw and the cloud
case of tests/test_cloud_gpu.py.  Of these runs stdout is compared too (same working directory, same words, ECCKD_LOG_TIMES
unset); a run of two processes shares device 0, and the file of rank 0 and the stdout of both ranks are compared."""
import argparse, os, pathlib, shutil, subprocess, sys, tempfile

import numpy as np
from scipy.io import netcdf_file

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

LW_GASES = ("--scale", "0.5", "ideal_h2o.nc", "--const", "6e-4", "ideal_co2.nc")
SW_GASES = ("ideal_h2o.nc", "--scale", "0.5", "ideal_o3.nc")
LW_SPECTRA = ("append_path=.", "input=ideal_h2o.nc ideal_co2.nc", "scaling=1.0 2.5")
SW_SPECTRA = LW_SPECTRA[:1] + ("input=ideal_h2o.nc ideal_o3.nc", "scaling=1.0 2.5", "ssi=ssi.nc", "cos_solar_zenith_angle=0.3 0.5 0.8")
# (directory, tool, arguments, output files; a *.h5 output is compared under the names of the classic file named after it)
RUNS = [
    ("lw", "ckdmip_lw", ("--merge-only", *LW_GASES, "--output", "merged.nc"), ["merged.nc"]),
    ("lw", "ckdmip_lw", ("--config", "lw_b.nam", "--scenario", "test-1", "--column-range", "2", "3", *LW_GASES, "--output", "lbl_b.nc"), ["lbl_b.nc"]),
    ("lw", "ckdmip_lw", ("--config", "lw4.nam", *LW_GASES, "--output", "lbl_4.nc"), ["lbl_4.nc"]),
    ("lw", "ckdmip_lw", ("--scenario", "present", "--ckd", "od.nc", "--output", "fluxes.nc"), ["fluxes.nc"]),
    ("lw", "ckdmip_lw", ("--config", "ckd4.nam", "--scenario", "present", "--ckd", "od.nc", "--output", "fluxes4.nc"), ["fluxes4.nc"]),
    ("lw", "ckdmip_lw", ("--config", "lw_b.nam", "--scenarios", "table.txt", "ideal_h2o.nc", "ideal_co2.nc"), ["scen_a.nc", "scen_b.nc", "scen_c.nc"]),
    ("sw", "ckdmip_sw", ("--merge-only", "ideal_h2o.nc", "--scale", "2", "ideal_o3.nc", "--output", "merged.nc"), ["merged.nc"]),
    ("sw", "ckdmip_sw", ("--config", "sw_b.nam", "--scenario", "present", "--ssi", "ssi.nc", *SW_GASES, "--output", "lbl_sw_b.nc"), ["lbl_sw_b.nc"]),
    ("sw", "ckdmip_sw", ("--config", "sw_b.nam", "--ssi", "ssi.nc", "--rayleigh", "rayleigh.nc", *SW_GASES, "--output", "lbl_ray.nc"), ["lbl_ray.nc"]),
    ("sw", "ckdmip_sw", ("--config", "sw.nam", "--ckd", "od_sw.nc", "--output", "fluxes_sw.nc"), ["fluxes_sw.nc"]),
    ("sw", "ckdmip_sw", ("--config", "sw.nam", "--ckd", "od_sw.nc", "--rayleigh-scattering", "--output", "fluxes_ray.nc"), ["fluxes_ray.nc"]),
    ("sw", "ckdmip_sw", ("--config", "sw_b.nam", "--ssi", "ssi.nc", "--scenarios", "table.txt", "ideal_h2o.nc", "ideal_o3.nc"), ["scen_a.nc", "scen_b.nc", "scen_c.nc"]),
    ("lw", "lw_spectra", (*LW_SPECTRA, "output=spectra.nc"), ["spectra.nc"]),
    ("lw", "lw_spectra", (*LW_SPECTRA, "gpoints=gpoints.nc", "output=spectra_g.nc"), ["spectra_g.nc"]),
    ("lw", "lw_spectra", (*LW_SPECTRA, "iprofile=1", "output=spectra_1.nc"), ["spectra_1.nc"]),
    ("lw", "lw_spectra", (*LW_SPECTRA, "output=spectra.h5"), ["spectra.h5"]),
    ("sw", "sw_spectra", (*SW_SPECTRA, "output=spectra.nc"), ["spectra.nc"]),
    ("sw", "sw_spectra", (*SW_SPECTRA, "gpoints=gpoints.nc", "output=spectra_g.nc"), ["spectra_g.nc"]),
    ("sw", "sw_spectra", (*SW_SPECTRA, "iprofile=1", "output=spectra_1.nc"), ["spectra_1.nc"]),
    ("sw", "sw_spectra", (*SW_SPECTRA, "output=spectra.h5"), ["spectra.h5"]),
]
REFUSED = [
    ("sw", "ckdmip_sw", ("--merge-only", "--rayleigh", "rayleigh.nc", "ideal_h2o.nc", "--output", "x.nc")),
    ("sw", "ckdmip_lw", ("--ckd", "od.nc", "--rayleigh-scattering", "--output", "x.nc")),
    ("sw", "sw_spectra", ("append_path=.", "input=ideal_h2o.nc", "output=x.nc")),                                  # no ssi
    ("sw", "sw_spectra", (*SW_SPECTRA[:-1], "cos_solar_zenith_angle=1.5", "output=x.nc")),
]
TIME_LIMIT = 120      # seconds per tool run; each takes a few at these sizes

SW_FIND_G = ("averaging_method=total-transmission", "sw.cfg")
# (directory, arguments, output file, number of processes)
FIND_G_RUNS = [
    ("find_g/lw", ("find_g.cfg", "output=plain.nc"), "plain.nc", 1),
    ("find_g/lw", ("find_g.cfg", "output=seq.nc", "sequential_bands=1"), "seq.nc", 1),
    ("find_g/lw", ("find_g.cfg", "output=after.nc", "gases_side_by_side=1"), "after.nc", 1),
    ("find_g/lw", ("g_split.cfg", "output=g_split.nc"), "g_split.nc", 1),
    ("find_g/lw", ("base_split.cfg", "output=base_split.nc"), "base_split.nc", 1),
    ("find_g/lw", ("base_boundary.cfg", "output=base_boundary.nc"), "base_boundary.nc", 1),
    ("find_g/lw", ("find_g.cfg", "output=target.nc", "target_g_points=12"), "target.nc", 1),
    ("find_g/lw", ("find_g.cfg", "output=plain.h5"), "plain.h5", 1),
    ("find_g/sw", (*SW_FIND_G, "output=gpoints_sw.nc"), "gpoints_sw.nc", 1),
    ("find_g/cloud", ("g.cfg", "output=gpoints_cloud.nc"), "gpoints_cloud.nc", 1),
    ("find_g/lw", ("find_g.cfg", "output=two.nc", "part_timeout=300"), "two.nc", 2),
    ("find_g/lw", ("base_boundary.cfg", "output=base_boundary_two.nc", "part_timeout=300"), "base_boundary_two.nc", 2),
    ("find_g/sw", (*SW_FIND_G, "output=two.nc", "part_timeout=300"), "two.nc", 2),
]
FIND_G_REFUSED = [
    ("find_g/lw", ("find_g.cfg",)),                                                                  # no output
    ("find_g/lw", ("no_tolerance.cfg", "output=x.nc")),
    ("find_g/lw", ("find_g.cfg", "output=x.nc", "averaging_method=cubic")),
    ("find_g/cloud", ("lw.cfg", "output=x.nc")),                                                     # cloud without ssi
    ("find_g/lw", ("find_g.cfg", "output=x.nc", "target_g_points=12", "sequential_bands=1")),
    ("find_g/lw", ("find_g.cfg", "output=x.nc", "heating_rate_tolerance=0.08 0.08 0.08")),          # three for two bands
]


def write_inputs(work):
    import torch  # noqa: F401
    from ecckd_amd import api, synthetic as syn
    from test_pipeline_gpu import make_do_all_inputs, make_optimize_files
    from test_cli_gpu import _write_columns_from
    lw, sw = work / "lw", work / "sw"
    lw.mkdir(); sw.mkdir()
    table = "# name output spec per file\na scen_a.nc asis asis\nb scen_b.nc scale=0.5 const=6e-4\nc scen_c.nc conc=2e-3 scale=2\n"
    with api.Context(0) as ctx:
        make_do_all_inputs(ctx, lw)
        model, _, scenes, _, _, names = make_optimize_files(ctx, lw)
    nam = ("&longwave_config\noptical_depth_name = \"optical_depth\",\nnspectralstride = 1,\nnangle = NANGLE,\n"
           "do_write_spectral_boundary_fluxes = BOUNDARY,\nband_wavenumber1(1:2) = 0, 1300,\nband_wavenumber2(1:2) = 1300, 3260,\niverbose = 3\n/\n")
    (lw / "lw_b.nam").write_text(nam.replace("NANGLE", "0").replace("BOUNDARY", "true"))
    (lw / "lw4.nam").write_text(nam.replace("NANGLE", "4").replace("BOUNDARY", "false"))
    (lw / "ckd4.nam").write_text("&longwave_config\noptical_depth_name = \"optical_depth\",\nnangle = 4,\niverbose = 3\n/\n")
    (lw / "table.txt").write_text(table)
    sc = scenes[0]                                     # od.nc: what run_ckd (not a tool under comparison) writes for raw.nc
    ncol, nhl = sc["pressure_hl"].shape
    w = netcdf_file(str(lw / "conc.nc"), "w", version=2)
    for dim, n in (("column", ncol), ("half_level", nhl), ("level", nhl - 1)):
        w.createDimension(dim, n)
    w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = sc["pressure_hl"]
    w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = sc["temperature_hl"]
    for i, g in enumerate(model["gases"]):
        if g["conc"] != "none":
            w.createVariable(names[i] + "_mole_fraction_fl", "d", ("column", "level"))[:] = sc["vmr_fl"][:, i, :]
    w.close()
    subprocess.run([str(ROOT / "bin" / "run_ckd"), "ckd_model=raw.nc", "input=conc.nc", "output=od.nc"], cwd=lw, check=True, timeout=TIME_LIMIT)

    nlay, nwav, lo, hi = 16, 8000, 250.0, 50000.0      # the shortwave files of test_ckdmip_sw_stand_in
    p1 = syn.pressure_grid(nlay)
    wn, dwn = syn.wavenumber_grid(nwav, lo, hi)
    w = netcdf_file(str(sw / "ssi.nc"), "w", version=2)
    w.createDimension("wavenumber", nwav)
    w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = syn.solar_spectral_irradiance(wn, dwn)
    w.close()
    t0 = syn.temperature_profile(p1)
    for g, seed, nlines, scale, vmr in (("h2o", 81, 60, 3.0, 5e-3), ("o3", 83, 30, 0.8, 1e-6)):
        od = syn.optical_depth(np, p1, wn, syn.SEED_BASE + seed, nlines=nlines, column_scale=scale, dtype="float32", lo=lo, hi=hi)
        _write_columns_from(sw / f"ideal_{g}.nc", g, p1, [t0 - 20.0, t0, t0 + 20.0], wn, od, vmr)
    ray = 0.3 * (wn / hi) ** 4 * np.linspace(0.5, 1.5, nlay)[:, None]
    _write_columns_from(sw / "rayleigh.nc", "rayleigh", p1, [t0 - 20.0, t0, t0 + 20.0], wn, ray, 1.0)
    nam = ("&shortwave_config\noptical_depth_name = \"optical_depth\",\nsurf_albedo = 0.15,\nuse_mu0_dimension = true,\n"
           "cos_solar_zenith_angle(1:5) = 0.1, 0.3, 0.5, 0.7, 0.9,\nnspectralstride = 1,\nBOUNDARY"
           "band_wavenumber1(1:2) = 250, 10000,\nband_wavenumber2(1:2) = 10000, 50000,\niverbose = 3\n/\n")
    (sw / "sw.nam").write_text(nam.replace("BOUNDARY", ""))
    (sw / "sw_b.nam").write_text(nam.replace("BOUNDARY", "do_write_spectral_boundary_fluxes = true,\n"))
    (sw / "table.txt").write_text(table.replace("const=6e-4", "scale=3"))
    rs = np.random.RandomState(5)                      # od_sw.nc of the --ckd tests
    ncol, ng = 2, 7
    w = netcdf_file(str(sw / "od_sw.nc"), "w", version=2)
    for dim, n in (("column", ncol), ("half_level", nlay + 1), ("level", nlay), ("g_point", ng)):
        w.createDimension(dim, n)
    w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p1, (ncol, 1))
    w.createVariable("optical_depth", "d", ("column", "level", "g_point"))[:] = rs.uniform(0.0, 0.4, (ncol, nlay, ng))
    w.createVariable("rayleigh_optical_depth", "d", ("column", "level", "g_point"))[:] = rs.uniform(0.0, 0.05, (ncol, nlay, ng))
    w.createVariable("incoming_sw", "d", ("column", "g_point"))[:] = rs.uniform(10.0, 300.0, (ncol, ng))
    w.close()
    rng = np.random.default_rng(3)                     # g points: 12 of them, 5 % of the points at none
    for d in (lw, sw):
        g_point = rng.integers(0, 12, size=nwav).astype(np.int32)
        g_point[rng.random(nwav) < 0.05] = -1
        w = netcdf_file(str(d / "gpoints.nc"), "w", version=2)
        w.createDimension("wavenumber", nwav)
        w.createVariable("g_point", "i", ("wavenumber",))[:] = g_point
        w.close()


def write_find_g_inputs(work):
    """find_g/lw, find_g/sw, find_g/cloud: what the find_g_points tool tests run on, with their orderings (this tree's
    reorder_spectrum and reorder_cloud_spectrum, which are not under comparison)"""
    from ecckd_amd import synthetic as syn
    from test_pipeline_gpu import NLAY, _write_spectrum
    from test_cli_gpu import LW_CFG, _make_lw_files
    from test_cloud_gpu import CLOUD_CFG, GASES_CFG, _sw_case

    def tool(d, name, *words):
        subprocess.run([str(ROOT / "bin" / name), *words], cwd=d, check=True, capture_output=True, timeout=TIME_LIMIT)

    lw, sw, cloud = work / "find_g" / "lw", work / "find_g" / "sw", work / "find_g" / "cloud"
    for d in (lw, sw, cloud):
        d.mkdir(parents=True)
    _make_lw_files(lw)
    os.symlink(lw / "h2o.nc", lw / "co2_bg_is_h2o.nc")
    for g in ("h2o", "co2"):
        tool(lw, "reorder_spectrum", f"input={g}.nc", f"output=order_{g}.nc", "wavenumber1=0 1300", "wavenumber2=1300 3260")
        # for the base splits: the first band from 0, as asked for (tests/test_cli_gpu.py::_start_first_band_at_zero)
        shutil.copy(lw / f"order_{g}.nc", lw / f"order0_{g}.nc")
        f = netcdf_file(str(lw / f"order0_{g}.nc"), "a")
        f.variables["wavenumber1_band"][0] = 0.0
        f.close()
    cfg = LW_CFG.format(d=".")
    after_bg, from_zero = "  background_input \"co2.nc\"\n", cfg.replace("order_", "order0_")
    (lw / "find_g.cfg").write_text(cfg)
    (lw / "g_split.cfg").write_text(cfg.replace(after_bg, after_bg + "  g_split 0 0.7\n  subband_wavenumber_boundary 2000 2600\n"))
    (lw / "base_split.cfg").write_text(from_zero.replace("  min_g_points 2 1\n", "  min_g_points 2 1\n  base_split 1 0.5\n"))
    (lw / "base_boundary.cfg").write_text(from_zero.replace("  min_g_points 2 1\n", "  min_g_points 2 1\n  base_wavenumber_boundary 700\n"))
    (lw / "no_tolerance.cfg").write_text(cfg.replace("heating_rate_tolerance 0.08\n", ""))
    for name in ("g_split", "base_split", "base_boundary", "no_tolerance"):
        assert (lw / f"{name}.cfg").read_text() not in (cfg, from_zero), name

    nwav, lo, hi = 16000, 250.0, 50000.0                # the shortwave files of test_find_g_points_sw
    p = syn.pressure_grid(NLAY)
    wn, dwn = syn.wavenumber_grid(nwav, lo, hi)
    w = netcdf_file(str(sw / "ssi.nc"), "w", version=2)
    w.createDimension("wavenumber", nwav)
    w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = syn.solar_spectral_irradiance(wn, dwn)
    w.close()
    for g, (seed, scale, vmr) in {"h2o": (61, 5.0, 5e-3), "o3": (67, 1.5, 1e-6)}.items():
        od = syn.optical_depth(np, p, wn, syn.SEED_BASE + seed, nlines=40, column_scale=scale, dtype="float32", lo=lo, hi=hi)
        _write_spectrum(sw / f"{g}.nc", g, p, syn.temperature_profile(p), wn, od, vmr)
        tool(sw, "reorder_spectrum", f"input={g}.nc", f"output=order_{g}.nc", "ssi=ssi.nc", "wavenumber1=250 10000", "wavenumber2=10000 50000")
    (sw / "sw.cfg").write_text("ssi ssi.nc\naveraging_method transmission\nheating_rate_tolerance 0.03\nmax_iterations 40\ngases h2o o3\n"
                               "\\begin h2o\n input h2o.nc\n reordering_input order_h2o.nc\n background_input o3.nc\n\\end h2o\n"
                               "\\begin o3\n input o3.nc\n reordering_input order_o3.nc\n background_input h2o.nc\n max_scaling 3.0\n\\end o3\n")

    _sw_case(cloud)                                     # the inputs of test_find_g_points_with_cloud
    b1, b2 = "250 2500 10000 25000", "2500 10000 25000 50000"
    for g in ("h2o", "o3"):
        tool(cloud, "reorder_spectrum", f"input=present_{g}.nc", f"output=order_{g}.nc", "ssi=ssi.nc", f"wavenumber1={b1}", f"wavenumber2={b2}")
    tool(cloud, "reorder_cloud_spectrum", "input=mie.nc", "isize=1", "wavenumber_input=ssi.nc", "output=order_cloud.nc", f"wavenumber1={b1}",
         f"wavenumber2={b2}")
    with_cloud = CLOUD_CFG.format(order="order_cloud.nc", rng=0.1)
    (cloud / "g.cfg").write_text(GASES_CFG.format(ext="nc") + with_cloud)
    (cloud / "lw.cfg").write_text(GASES_CFG.format(ext="nc").replace("ssi ssi.nc\n", "") + with_cloud)


def run_find_g(tree, d, words, world):
    """find_g_points of `tree` as `world` processes on device 0 -> [(exit code, stdout, stderr) per rank]"""
    env = {k: v for k, v in os.environ.items() if k != "ECCKD_LOG_TIMES"}
    if world > 1:
        env.update(WORLD_SIZE=str(world), ECCKD_DEVICE="0")
    procs = [subprocess.Popen([str(tree / "bin" / "find_g_points"), *words], cwd=d, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)) if world > 1 else env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            out, err = p.communicate(timeout=TIME_LIMIT)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, out, err))
    return outs


def compare_find_g(work, trees):
    """-> number of differences, or None when a run that must succeed did not (nothing more is run then)"""
    bad = 0
    for d, words, output, world in FIND_G_RUNS:
        got = {}
        for tag, tree in trees.items():
            got[tag] = run_find_g(tree, work / d, words, world)
            if any(rc != 0 for rc, _, _ in got[tag]):
                print(f"{tag} find_g_points {' '.join(words)} ({world} process(es)): exit {[rc for rc, _, _ in got[tag]]}\n" + "\n".join(e for _, _, e in got[tag]))
                return None
            (work / d / tag).mkdir(exist_ok=True)
            shutil.move(str(work / d / output), str(work / d / tag / output))
        diffs = compare(work / d / "parent" / output, work / d / "branch" / output, work / d / "parent" / (output[:-3] + ".nc"))
        diffs += [f"stdout of rank {r} differs" for r in range(world) if got["parent"][r][1] != got["branch"][r][1]]
        if [f for f in os.listdir(work / d) if ".part" in f]:
            diffs.append("part files left behind")
        print(f"find_g_points {' '.join(words)} ({world} process(es)) -> {output} and stdout: {'identical' if not diffs else 'DIFFERS'}")
        for line in diffs:
            print("    " + line[:300])
        bad += bool(diffs)
    for d, words in FIND_G_REFUSED:
        got = {tag: run_find_g(tree, work / d, words, 1)[0] for tag, tree in trees.items()}
        for tag, (rc, _, err) in got.items():
            if rc < 0:                                  # killed by a signal: nothing more runs on this device
                print(f"{tag} find_g_points {' '.join(words)}: exit {rc}\n{err}")
                return None
        same = got["parent"][0] == got["branch"][0] > 0 and got["parent"][2] == got["branch"][2] and not (work / d / "x.nc").exists()
        print(f"find_g_points {' '.join(words)} (refused, exit {got['parent'][0]}: {got['parent'][2].strip()[:80]}): {'identical' if same else 'DIFFERS'}")
        if not same:
            print(f"    parent {got['parent']}\n    branch {got['branch']}")
        bad += not same
    return bad


def global_att(name, value):
    """A global attribute without what names the executable: None for `history`, `config` without its `0=<argv[0]>; `"""
    if name == "history" or value is None:
        return None
    text = value.decode() if isinstance(value, bytes) else value
    return text.split("; ", 1)[-1] if name == "config" and text.startswith("0=") else text


def classic(path):
    """What scipy reads of a classic file, or None for another format"""
    with open(path, "rb") as f:
        if f.read(3) != b"CDF":
            return None
    f = netcdf_file(str(path), "r", mmap=False)
    out = dict(dims=list(f.dimensions.items()), atts={k: global_att(k, v) for k, v in f._attributes.items()},
               vars=[(n, v.typecode(), v.dimensions, dict(v._attributes), v.data.tobytes()) for n, v in f.variables.items()])
    f.close()
    return out


def through_ncfile(path, names):
    from ecckd_amd.ncio import NcFile
    with NcFile(path) as f:
        out = dict(dims=[(d, f.dim(d)) for d in names["dims"]], atts=[(a, global_att(a, f.att_text(a))) for a in names["atts"]], vars=[])
        for v, atts in names["vars"]:
            out["vars"].append((v, f.var_info(v), f.read(v).tobytes(), [(a, f.att_text(a, v)) for a in atts]))
    return out


def compare(a, b, twin_a):
    """-> list of differences between the files a and b; twin_a: the classic file whose names a *.h5 pair is read under"""
    bad = []
    ca, cb = classic(a), classic(b)
    if (ca is None) != (cb is None):
        return ["one file is classic, the other is not"]
    if ca is not None:
        for key in ("dims", "atts"):
            if ca[key] != cb[key]:
                bad.append(f"{key}: {ca[key]} != {cb[key]}")
        if [v[:4] for v in ca["vars"]] != [v[:4] for v in cb["vars"]]:
            bad.append("variable names, order, types, dimensions or attributes differ")
        bad += [f"bytes of {va[0]} differ" for va, vb in zip(ca["vars"], cb["vars"]) if va[4] != vb[4]]
    ref = ca if ca is not None else classic(twin_a)
    names = dict(dims=[d for d, _ in ref["dims"]], atts=list(ref["atts"]), vars=[(v[0], list(v[3])) for v in ref["vars"]])
    na, nb = through_ncfile(a, names), through_ncfile(b, names)
    for key in ("dims", "atts"):
        if na[key] != nb[key]:
            bad.append(f"NcFile {key}: {na[key]} != {nb[key]}")
    bad += [f"NcFile: {va[0]} differs" for va, vb in zip(na["vars"], nb["vars"]) if va != vb]
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent", type=pathlib.Path)
    ap.add_argument("branch", type=pathlib.Path)
    ap.add_argument("--work", type=pathlib.Path, help="working directory to keep (default: a temporary one)")
    args = ap.parse_args()
    trees = {"parent": args.parent.resolve(), "branch": args.branch.resolve()}
    tmp = None if args.work else tempfile.TemporaryDirectory()
    work = (args.work or pathlib.Path(tmp.name)).resolve()
    work.mkdir(parents=True, exist_ok=True)
    write_inputs(work)
    write_find_g_inputs(work)
    bad = 0
    for d, tool, words, outputs in RUNS:
        for tag, tree in trees.items():
            r = subprocess.run([str(tree / "bin" / tool), *words], cwd=work / d, capture_output=True, text=True, timeout=TIME_LIMIT)
            if r.returncode != 0:
                print(f"{tag} {tool} {' '.join(words)}: exit {r.returncode}\n{r.stderr}")
                return 1
            (work / d / tag).mkdir(exist_ok=True)
            for o in outputs:
                shutil.move(str(work / d / o), str(work / d / tag / o))
        for o in outputs:
            twin = work / d / "parent" / (o[:-3] + ".nc")
            diffs = compare(work / d / "parent" / o, work / d / "branch" / o, twin)
            print(f"{tool} {' '.join(words)} -> {o}: {'identical' if not diffs else 'DIFFERS'}")
            for line in diffs:
                print("    " + line[:300])
            bad += bool(diffs)
    for d, tool, words in REFUSED:
        got = {}
        for tag, tree in trees.items():
            r = subprocess.run([str(tree / "bin" / tool), *words], cwd=work / d, capture_output=True, text=True, timeout=TIME_LIMIT)
            got[tag] = (r.returncode, r.stderr)
            if r.returncode < 0:                       # killed by a signal: nothing more runs on this device
                print(f"{tag} {tool} {' '.join(words)}: exit {r.returncode}\n{r.stderr}")
                return 1
        same = got["parent"] == got["branch"] and got["parent"][0] > 0 and not (work / d / "x.nc").exists()
        print(f"{tool} {' '.join(words)} (refused, exit {got['parent'][0]}): {'identical' if same else 'DIFFERS'}")
        if not same:
            print(f"    parent {got['parent']}\n    branch {got['branch']}")
        bad += not same
    more = compare_find_g(work, trees)
    if more is None:
        return 1
    bad += more
    print(f"{bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
