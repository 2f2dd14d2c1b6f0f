"""bin/optimize_lut optimize_rayleigh=1: the Rayleigh coefficients optimised by the tool, with and without
rayleigh_scattering=1, on the synthetic training files of tests/test_cli_optimize_rayleigh_gpu.py (its `files` recipe,
imported), and the chain of that file's test_chain_through_ckdmip_sw with a third training beside its two."""
import re

import numpy as np
import pytest
from scipy.io import netcdf_file

from ecckd_amd import synthetic as syn
from test_cli_gpu import _nc, _write_columns_from, run_tool
from test_cli_optimize_rayleigh_gpu import KEYS, PARAMETER_ERROR, _rayleigh_optical_depth, _write_training_columns, files  # noqa: F401

pytestmark = pytest.mark.gpu

RAYLEIGH = "rayleigh_molar_scattering_coeff"


def _variables(path):
    f = _nc(path)
    out = {k: (v[...].copy(), v.typecode()) for k, v in f.variables.items()}
    f.close()
    return out


@pytest.mark.parametrize("scattering", [False, True])
def test_the_key_optimises_the_coefficient(ctx, files, scattering):
    from ecckd_amd import ncio, pipeline
    d, raw = files["d"], files["raw"]
    tag = "ray" if scattering else "plain"
    extra = ("rayleigh_scattering=1",) if scattering else ()
    r = run_tool("optimize_lut", "input=raw_sw.nc", f"output=act_{tag}.nc", "training_input=lbl_ray.nc", "optimize_rayleigh=1",
                 "rayleigh_prior_error=1.0", *extra, *KEYS, "max_iterations=40", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    log = r.stdout + r.stderr
    assert "Optimizing Rayleigh scattering coefficients with prior error of 1" in log      # the reference's line (optimize_lut.cpp:135)
    cost = [float(x) for x in re.findall(r"Iteration \d+: cost function = ([0-9.eE+-]+)", log)]
    assert len(cost) > 3 and cost[-1] < cost[0], cost
    a, b = _variables(d / "raw_sw.nc"), _variables(d / f"act_{tag}.nc")
    assert set(a) == set(b)                                                                # nothing else about the file changes
    k0, k1 = a[RAYLEIGH][0], b[RAYLEIGH][0]
    assert b[RAYLEIGH][1] == "f" and k1.shape == k0.shape and np.all(k1 > 0) and np.all(np.isfinite(k1))
    assert not np.array_equal(k0, k1)
    assert not np.array_equal(a["h2o_molar_absorption_coeff"][0], b["h2o_molar_absorption_coeff"][0])
    # the state is the gases' elements and ng more
    ng = k0.size
    n_plain = int(re.search(r"Optimizing (\d+) coefficients", (run_tool("optimize_lut", "input=raw_sw.nc", "output=tmp.nc", "training_input=lbl_ray.nc",
                                                                         *extra, *KEYS, "max_iterations=1", cwd=d).stdout)).group(1))
    assert int(re.search(r"Optimizing (\d+) coefficients", log).group(1)) == n_plain + ng
    # the host mirror on the same file gives the same coefficients
    opt, res = pipeline.optimize_lut(ctx, raw, [str(d / "lbl_ray.nc")], max_iterations=40, rayleigh_scattering=scattering,
                                     optimize_rayleigh=True, rayleigh_prior_error=1.0, max_no_rayleigh_wavenumber=10000.0,
                                     prior_error=2.0, broadband_weight=0.4, flux_weight=0.3,
                                     flux_profile_weight=0.05, temperature_corr=0.8, pressure_corr=0.8, conc_corr=0.8,
                                     min_prior_error=-1.0, max_prior_error=-1.0)
    assert np.array_equal(np.asarray(opt["rayleigh_molar_scattering"]).astype(np.float32), k1)
    # without a prior the tool says so
    r = run_tool("optimize_lut", "input=raw_sw.nc", "output=tmp.nc", "training_input=lbl_ray.nc", "optimize_rayleigh=1", *extra, *KEYS,
                 "max_iterations=2", cwd=d)
    assert r.returncode == 0 and "Optimizing Rayleigh scattering coefficients without a prior" in r.stdout + r.stderr


@pytest.mark.parametrize("options", [(), ("relative_to=lbl_ray.nc",), ("remove_min_max=1", "bounded_minimization=0")])
def test_gases_rayleigh_leaves_every_gas_table_alone(ctx, files, options):
    d = files["d"]
    r = run_tool("optimize_lut", "input=raw_sw.nc", "output=only.nc", "training_input=lbl_ray.nc", "gases=rayleigh", "optimize_rayleigh=1",
                 *options, *KEYS, "max_iterations=25", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    log = r.stdout + r.stderr
    assert 'gas "rayleigh" is not in' not in log
    a, b = _variables(d / "raw_sw.nc"), _variables(d / "only.nc")
    ng = a[RAYLEIGH][0].size
    assert int(re.search(r"Optimizing (\d+) coefficients", log).group(1)) == ng
    for name, (v, tc) in a.items():
        if name.endswith("_molar_absorption_coeff"):
            assert np.array_equal(v, b[name][0]) and b[name][1] == tc, name
    if "relative_to=lbl_ray.nc" not in options:           # (fitted relative to the training file itself there is nothing to fit)
        assert not np.array_equal(a[RAYLEIGH][0], b[RAYLEIGH][0])
    assert np.all(b[RAYLEIGH][0] > 0)
    assert ("h2o_molar_absorption_coeff_min" in b) == ("remove_min_max=1" not in options)


def test_refusals(ctx, files, tmp_path):
    d = files["d"]
    # rayleigh_prior_error > 0 without the key: as before
    r = run_tool("optimize_lut", "input=raw_sw.nc", "output=x.nc", "training_input=lbl_ray.nc", "rayleigh_prior_error=0.5", *KEYS, cwd=d)
    assert r.returncode == PARAMETER_ERROR and "rayleigh_prior_error > 0" in r.stderr and not (d / "x.nc").exists()
    # the name "rayleigh" in `gases` without the key: a name the model does not have, as before - warned about, the other gases
    # optimised, the coefficient untouched; alone it leaves no active gas
    r = run_tool("optimize_lut", "input=raw_sw.nc", "output=named.nc", "training_input=lbl_ray.nc", "gases=h2o rayleigh", *KEYS, "max_iterations=3", cwd=d)
    assert r.returncode == 0 and 'gas "rayleigh" is not in' in r.stderr + r.stdout, r.stderr + r.stdout
    assert "Optimizing Rayleigh scattering coefficients" not in r.stdout + r.stderr
    a, b = _variables(d / "raw_sw.nc"), _variables(d / "named.nc")
    assert np.array_equal(a[RAYLEIGH][0], b[RAYLEIGH][0])
    r = run_tool("optimize_lut", "input=raw_sw.nc", "output=x.nc", "training_input=lbl_ray.nc", "gases=rayleigh", *KEYS, cwd=d)
    assert r.returncode == PARAMETER_ERROR and "no active gas" in r.stderr and not (d / "x.nc").exists()
    # the key on a longwave model
    from ecckd_amd import ncio
    import ckd_synth
    lw = ckd_synth.make_model(seed=2)
    ng = lw["planck_function"].shape[1]
    ib, nband = lw["iband_per_g"], lw["nband"]
    first = np.array([np.nonzero(ib == b)[0][0] for b in range(nband)])
    last = np.array([np.nonzero(ib == b)[0][-1] for b in range(nband)])
    lw.update(wavenumber1=np.arange(ng) * 100.0, wavenumber2=np.arange(1, ng + 1) * 100.0, gpoint_fraction=np.eye(ng),
              wavenumber1_band=100.0 * first, wavenumber2_band=100.0 * (last + 1))
    ncio.write_ckd_model(str(d / "raw_lw.nc"), lw)
    r = run_tool("optimize_lut", "input=raw_lw.nc", "output=x.nc", "training_input=lbl_ray.nc", "optimize_rayleigh=1", *KEYS, cwd=d)
    assert r.returncode == PARAMETER_ERROR and "optimize_rayleigh" in r.stderr and not (d / "x.nc").exists()


# ---- the chain of test_chain_through_ckdmip_sw with a third training: two-stream transfer AND optimised Rayleigh coefficients ----
def test_chain_through_ckdmip_sw_with_optimised_rayleigh(ctx, tmp_path):
    """The chain of tests/test_cli_optimize_rayleigh_gpu.py::test_chain_through_ckdmip_sw, restated at the same size, with
    optimize_rayleigh=1 beside the two trainings that test runs.  Asserted is what that test asserts: a trained model's RMS
    error against the line-by-line file over the top-of-atmosphere upwelling and the surface total downwelling band fluxes
    is not above the raw model's.  The three trained errors are printed."""
    d = tmp_path
    nlay, nwav, lo, hi = 16, 8000, 250.0, 50000.0
    p1 = syn.pressure_grid(nlay)
    wn, dwn = syn.wavenumber_grid(nwav, lo, hi)
    ssi = syn.solar_spectral_irradiance(wn, dwn)
    w = netcdf_file(str(d / "ssi.nc"), "w", version=2)
    w.createDimension("wavenumber", nwav)
    w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = ssi
    w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
    w.createVariable("total_solar_irradiance", "d", ())[...] = ssi.sum()
    w.close()
    base = {"h2o": (syn.optical_depth(np, p1, wn, syn.SEED_BASE + 81, nlines=60, column_scale=3.0, dtype="float32", lo=lo, hi=hi), 5e-3),
            "o3": (syn.optical_depth(np, p1, wn, syn.SEED_BASE + 83, nlines=30, column_scale=0.8, dtype="float32", lo=lo, hi=hi), 1e-6)}
    t0 = syn.temperature_profile(p1)
    temps = [t0 - 20.0, t0, t0 + 20.0]
    for g, (od, vmr) in base.items():
        _write_columns_from(d / f"present_{g}.nc", g, p1, [t0], wn, od, vmr)
        _write_columns_from(d / f"ideal_{g}.nc", g, p1, temps, wn, od, vmr)
    _write_columns_from(d / "ideal_h2o_x4.nc", "h2o", p1, temps, wn, base["h2o"][0] * np.float32(4.0), base["h2o"][1] * 4.0)
    ncol, mu0s = 3, np.array([0.1, 0.3, 0.5, 0.7, 0.9])
    amount = {"h2o": np.array([0.7, 1.5, 3.0]), "o3": np.array([1.0, 2.0, 0.5])}
    for g, (od, vmr) in base.items():
        _write_training_columns(d / f"train_{g}.nc", g, p1, t0, wn, od[None].astype(np.float64) * amount[g][:, None, None], vmr * amount[g])
    _write_training_columns(d / "rayleigh.nc", "rayleigh", p1, t0, wn, np.tile(_rayleigh_optical_depth(p1, wn)[None], (ncol, 1, 1)), np.ones(ncol))
    nam = ("&shortwave_config\noptical_depth_name = \"optical_depth\",\nsurf_albedo = 0.15,\nuse_mu0_dimension = true,\n"
           "cos_solar_zenith_angle(1:5) = 0.1, 0.3, 0.5, 0.7, 0.9,\nnspectralstride = 1,\nBOUNDARY"
           "band_wavenumber1(1:2) = 250, 10000,\nband_wavenumber2(1:2) = 10000, 50000,\n/\n")
    (d / "sw.nam").write_text(nam.replace("BOUNDARY", ""))
    (d / "sw_b.nam").write_text(nam.replace("BOUNDARY", "do_write_spectral_boundary_fluxes = true,\n"))

    def ok(r):
        assert r.returncode == 0, r.stderr + r.stdout
        return r

    for g in base:
        ok(run_tool("reorder_spectrum", f"input=present_{g}.nc", f"output=order_{g}.nc", "ssi=ssi.nc", "wavenumber1=250 10000", "wavenumber2=10000 50000", cwd=d))
    (d / "g.cfg").write_text(
        "ssi ssi.nc\nheating_rate_tolerance 0.06\nmax_iterations 30\naveraging_method total-transmission\ngases h2o o3\n"
        "\\begin h2o\n input present_h2o.nc\n reordering_input order_h2o.nc\n background_input present_o3.nc\n\\end h2o\n"
        "\\begin o3\n input present_o3.nc\n reordering_input order_o3.nc\n background_input present_h2o.nc\n\\end o3\n")
    ok(run_tool("find_g_points", "g.cfg", "output=gpoints.nc", cwd=d))
    (d / "lut.cfg").write_text(
        "input gpoints.nc\noutput raw.nc\nssi ssi.nc\naveraging_method transmission-3\ngases h2o o3\n"
        "\\begin h2o\n conc_dependence lut\n input \"ideal_h2o.nc ideal_h2o_x4.nc\"\n\\end h2o\n"
        "\\begin o3\n conc_dependence linear\n input ideal_o3.nc\n\\end o3\n")
    ok(run_tool("create_look_up_table", "lut.cfg", cwd=d))
    ok(run_tool("ckdmip_sw", "--config", "sw_b.nam", "--scenario", "present", "--ssi", "ssi.nc", "--rayleigh", "rayleigh.nc", "train_h2o.nc",
                "train_o3.nc", "--output", "lbl_ray.nc", cwd=d))
    f = _nc(d / "lbl_ray.nc")
    truth_dn = f.variables["band_flux_dn_sw"][:, :, -1, :].astype(np.float64)          # (column, mu0, band): surface, direct + diffuse
    truth_up = f.variables["band_flux_up_sw"][:, :, 0, :].astype(np.float64)           # top of atmosphere
    f.close()

    keys = ("training_input=lbl_ray.nc", "gpointfile=gpoints.nc", "prior_error=2.0", "broadband_weight=0.4", "flux_weight=0.3",
            "flux_profile_weight=0.05", "spectral_boundary_weight=0.01", "max_iterations=60", "convergence_criterion=0")
    ok(run_tool("optimize_lut", "input=raw.nc", "output=ckd_plain.nc", *keys, cwd=d))
    ok(run_tool("optimize_lut", "input=raw.nc", "output=ckd_ray.nc", "rayleigh_scattering=1", *keys, cwd=d))
    r = ok(run_tool("optimize_lut", "input=raw.nc", "output=ckd_ray_opt.nc", "rayleigh_scattering=1", "optimize_rayleigh=1", "rayleigh_prior_error=1.0",
                    *keys, cwd=d))
    assert "Optimizing Rayleigh scattering coefficients with prior error of 1" in r.stdout + r.stderr
    a, b, c = _nc(d / "raw.nc"), _nc(d / "ckd_ray.nc"), _nc(d / "ckd_ray_opt.nc")
    band = a.variables["band_number"][...].astype(int)
    assert np.array_equal(a.variables[RAYLEIGH][...], b.variables[RAYLEIGH][...])
    assert not np.array_equal(a.variables[RAYLEIGH][...], c.variables[RAYLEIGH][...]) and np.all(c.variables[RAYLEIGH][...] > 0)
    print("ln(optimised / first-guess Rayleigh coefficient) per g point:", np.log(c.variables[RAYLEIGH][...] / a.variables[RAYLEIGH][...]))
    a.close(); b.close(); c.close()

    w = netcdf_file(str(d / "eval.nc"), "w", version=2)
    for dim, n in (("column", ncol), ("half_level", nlay + 1), ("level", nlay)):
        w.createDimension(dim, n)
    w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p1, (ncol, 1))
    w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = np.tile(t0, (ncol, 1))
    for g, (_, vmr) in base.items():
        w.createVariable(g + "_mole_fraction_fl", "d", ("column", "level"))[:] = np.tile((vmr * amount[g])[:, None], (1, nlay))
    w.close()
    rms = {}
    for tag in ("raw", "ckd_plain", "ckd_ray", "ckd_ray_opt"):
        ok(run_tool("run_ckd", f"ckd_model={tag}.nc", "input=eval.nc", f"output=od_{tag}.nc", f"tsi={ssi.sum()}", cwd=d))
        ok(run_tool("ckdmip_sw", "--config", "sw.nam", "--ckd", f"od_{tag}.nc", "--rayleigh-scattering", "--output", f"flux_{tag}.nc", cwd=d))
        f = _nc(d / f"flux_{tag}.nc")
        dn_g = f.variables["spectral_flux_dn_sw"][:, :, -1, :].astype(np.float64)      # (column, mu0, g_point)
        up_g = f.variables["spectral_flux_up_sw"][:, :, 0, :].astype(np.float64)
        f.close()
        dn = np.stack([dn_g[..., band == k].sum(-1) for k in range(2)], axis=-1)
        up = np.stack([up_g[..., band == k].sum(-1) for k in range(2)], axis=-1)
        rms[tag] = float(np.sqrt(np.mean(np.concatenate([(dn - truth_dn).ravel(), (up - truth_up).ravel()]) ** 2)))
    print("RMS error of TOA upwelling and surface total downwelling band fluxes (W m-2): no scattering %.4g, two-stream %.4g, "
          "two-stream with optimised Rayleigh %.4g (raw model %.4g)" % (rms["ckd_plain"], rms["ckd_ray"], rms["ckd_ray_opt"], rms["raw"]))
    assert np.isfinite(rms["raw"]) and rms["ckd_ray"] <= rms["raw"] and rms["ckd_ray_opt"] <= rms["raw"]
