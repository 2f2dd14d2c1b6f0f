"""bin/optimize_lut rayleigh_scattering=1.

test_chain_through_ckdmip_sw is the whole loop with the binaries only: `ckdmip_sw --rayleigh` writes the training file, the
tool trains on it, `run_ckd` + `ckdmip_sw --ckd --rayleigh-scattering` evaluate the raw and the trained model, and the trained
one is judged by the fluxes the optimiser minimises.

The other tests run on a synthetic scattering training file (the variables and the global attribute that `ckdmip_sw --rayleigh`
writes): the total downwelling is the truth, the band albedo comes from it, nothing is masked, the cost falls, and the result is
the host mirror's (pipeline.optimize_lut(rayleigh_scattering=True)) on the same files.  A file without the attribute is refused
by name, and rayleigh_scattering=0 is the key left out."""
import re

import numpy as np
import pytest
from scipy.io import netcdf_file

import ckd_synth
import opt_rayleigh_ref as orr
from ecckd_amd import synthetic as syn
from test_cli_gpu import _nc, _same_files, _write_columns_from, run_tool

pytestmark = pytest.mark.gpu

PARAMETER_ERROR = 147
NCOL, NLAY = 3, 12
MU0_FILE = np.array([0.9, 0.7, 0.5, 0.3, 0.1])
KEYS = ("prior_error=2.0", "broadband_weight=0.4", "flux_weight=0.3", "flux_profile_weight=0.05", "temperature_corr=0.8",
        "pressure_corr=0.8", "conc_corr=0.8", "convergence_criterion=0")


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    """raw_sw.nc, a shortwave definition with a Rayleigh coefficient, and two training files of a perturbed definition's
    scattering fluxes at five zenith angles over a surface of albedo 0.2: lbl_ray.nc as `ckdmip_sw --rayleigh` marks it,
    lbl_plain.nc with the same variables and no attribute"""
    from ecckd_amd import ncio
    d = tmp_path_factory.mktemp("optimize_rayleigh")
    model = ckd_synth.make_model_sw(seed=8)
    for g in model["gases"]:                      # every band keeps light at the surface: its albedo sum(up) / sum(dn) is defined
        for k in ("molar_abs", "min_molar_abs", "max_molar_abs"):
            g[k] = g[k] * 0.02
    ng, names = model["ng"], [g["name"] for g in model["gases"]]
    ib, nband = model["iband_per_g"], model["nband"]
    first = np.array([np.nonzero(ib == b)[0][0] for b in range(nband)])
    last = np.array([np.nonzero(ib == b)[0][-1] for b in range(nband)])
    model.update(wavenumber1=250.0 + np.arange(ng) * 400.0, wavenumber2=250.0 + np.arange(1, ng + 1) * 400.0, gpoint_fraction=np.eye(ng),
                 wavenumber1_band=250.0 + 400.0 * first, wavenumber2_band=250.0 + 400.0 * (last + 1))
    ncio.write_ckd_model(str(d / "raw_sw.nc"), model)
    raw = ncio.read_ckd_model(str(d / "raw_sw.nc"))
    truth = dict(raw, gases=[dict(g, molar_abs=g["molar_abs"] * np.exp(0.2 * np.random.RandomState(i).normal(size=g["molar_abs"].shape)))
                             for i, g in enumerate(raw["gases"])])
    base = ckd_synth.make_scenes(raw, nscene=1, ncol=NCOL, nlay=NLAY)[0]
    direct, dn, up = (np.empty((NCOL, 5, NLAY + 1, nband)) for _ in range(3))
    for k, mu in enumerate(MU0_FILE):
        sc = dict(base, gas_present=None, mu0=np.full(NCOL, mu), tsi=1361.0, albedo=np.full(nband, 0.2))
        o = orr.OracleRayleigh(oracle, truth, [sc], {})
        f3 = o.fluxes3(o.x0, sc)
        bands = lambda a: np.stack([a[..., ib == b].sum(-1) for b in range(nband)], axis=-1)
        direct[:, k], dn[:, k], up[:, k] = bands(f3[0]), bands(f3[0] + f3[1]), bands(f3[2])
    file_gases = [n for n in names if n != "composite"]
    vmr = np.stack([base["vmr_fl"][:, names.index(n), :] for n in file_gases], axis=1)
    for name, marked in (("lbl_ray.nc", True), ("lbl_plain.nc", False)):
        w = netcdf_file(str(d / name), "w", version=2)
        for dim, n in (("column", NCOL), ("mu0", 5), ("half_level", NLAY + 1), ("level", NLAY), ("gas", len(file_gases)), ("band", nband)):
            w.createDimension(dim, n)
        for var, dims, a in (("mu0", ("mu0",), MU0_FILE), ("pressure_hl", ("column", "half_level"), base["pressure_hl"]),
                             ("temperature_hl", ("column", "half_level"), base["temperature_hl"]),
                             ("mole_fraction_fl", ("column", "gas", "level"), vmr),
                             ("flux_dn_direct_sw", ("column", "mu0", "half_level"), direct.sum(-1)),
                             ("flux_dn_sw", ("column", "mu0", "half_level"), dn.sum(-1)), ("flux_up_sw", ("column", "mu0", "half_level"), up.sum(-1)),
                             ("band_flux_dn_direct_sw", ("column", "mu0", "half_level", "band"), direct),
                             ("band_flux_dn_sw", ("column", "mu0", "half_level", "band"), dn),
                             ("band_flux_up_sw", ("column", "mu0", "half_level", "band"), up),
                             ("band_wavenumber1_sw", ("band",), model["wavenumber1_band"]), ("band_wavenumber2_sw", ("band",), model["wavenumber2_band"])):
            w.createVariable(var, "d", dims)[:] = a
        w.constituent_id = " ".join(file_gases)
        if marked:
            w.rayleigh_scattering = "two-stream"
        w.close()
    return dict(d=d, raw=raw, limit=float(model["wavenumber2_band"][nband // 2]))


def test_scattering_training_run(ctx, files):
    from ecckd_amd import ncio, pipeline
    d, raw = files["d"], files["raw"]
    r = run_tool("optimize_lut", "input=raw_sw.nc", "output=opt_ray.nc", "training_input=lbl_ray.nc", "rayleigh_scattering=1", *KEYS,
                 "max_iterations=40", f"max_no_rayleigh_wavenumber={files['limit']}", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "max_no_rayleigh_wavenumber" in r.stdout + r.stderr and "ignored" in r.stdout + r.stderr
    cost = [float(x) for x in re.findall(r"Iteration \d+: cost function = ([0-9.eE+-]+)", r.stdout + r.stderr)]
    assert len(cost) > 3 and cost[-1] < cost[0], cost
    opt, res = pipeline.optimize_lut(ctx, raw, [str(d / "lbl_ray.nc")], max_iterations=40, rayleigh_scattering=True,
                                     max_no_rayleigh_wavenumber=files["limit"], prior_error=2.0, broadband_weight=0.4, flux_weight=0.3,
                                     flux_profile_weight=0.05, temperature_corr=0.8, pressure_corr=0.8, conc_corr=0.8,
                                     min_prior_error=-1.0, max_prior_error=-1.0)
    assert res["status"] in (0, 2, 3) and res["iterations"] > 3
    ncio.write_ckd_model(str(d / "py_ray.nc"), opt)
    _same_files(d / "opt_ray.nc", d / "py_ray.nc")
    assert any(not np.array_equal(a["molar_abs"], b["molar_abs"]) for a, b in zip(opt["gases"], raw["gases"]))
    # the plain training on the same file reads the direct beam and masks: another result
    r = run_tool("optimize_lut", "input=raw_sw.nc", "output=opt_plain.nc", "training_input=lbl_ray.nc", *KEYS, "max_iterations=40",
                 f"max_no_rayleigh_wavenumber={files['limit']}", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    a, b = _nc(d / "opt_ray.nc"), _nc(d / "opt_plain.nc")
    assert not np.array_equal(a.variables["h2o_molar_absorption_coeff"][...], b.variables["h2o_molar_absorption_coeff"][...])
    a.close(); b.close()


def test_a_file_without_the_attribute_is_refused(ctx, files):
    d = files["d"]
    r = run_tool("optimize_lut", "input=raw_sw.nc", "output=x.nc", "training_input=lbl_plain.nc", "rayleigh_scattering=1", *KEYS, cwd=d)
    assert r.returncode == PARAMETER_ERROR and "lbl_plain.nc" in r.stderr and "rayleigh_scattering" in r.stderr
    assert not (d / "x.nc").exists()
    r = run_tool("optimize_lut", "input=raw_sw.nc", "output=x.nc", "training_input=lbl_ray.nc", "relative_to=lbl_plain.nc",
                 "rayleigh_scattering=1", *KEYS, cwd=d)
    assert r.returncode == PARAMETER_ERROR and "lbl_plain.nc" in r.stderr


def test_the_key_at_zero_is_the_key_left_out(ctx, files):
    """every variable of the output bit for bit (the global attributes `history` and `config` record the command line itself)"""
    d = files["d"]
    for out, extra in (("off.nc", ("rayleigh_scattering=0",)), ("absent.nc", ())):
        r = run_tool("optimize_lut", "input=raw_sw.nc", f"output={out}", "training_input=lbl_plain.nc", *extra, *KEYS, "max_iterations=15", cwd=d)
        assert r.returncode == 0, r.stderr + r.stdout
    _same_files(d / "off.nc", d / "absent.nc")


# ---- the chain: ckdmip_sw --rayleigh -> optimize_lut rayleigh_scattering=1 -> run_ckd -> ckdmip_sw --ckd --rayleigh-scattering ----
def _write_training_columns(path, gas, p1, t0, wn, od, vmr):
    """A spectral file of od (ncol, nlay, nwav) with one mole fraction per column, as FLOAT like the CKDMIP spectra"""
    ncol, nlay = od.shape[:2]
    w = netcdf_file(str(path), "w", version=2)
    for dim, n in (("column", ncol), ("half_level", nlay + 1), ("level", nlay), ("wavenumber", wn.size)):
        w.createDimension(dim, n)
    w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p1, (ncol, 1))
    w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = np.tile(t0, (ncol, 1))
    w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
    w.createVariable("mole_fraction_fl", "d", ("column", "level"))[:] = np.tile(np.asarray(vmr, dtype=np.float64)[:, None], (1, nlay))
    w.createVariable("optical_depth", "f", ("column", "level", "wavenumber"))[:] = od.astype(np.float32)
    w.createVariable("reference_surface_mole_fraction", "d", ())[...] = float(np.mean(vmr))
    w.constituent_id = gas
    w.close()


def _rayleigh_optical_depth(p1, wn):
    """Bucholtz (1995) cross-section per molecule times the molecules of each layer (nlay, nwav): the physics from which
    create_look_up_table makes the model's Rayleigh coefficient, so that the line-by-line truth and the model scatter alike"""
    um = 10000.0 / wn
    xs = np.where(um < 0.5, 3.01577e-32 * um ** -(3.55212 + 1.35579 * um + 0.11563 / um),
                  4.01061e-32 * um ** -(3.99668 + 0.00110298 * um + 0.0271393 / um))
    return ((p1[1:] - p1[:-1]) * orr.MOLES_PER_PA)[:, None] * (xs * 6.02214076e23)[None, :]


def test_chain_through_ckdmip_sw(ctx, tmp_path):
    """At the size of test_do_all_sw_with_the_tools (16 layers, 8 000 wavenumbers, two bands, 3 columns x 5 zenith angles).  The
    trained model's RMS error against the line-by-line file over the top-of-atmosphere upwelling and the surface total
    downwelling band fluxes - terms of the cost - must not exceed the raw model's; how it compares with a training of the
    no-scattering forward model on the same file is printed, not asserted."""
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

    # the CKD model: do_all_sw.sh up to create_look_up_table (solar weights, Rayleigh coefficient)
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

    # 1. the training file: line-by-line two-stream fluxes with Rayleigh scattering, spectral boundary fluxes included
    ok(run_tool("ckdmip_sw", "--config", "sw_b.nam", "--scenario", "present", "--ssi", "ssi.nc", "--rayleigh", "rayleigh.nc", "train_h2o.nc",
                "train_o3.nc", "--output", "lbl_ray.nc", cwd=d))
    f = _nc(d / "lbl_ray.nc")
    assert f.rayleigh_scattering == b"two-stream" and f.constituent_id == b"h2o o3"
    assert f.variables["spectral_flux_dn_surf_sw"].shape == (ncol, 5, nwav)
    truth_dn = f.variables["band_flux_dn_sw"][:, :, -1, :].astype(np.float64)          # (column, mu0, band): surface, direct + diffuse
    truth_up = f.variables["band_flux_up_sw"][:, :, 0, :].astype(np.float64)           # top of atmosphere
    direct_surf = f.variables["band_flux_dn_direct_sw"][:, :, -1, :].astype(np.float64)
    f.close()
    assert np.all(truth_dn[..., 1] > direct_surf[..., 1] * 1.01) and np.all(truth_up[..., 1] > 0.15 * truth_dn[..., 1])   # it scatters

    # 2. the training, and for comparison the no-scattering forward model on the same file (direct beam, upwelling masked above 10 000 cm-1)
    keys = ("training_input=lbl_ray.nc", "gpointfile=gpoints.nc", "prior_error=2.0", "broadband_weight=0.4", "flux_weight=0.3",
            "flux_profile_weight=0.05", "spectral_boundary_weight=0.01", "max_iterations=60", "convergence_criterion=0")
    r = ok(run_tool("optimize_lut", "input=raw.nc", "output=ckd_ray.nc", "rayleigh_scattering=1", *keys, cwd=d))
    log = r.stdout + r.stderr
    assert "Mapping high-resolution boundary fluxes to g-points" in log           # spectral_flux_dn_surf_sw was read
    cost = [float(x) for x in re.findall(r"Iteration \d+: cost function = ([0-9.eE+-]+)", log)]
    assert 3 < len(cost) <= 61 and cost[-1] < cost[0], cost
    ok(run_tool("optimize_lut", "input=raw.nc", "output=ckd_plain.nc", *keys, cwd=d))
    a, b = _nc(d / "raw.nc"), _nc(d / "ckd_ray.nc")
    band = a.variables["band_number"][...].astype(int)
    assert not np.array_equal(a.variables["h2o_molar_absorption_coeff"][...], b.variables["h2o_molar_absorption_coeff"][...])
    a.close(); b.close()

    # 3. the evaluation: the models' optical depths through the two-stream transfer
    w = netcdf_file(str(d / "eval.nc"), "w", version=2)
    for dim, n in (("column", ncol), ("half_level", nlay + 1), ("level", nlay)):
        w.createDimension(dim, n)
    w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p1, (ncol, 1))
    w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = np.tile(t0, (ncol, 1))
    for g, (_, vmr) in base.items():
        w.createVariable(g + "_mole_fraction_fl", "d", ("column", "level"))[:] = np.tile((vmr * amount[g])[:, None], (1, nlay))
    w.close()
    rms = {}
    for tag in ("raw", "ckd_ray", "ckd_plain"):
        ok(run_tool("run_ckd", f"ckd_model={tag}.nc", "input=eval.nc", f"output=od_{tag}.nc", f"tsi={ssi.sum()}", cwd=d))
        ok(run_tool("ckdmip_sw", "--config", "sw.nam", "--ckd", f"od_{tag}.nc", "--rayleigh-scattering", "--output", f"flux_{tag}.nc", cwd=d))
        f = _nc(d / f"flux_{tag}.nc")
        assert f.rayleigh_scattering == b"two-stream" and np.allclose(f.variables["mu0"][:], mu0s)
        assert np.allclose(f.variables["flux_dn_sw"][:, :, 0], mu0s[None, :] * ssi.sum(), rtol=1e-5)      # the sun of the training file
        dn_g = f.variables["spectral_flux_dn_sw"][:, :, -1, :].astype(np.float64)      # (column, mu0, g_point)
        up_g = f.variables["spectral_flux_up_sw"][:, :, 0, :].astype(np.float64)
        f.close()
        dn = np.stack([dn_g[..., band == k].sum(-1) for k in range(2)], axis=-1)
        up = np.stack([up_g[..., band == k].sum(-1) for k in range(2)], axis=-1)
        rms[tag] = float(np.sqrt(np.mean(np.concatenate([(dn - truth_dn).ravel(), (up - truth_up).ravel()]) ** 2)))
    print("RMS error of TOA upwelling and surface total downwelling band fluxes (W m-2):", rms)
    print("trained with scattering better than trained without:", rms["ckd_ray"] < rms["ckd_plain"])
    assert np.isfinite(rms["raw"]) and rms["ckd_ray"] <= rms["raw"]
