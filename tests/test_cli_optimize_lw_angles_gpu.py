"""bin/optimize_lut nangle=N.

test_chain_through_ckdmip_lw is the whole loop: `ckdmip_lw` with nangle = 4 writes the training file, the tool trains on it
under the same quadrature, the host mirror (pipeline.optimize_lut(nangle=4)) writes the same file, and `run_ckd` +
`ckdmip_lw --ckd` with nangle = 4 evaluate the raw and the trained model: the trained one's fluxes are the optimiser's final
ones, and no further from the 4-angle truth than the raw one's.

The refusals need no GPU: they fire right after the configuration is read, before the device is opened, so they are asserted
with no device visible as well."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

import ckd_synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMETER_ERROR = 147
KEYS = ("prior_error=2.0", "broadband_weight=0.4", "flux_weight=0.3", "flux_profile_weight=0.05", "temperature_corr=0.8",
        "pressure_corr=0.8", "conc_corr=0.8", "convergence_criterion=0")


def _tool(name, *args, cwd=None, env=None):
    exe = os.path.join(ROOT, "bin", name)
    if not os.path.exists(exe):                      # a fresh checkout: build the library and the tools first
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return subprocess.run([exe, *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, **env) if env else None)


def _nc(path):
    return netcdf_file(str(path), "r", mmap=False)


@pytest.mark.gpu
def test_chain_through_ckdmip_lw(ctx, tmp_path):
    """At the size of test_do_all_lw_with_the_tools: two gases, two bands, 16 layers, 8 000 wavenumbers, three columns."""
    from ecckd_amd import api, ncio, pipeline
    from test_pipeline_gpu import make_do_all_inputs
    d = tmp_path
    inp = make_do_all_inputs(ctx, d)
    nlay = inp["nlay"]

    def ok(r):
        assert r.returncode == 0, r.stderr + r.stdout
        return r

    # the CKD model: do_all_lw.sh up to create_look_up_table
    for g in ("h2o", "co2"):
        ok(_tool("reorder_spectrum", f"input=present_{g}.nc", f"output=order_{g}.nc", "wavenumber1=0 1300", "wavenumber2=1300 3260", cwd=d))
    (d / "find_g.cfg").write_text(
        "heating_rate_tolerance 0.3\nmax_iterations 30\naveraging_method transmission\ngases h2o co2\n"
        "\\begin h2o\n input present_h2o.nc\n reordering_input order_h2o.nc\n background_input present_co2.nc\n\\end h2o\n"
        "\\begin co2\n input present_co2.nc\n reordering_input order_co2.nc\n background_input present_h2o.nc\n\\end co2\n")
    ok(_tool("find_g_points", "find_g.cfg", "output=gpoints.nc", cwd=d))
    (d / "lut.cfg").write_text(
        "input gpoints.nc\noutput raw.nc\ngases h2o co2\n"
        "\\begin h2o\n conc_dependence lut\n input \"ideal_h2o.nc ideal_h2o_x4.nc\"\n\\end h2o\n"
        "\\begin co2\n conc_dependence linear\n input ideal_co2.nc\n\\end co2\n")
    ok(_tool("create_look_up_table", "lut.cfg", cwd=d))

    # 1. the training file: line-by-line band fluxes of the three idealised columns (h2o at 1.5 times its file's amount) under
    #    four Gauss-Legendre angles per hemisphere, and for the record the two-stream ones
    nam = ("&longwave_config\noptical_depth_name = \"optical_depth\",\nnspectralstride = 1,\nnangle = NANGLE,\n"
           "do_write_spectral_boundary_fluxes = false,\nband_wavenumber1(1:2) = 0, 1300,\nband_wavenumber2(1:2) = 1300, 3260,\n/\n")
    (d / "lw4.nam").write_text(nam.replace("NANGLE", "4"))
    (d / "lw0.nam").write_text(nam.replace("NANGLE", "0"))
    for n in (4, 0):
        ok(_tool("ckdmip_lw", "--config", f"lw{n}.nam", "--scenario", "train", "--scale", "1.5", "ideal_h2o.nc", "ideal_co2.nc", "--output",
                 f"lbl{n}.nc", cwd=d))
    f4, f0 = _nc(d / "lbl4.nc"), _nc(d / "lbl0.nc")
    assert "nangle" not in f4._attributes                                   # ckdmip_lw writes no such attribute: the file is accepted
    truth_dn, truth_up = f4.variables["band_flux_dn_lw"][...].astype(np.float64), f4.variables["band_flux_up_lw"][...].astype(np.float64)
    two_up = f0.variables["band_flux_up_lw"][...].astype(np.float64)
    vmr_file = f4.variables["mole_fraction_fl"][...].astype(np.float64)     # (column, gas, level)
    t_file = f4.variables["temperature_hl"][...].astype(np.float64)
    f4.close(); f0.close()
    assert 1e-4 < np.max(np.abs(two_up - truth_up) / truth_up) < 0.05      # the two transfers differ, by the two-stream bias

    # 2. the training under the quadrature, tool and host mirror
    r = ok(_tool("optimize_lut", "input=raw.nc", "output=ckd4.nc", "training_input=lbl4.nc", "nangle=4", *KEYS, "max_iterations=40", cwd=d))
    log = r.stdout + r.stderr
    assert re.search(r"4 Gauss-Legendre zenith angles", log)
    cost = [float(x) for x in re.findall(r"Iteration \d+: cost function = ([0-9.eE+-]+)", log)]
    assert len(cost) > 3 and cost[-1] < cost[0], cost
    f = _nc(d / "ckd4.nc")
    assert b"nangle" in f.config                                           # the key is recorded by the existing mechanism
    band = f.variables["band_number"][...].astype(int)
    f.close()
    raw = ncio.read_ckd_model(str(d / "raw.nc"))
    kw = dict(prior_error=2.0, broadband_weight=0.4, flux_weight=0.3, flux_profile_weight=0.05, temperature_corr=0.8, pressure_corr=0.8,
              conc_corr=0.8, min_prior_error=-1.0, max_prior_error=-1.0)
    opt_model, res = pipeline.optimize_lut(ctx, raw, [str(d / "lbl4.nc")], max_iterations=40, nangle=4, **kw)
    assert res["status"] in (0, 2, 3) and res["iterations"] > 3
    ncio.write_ckd_model(str(d / "py4.nc"), opt_model)
    a, b = _nc(d / "ckd4.nc"), _nc(d / "py4.nc")
    assert set(a.variables) == set(b.variables)
    for k in a.variables:                                                   # variable by variable, bit for bit
        assert np.array_equal(a.variables[k][...], b.variables[k][...]), k
    a.close(); b.close()
    # the two-stream training of the same file is another result
    ok(_tool("optimize_lut", "input=raw.nc", "output=ckd0.nc", "training_input=lbl4.nc", *KEYS, "max_iterations=40", cwd=d))
    a, b = _nc(d / "ckd4.nc"), _nc(d / "ckd0.nc")
    assert not np.array_equal(a.variables["h2o_molar_absorption_coeff"][...], b.variables["h2o_molar_absorption_coeff"][...])
    a.close(); b.close()

    # 3. the evaluation: run_ckd's optical depths through `ckdmip_lw --ckd` with nangle = 4
    ncol = t_file.shape[0]
    w = netcdf_file(str(d / "eval.nc"), "w", version=2)
    for dim, n in (("column", ncol), ("half_level", nlay + 1), ("level", nlay)):
        w.createDimension(dim, n)
    w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(inp["p1"], (ncol, 1))
    w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = t_file
    for i, g in enumerate(("h2o", "co2")):
        w.createVariable(g + "_mole_fraction_fl", "d", ("column", "level"))[:] = vmr_file[:, i, :]
    w.close()
    (d / "ckd4.nam").write_text("&longwave_config\noptical_depth_name = \"optical_depth\",\nnangle = 4,\n/\n")
    rms, flux = {}, {}
    for tag in ("raw", "ckd4", "ckd0"):
        ok(_tool("run_ckd", f"ckd_model={tag}.nc", "input=eval.nc", f"output=od_{tag}.nc", cwd=d))
        ok(_tool("ckdmip_lw", "--config", "ckd4.nam", "--scenario", "train", "--ckd", f"od_{tag}.nc", "--output", f"flux_{tag}.nc", cwd=d))
        f = _nc(d / f"flux_{tag}.nc")
        dn_g = f.variables["spectral_flux_dn_lw"][...].astype(np.float64)                  # (column, half_level, g_point)
        up_g = f.variables["spectral_flux_up_lw"][...].astype(np.float64)
        f.close()
        flux[tag] = (dn_g, up_g)
        dn = np.stack([dn_g[..., band == k].sum(-1) for k in range(2)], axis=-1)
        up = np.stack([up_g[..., band == k].sum(-1) for k in range(2)], axis=-1)
        rms[tag] = float(np.sqrt(np.mean(np.concatenate([(dn - truth_dn).ravel(), (up - truth_up).ravel()]) ** 2)))
    print("RMS error of the band fluxes against the 4-angle line-by-line truth (W m-2):", rms)
    print("trained under the quadrature better than trained two-stream:", rms["ckd4"] < rms["ckd0"])
    assert np.isfinite(rms["raw"]) and rms["ckd4"] <= rms["raw"]
    # ... which are the optimiser's final fluxes: the written model through an nangle = 4 handle on the training file's scene
    names = [g["name"] for g in opt_model["gases"]]
    written = ncio.read_ckd_model(str(d / "ckd4.nc"))
    s = ncio.read_lbl_fluxes(str(d / "lbl4.nc"), names, ctx=ctx)
    m = dict(written, iband_per_g=pipeline.iband_per_g(written, s["band_wavenumber1"], s["band_wavenumber2"]))
    opt = api.Optimizer(ctx, m, [pipeline._scene_for_optimizer(s, False)], nangle=4, **kw)
    _, fl = opt.forward(opt.initial_state())
    opt.close()
    big = np.abs(fl).max()
    # (run_ckd writes the optical depths as FLOAT: the agreement of tests/test_cli_gpu.py's --ckd check)
    assert np.allclose(flux["ckd4"][0], fl[:, 0], rtol=3e-5, atol=1e-6 * big) and np.allclose(flux["ckd4"][1], fl[:, 1], rtol=3e-5, atol=1e-6 * big)


# ---- refusals: exit 147 right after the configuration is read, with and without a device to open ----
@pytest.fixture(scope="module")
def refusal_files(tmp_path_factory):
    from ecckd_amd import ncio
    d = tmp_path_factory.mktemp("optimize_lw_angles_refusals")
    for name, model in (("raw_lw.nc", ckd_synth.make_model(seed=12)), ("raw_sw.nc", ckd_synth.make_model_sw(seed=8))):
        ng, ib, nband = len(model["iband_per_g"]), model["iband_per_g"], model["nband"]
        model.update(wavenumber1=np.arange(ng) * 10.0, wavenumber2=np.arange(1, ng + 1) * 10.0, gpoint_fraction=np.eye(ng),
                     wavenumber1_band=np.array([10.0 * np.nonzero(ib == b)[0][0] for b in range(nband)]),
                     wavenumber2_band=np.array([10.0 * (np.nonzero(ib == b)[0][-1] + 1) for b in range(nband)]))
        ncio.write_ckd_model(str(d / name), model)
    # a training file that says it was made with two angles: its attribute is all the tool reads of it before it refuses
    for name, nangle in (("lbl_two_angles.nc", 2), ("lbl_four_angles.nc", 4)):
        w = ncio.NcWriter(str(d / name))
        w.define_dimension("column", 1)
        w.define_dimension("half_level", 3)
        w.define_variable("pressure_hl", "double", "column", "half_level")
        w.write_attribute("nangle", nangle, nc_type="int")
        w.write_attribute("constituent_id", "h2o co2")
        w.end_define_mode()
        w.write("pressure_hl", np.array([[1.0, 500.0, 1000.0]]))
        w.close()
    return d


NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


@pytest.mark.parametrize("env", [None, NO_DEVICE], ids=["device", "no_device"])
@pytest.mark.parametrize("case", ["seventeen", "negative", "shortwave_input", "file_says_two", "relative_to_says_two"])
def test_refusals(refusal_files, case, env):
    from ecckd_amd import ncio
    d = refusal_files
    assert ncio.lbl_fluxes_nangle(str(d / "lbl_two_angles.nc")) == 2
    args = dict(seventeen=("input=raw_lw.nc", "training_input=lbl_four_angles.nc", "nangle=17"),
                negative=("input=raw_lw.nc", "training_input=lbl_four_angles.nc", "nangle=-1"),
                shortwave_input=("input=raw_sw.nc", "training_input=lbl_four_angles.nc", "nangle=4"),
                file_says_two=("input=raw_lw.nc", "training_input=lbl_two_angles.nc", "nangle=4"),
                relative_to_says_two=("input=raw_lw.nc", "training_input=lbl_four_angles.nc", "relative_to=lbl_two_angles.nc", "nangle=4"))[case]
    r = _tool("optimize_lut", *args, "output=x.nc", *KEYS, cwd=d, env=env)
    assert r.returncode == PARAMETER_ERROR, r.stderr + r.stdout
    assert "nangle" in r.stderr and not (d / "x.nc").exists()
    if case in ("file_says_two", "relative_to_says_two"):
        assert "lbl_two_angles.nc" in r.stderr


def test_pipeline_refusals(refusal_files):
    """the host mirror refuses the same before it opens anything on the device (ctx is never touched)"""
    from ecckd_amd import EcckdError, ncio, pipeline
    d = refusal_files
    lw, sw = ncio.read_ckd_model(str(d / "raw_lw.nc")), ncio.read_ckd_model(str(d / "raw_sw.nc"))
    for model, files, kw in ((lw, ["lbl_four_angles.nc"], dict(nangle=17)), (sw, ["lbl_four_angles.nc"], dict(nangle=4)),
                             (lw, ["lbl_two_angles.nc"], dict(nangle=4)), (lw, ["lbl_two_angles.nc"], dict(nangle=0)),
                             (lw, ["lbl_four_angles.nc"], dict(nangle=4, relative_to=str(d / "lbl_two_angles.nc")))):
        with pytest.raises(EcckdError) as e:
            pipeline.optimize_lut(None, model, [str(d / f) for f in files], **kw)
        assert e.value.code == PARAMETER_ERROR and "nangle" in str(e.value)
