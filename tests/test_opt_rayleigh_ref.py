"""CPU checks around the scattering optimiser: the numpy restatement of the shortwave cost (tests/opt_rayleigh_ref.py) pinned
against the C oracle where the two must agree, the new entry point in header and bindings, and optimize_lut's refusal of
rayleigh_scattering=1 on a longwave model before a device is opened."""
import os
import re
import subprocess

import numpy as np
import pytest

import ckd_synth
import opt_rayleigh_ref as orr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(flux_weight=0.2, flux_profile_weight=0.05, broadband_weight=0.4, spectral_boundary_weight=0.0,
           negative_od_penalty=1.0e4, pressure_weight_power=0.5, prior_error=4.0, pressure_corr=0.95,
           temperature_corr=0.95, conc_corr=0.9, cap_relative_linear=0.0)


def _problem_sw(oracle, seed, albedo=(0.15, 0.3, 0.06), boundary=False, ch4_low=False, relative=False, **over):
    """tests/test_optimize_gpu.py's _problem_sw with the Rayleigh coefficient at zero, where the scattering transfer is the
    reference's radiative_transfer_norayleigh_sw: no diffuse light, exp(-2 tau) on the way up"""
    cfg = dict(CFG, **over)
    model = ckd_synth.make_model_sw(seed=seed)
    truth = ckd_synth.make_model_sw(seed=seed)
    rs = np.random.RandomState(seed + 5)
    for m in (model, truth):
        m["rayleigh_molar_scattering"] = np.zeros(m["ng"])
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    bw = 0.02 * rs.uniform(size=model["ng"]) if boundary else None
    scenes = ckd_synth.make_scenes_sw(model, albedo, boundary_weights=bw, ch4_low=ch4_low)
    orc_truth = ckd_synth.OracleSW(oracle, truth, scenes, cfg)
    for s in scenes:
        bf = orc_truth.band_fluxes(orc_truth.x0, s)
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
        if boundary:
            s["spectral_flux_dn_surf"] = np.ascontiguousarray(orc_truth.fluxes(orc_truth.x0, s)[:, 0, -1, :])
        if relative:
            f = orc_truth.fluxes(orc_truth.x0 + 0.05, s)
            s["relative_flux_dn"], s["relative_flux_up"] = np.ascontiguousarray(0.3 * f[:, 0]), np.ascontiguousarray(0.3 * f[:, 1])
    return model, scenes, cfg


@pytest.mark.parametrize("variant", ["base", "spectral_only", "mixed_albedo", "boundary", "negative_od", "relative_to"])
def test_numpy_cost_matches_the_c_oracle_without_scattering(oracle, variant):
    kw = {}
    if variant == "spectral_only":
        kw = dict(broadband_weight=0.0)
    if variant == "mixed_albedo":
        kw = dict(albedo=(0.2, 0.0, 0.1))
    if variant == "boundary":
        kw = dict(boundary=True)
    if variant == "negative_od":
        kw = dict(ch4_low=True)
    if variant == "relative_to":
        kw = dict(relative=True, boundary=True)
    model, scenes, cfg = _problem_sw(oracle, seed=3, **kw)
    c_orc = ckd_synth.OracleSW(oracle, model, scenes, cfg)
    np_orc = orr.OracleRayleigh(oracle, model, scenes, cfg, hr_from_net=False)
    rs = np.random.RandomState(1)
    free = c_orc.x0 > -1.0e20
    x = c_orc.x0 + np.where(free, 0.2 * rs.normal(size=c_orc.x0.size), 0.0)
    if variant == "negative_od":
        sizes = np.cumsum([0] + c_orc.sizes)
        x[sizes[3]:sizes[4]] += 9.0
        assert sum(int((c_orc.optical_depth(x, s) < 0).sum()) for s in scenes) > 10
    assert np_orc.cost_rt(x) == pytest.approx(c_orc.cost_rt(x), rel=1e-12)
    # and the net-flux heating rate is another cost wherever light comes back up (the penalty of the negative optical depths
    # buries that difference)
    if variant != "negative_od":
        assert abs(orr.OracleRayleigh(oracle, model, scenes, cfg, hr_from_net=True).cost_rt(x) - c_orc.cost_rt(x)) > 1e-6 * c_orc.cost_rt(x)


def test_header_and_bindings_declare_create_ex():
    from ecckd_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ecckd_hip.h")).read()
    assert re.search(r"\bint\s+ecckd_opt_create_ex\s*\(", txt) and re.search(r"#define\s+ECCKD_OPT_RAYLEIGH_SCATTERING\s+1u", txt)
    assert "ecckd_opt_create_ex" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ecckd_opt_create_ex"][1]) == len(_lib.SIGNATURES["ecckd_opt_create"][1]) + 1


def test_optimize_lut_refuses_scattering_on_a_longwave_model(tmp_path):
    """before any device is opened: this test has no GPU"""
    import __graft_entry__ as g
    from ecckd_amd import ncio
    g.build()
    model = ckd_synth.make_model(seed=2)
    ng, nwav = len(model["iband_per_g"]), 33
    gf = np.random.RandomState(1).uniform(size=(ng, nwav)); gf /= gf.sum(0, keepdims=True)
    model.update(wavenumber1=np.arange(nwav) * 10.0, wavenumber2=np.arange(1, nwav + 1) * 10.0, gpoint_fraction=gf,
                 wavenumber1_band=np.array([0.0, 100.0, 200.0]), wavenumber2_band=np.array([100.0, 200.0, 330.0]))
    ncio.write_ckd_model(str(tmp_path / "lw.nc"), model)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")        # no device even where there is one
    r = subprocess.run([os.path.join(ROOT, "bin", "optimize_lut"), "input=lw.nc", "output=out.nc", "training_input=none.nc",
                        "rayleigh_scattering=1"], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 147, r.stderr + r.stdout                                   # ECCKD_PARAMETER_ERROR
    assert "rayleigh_scattering" in r.stderr + r.stdout and "lw.nc" in r.stderr + r.stdout
    assert not (tmp_path / "out.nc").exists()
