"""The numpy reference of the optimiser's longwave cost under the zenith-angle quadrature (tests/opt_lw_angles_ref.py), on the
CPU: with the single angle sec = 1.66 it is the C oracle's two-stream cost - relative_to scene, per-g boundary term and clamped
cells included -, the weights of every rule sum to one, an isothermal opaque column radiates B at every N, and the Lambertian
surface rule holds for the angle-summed flux."""
import os
import re

import numpy as np
import pytest

import ckd_synth
import opt_lw_angles_ref as olr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(flux_weight=0.2, flux_profile_weight=0.05, broadband_weight=0.4, spectral_boundary_weight=0.3,
           negative_od_penalty=1.0e-8, pressure_weight_power=0.5, prior_error=4.0, pressure_corr=0.95,
           temperature_corr=0.95, conc_corr=0.9, cap_relative_linear=0.0)


def _two_stream_problem(oracle, **over):
    """the problem of tests/test_optimize_gpu.py with a relative_to scene, the boundary term and ch4 below its reference"""
    cfg = dict(CFG, **over)
    model, truth = ckd_synth.make_model(seed=3), ckd_synth.make_model(seed=3)
    rs = np.random.RandomState(8)
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    scenes = ckd_synth.make_scenes(model, ch4_low=True, ncol=2)
    orc_truth = ckd_synth.Oracle(oracle, truth, scenes, cfg)
    base = ckd_synth.Oracle(oracle, model, scenes, cfg)
    rel = base.fluxes(base.x0, scenes[0], unclamped=True)
    for s in scenes:
        f = orc_truth.fluxes(orc_truth.x0, s)
        bf = orc_truth.band_fluxes(orc_truth.x0, s)
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
        s["spectral_flux_dn_surf"] = np.ascontiguousarray(f[:, 0, -1, :])
        s["spectral_flux_up_toa"] = np.ascontiguousarray(f[:, 1, 0, :])
    scenes[1]["relative_flux_dn"], scenes[1]["relative_flux_up"] = np.ascontiguousarray(rel[:, 0]), np.ascontiguousarray(rel[:, 1])
    return model, scenes, cfg


@pytest.mark.parametrize("over", [{}, dict(flux_profile_weight=0.0), dict(broadband_weight=0.0), dict(pressure_weight_power=1.0)])
def test_single_angle_at_the_diffusivity_is_the_c_oracles_cost(oracle, over):
    model, scenes, cfg = _two_stream_problem(oracle, **over)
    c_orc = ckd_synth.Oracle(oracle, model, scenes, cfg)
    np_orc = olr.OracleLwAngles(oracle, model, scenes, cfg, [1.66], [1.0])
    rs = np.random.RandomState(2)
    x = c_orc.x0 + np.where(c_orc.x0 > -1.0e20, 0.2 * rs.normal(size=c_orc.x0.size), 0.0)
    sizes = np.cumsum([0] + c_orc.sizes)
    x[sizes[3]:sizes[4]] += 6.0                                      # the relative-linear gas drives about half the cells negative
    od = np.concatenate([c_orc.optical_depth(x, s).ravel() for s in scenes])
    assert (od < 0).sum() > 10 and (od > 0).sum() > 10
    assert scenes[1].get("relative_flux_dn") is not None and cfg["spectral_boundary_weight"] > 0
    a, b = np_orc.cost_rt(x), c_orc.cost_rt(x)
    print(f"numpy {a:.17g} C oracle {b:.17g} rel {abs(a - b) / abs(b):.3g}")
    assert a == pytest.approx(b, rel=olr.COST_REL_TOL)
    for s in scenes:
        ref = c_orc.fluxes(x, s)
        assert np.allclose(np_orc.fluxes(x, s), ref, rtol=1e-10, atol=1e-14 * np.abs(ref).max())


@pytest.mark.parametrize("nangle", range(1, 17))
def test_weights_sum_to_one_and_match_the_library(nangle):
    from ecckd_amd import api
    sec, wgt = olr.nodes(nangle)
    assert abs(wgt.sum() - 1.0) <= 1e-15 * nangle
    mu, w = api.gauss_legendre_01(nangle)                            # host only: the node set of lw_angle_table
    assert np.allclose(sec, 1.0 / mu, rtol=1e-13, atol=0) and np.allclose(wgt, 2.0 * w * mu, rtol=1e-13, atol=1e-17)
    assert np.all(np.diff(sec) < 0) and sec.min() > 1.0


@pytest.mark.parametrize("nangle", [1, 2, 3, 4, 8, 16])
def test_isothermal_opaque_column_radiates_planck(nangle):
    sec, wgt = olr.nodes(nangle)
    nlay, ng = 7, 3
    b = np.array([1.5, 20.0, 0.3])
    planck = np.tile(b, (nlay + 1, 1))
    dn, up = olr.transfer(planck, np.full((nlay, ng), 200.0), np.ones(ng), sec, wgt)
    assert np.allclose(dn[nlay], b, rtol=1e-14, atol=0) and np.allclose(up[0], b, rtol=1e-14, atol=0)
    assert np.all(dn[0] == 0.0)


@pytest.mark.parametrize("nangle", [1, 4, 16])
def test_lambertian_surface_rule_for_the_summed_flux(nangle):
    sec, wgt = olr.nodes(nangle)
    rs = np.random.RandomState(nangle)
    nlay, ng = 9, 4
    planck = rs.uniform(1.0, 5.0, (nlay + 1, ng))
    od = 10.0 ** rs.uniform(-7.0, 0.5, (nlay, ng))                   # thin and thick layers
    eps, _ = olr.layer_terms(od, sec)
    assert (eps > olr.THIN_EPS).any() and (eps <= olr.THIN_EPS).any()
    es = np.array([0.7, 0.7, 0.95, 1.0])
    dn, up = olr.transfer(planck, od, es, sec, wgt)
    assert np.allclose(up[nlay], es * planck[nlay] + (1.0 - es) * dn[nlay], rtol=1e-14, atol=0)
    dn1, up1 = olr.transfer(planck, od, np.ones(ng), sec, wgt)
    assert np.array_equal(dn, dn1) and np.all(up[0, :3] != up1[0, :3]) and np.array_equal(up[:, 3], up1[:, 3])


def test_header_and_bindings_declare_the_entry_points():
    from ecckd_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ecckd_hip.h")).read()
    assert re.search(r"\bint\s+ecckd_opt_create_angles\s*\(", txt) and re.search(r"\bint\s+ecckd_opt_nangle\s*\(", txt)
    assert len(_lib.SIGNATURES["ecckd_opt_create_angles"][1]) == len(_lib.SIGNATURES["ecckd_opt_create_ex"][1]) + 1
