"""GPU parity for optimize_lut (rows a17-a21): LUT interpolation, CKD fluxes, cost function,
hand-written adjoint gradient, Kronecker prior and the L-BFGS driver.

Oracle: oracle_ckd.c composed as solve_adept.cpp:72-211 (forward only).  The reference obtains
the gradient from Adept's tape; here it is checked against central finite differences of the
CPU oracle AND of the device cost.  The prior is checked against the dense LAPACK-inverse form
the reference uses.  Trajectories of adept::Minimizer are unpinned (third party, absent):
the driver is asserted on monotone decrease and final gradient norm."""
import numpy as np
import pytest

import ckd_synth

pytestmark = pytest.mark.gpu

CFG = dict(flux_weight=0.2, flux_profile_weight=0.05, broadband_weight=0.4, spectral_boundary_weight=0.0,
           negative_od_penalty=1.0e4, pressure_weight_power=0.5, prior_error=4.0, pressure_corr=0.95,
           temperature_corr=0.95, conc_corr=0.9, cap_relative_linear=0.0)


def _problem(oracle, seed=0, ch4_low=False, boundary=False, **over):
    cfg = dict(CFG, **over)
    model = ckd_synth.make_model(seed=seed)
    truth = ckd_synth.make_model(seed=seed)
    rs = np.random.RandomState(seed + 5)
    for g in truth["gases"]:                                # "LBL truth" = a perturbed model
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    scenes = ckd_synth.make_scenes(model, ch4_low=ch4_low)
    orc_truth = ckd_synth.Oracle(oracle, truth, scenes, cfg)
    for s in scenes:
        bf = orc_truth.band_fluxes(orc_truth.x0, s)
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
        if boundary:
            f = orc_truth.fluxes(orc_truth.x0, s)
            s["spectral_flux_dn_surf"] = np.ascontiguousarray(f[:, 0, -1, :])
            s["spectral_flux_up_toa"] = np.ascontiguousarray(f[:, 1, 0, :])
    orc = ckd_synth.Oracle(oracle, model, scenes, cfg)
    return model, scenes, cfg, orc


def _opt(ctx, model, scenes, cfg):
    from ecckd_amd import api
    return api.Optimizer(ctx, model, scenes, **cfg)


def test_forward_optical_depth_and_fluxes(ctx, oracle):
    model, scenes, cfg, orc = _problem(oracle)
    opt = _opt(ctx, model, scenes, cfg)
    x0 = opt.initial_state()
    assert np.allclose(x0, orc.x0, rtol=1e-15, atol=0)
    assert (x0 == -1.0e20).sum() > 0
    od, fl = opt.forward(x0)
    od_ref = np.concatenate([orc.optical_depth(x0, s) for s in scenes])
    fl_ref = np.concatenate([orc.fluxes(x0, s) for s in scenes])
    assert np.allclose(od, np.maximum(od_ref, 0.0), rtol=1e-12, atol=1e-300)
    assert np.allclose(fl, fl_ref, rtol=1e-10, atol=1e-300)
    opt.close()


def test_forward_unclamped_for_relative_to(ctx, oracle):
    """The "relative_to" fluxes (optimize_lut.cpp:229-234) come from od = value(aod) with NO clamp at zero: a cell whose
    relative-linear gas sits far enough below its reference concentration keeps its negative optical depth through
    radiative_transfer_lw.  ecckd_opt_forward_ex(unclamped) reproduces that; the default forward clamps as the cost does."""
    model, scenes, cfg, orc = _problem(oracle, seed=3, ch4_low=True)
    opt = _opt(ctx, model, scenes, cfg)
    x = opt.initial_state()
    sizes = np.cumsum([0] + orc.sizes)
    x[sizes[3]:sizes[4]] += 5.5                                # relative-linear gas strong enough for (vmr - ref) * k to win
    od_ref = np.concatenate([orc.optical_depth(x, s) for s in scenes])
    assert (od_ref < 0).sum() > 10 and od_ref.min() > -10.0    # moderately negative: exp(1.66 |od|) stays finite
    od_c, fl_c = opt.forward(x)
    od_u, fl_u = opt.forward(x, unclamped=True)
    assert np.allclose(od_u, od_ref, rtol=1e-12, atol=1e-300) and np.allclose(od_c, np.maximum(od_ref, 0.0), rtol=1e-12, atol=1e-300)
    fl_ref_u = np.concatenate([orc.fluxes(x, s, unclamped=True) for s in scenes])
    fl_ref_c = np.concatenate([orc.fluxes(x, s) for s in scenes])
    assert np.all(np.isfinite(fl_ref_u))
    # negative layers amplify: a flux that has grown through exp(+1.66 |od|) and then cancels carries the rounding of the big
    # number, so the comparison is relative to the largest flux of the profile set
    assert np.allclose(fl_u, fl_ref_u, rtol=1e-9, atol=1e-12 * np.abs(fl_ref_u).max()) and np.allclose(fl_c, fl_ref_c, rtol=1e-10, atol=1e-14 * np.abs(fl_ref_c).max())
    assert np.abs(fl_u - fl_c).max() > 1e-3 * np.abs(fl_c).max()
    J1, _ = opt.cost_grad(x)                                   # the mode does not leak into the cost function
    opt.forward(x, unclamped=True)
    assert opt.cost_grad(x)[0] == J1
    opt.close()


@pytest.mark.parametrize("variant", ["base", "no_profile_term", "boundary", "negative_od", "power1"])
def test_cost_and_gradient(ctx, oracle, variant):
    kw = {}
    if variant == "no_profile_term":
        kw = dict(flux_profile_weight=0.0, broadband_weight=0.0)
    if variant == "boundary":
        kw = dict(boundary=True, spectral_boundary_weight=0.3)
    if variant == "negative_od":
        kw = dict(ch4_low=True)
    if variant == "power1":
        kw = dict(pressure_weight_power=1.0, broadband_weight=1.0)
    model, scenes, cfg, orc = _problem(oracle, seed=3, **kw)
    opt = _opt(ctx, model, scenes, cfg)
    rs = np.random.RandomState(1)
    x0 = opt.initial_state()
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    if variant == "negative_od":
        # make the relative-linear gas strong so that (vmr - ref) * k drives cells negative
        sizes = np.cumsum([0] + orc.sizes)
        x[sizes[3]:sizes[4]] += 9.0
    J, g = opt.cost_grad(x)
    Jb_ref, gb_ref = orc.cost_prior(x, cfg["prior_error"])
    J_ref = orc.cost_rt(x) + Jb_ref
    assert J == pytest.approx(J_ref, rel=1e-10)
    if variant == "negative_od":
        od = np.concatenate([orc.optical_depth(x, s) for s in scenes])
        assert (od < 0).sum() > 10
    assert np.all(g[~free] == 0.0)
    # directional derivatives: device adjoint vs central differences of the CPU oracle
    for trial in range(3):
        d = np.where(free, rs.normal(size=x.size), 0.0)
        d /= np.linalg.norm(d)
        h = 1e-5
        fd = (orc.cost_rt(x + h * d) + orc.cost_prior(x + h * d, cfg["prior_error"])[0]
              - orc.cost_rt(x - h * d) - orc.cost_prior(x - h * d, cfg["prior_error"])[0]) / (2 * h)
        assert np.dot(g, d) == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    # single components vs central differences of the device cost
    idx = rs.choice(np.nonzero(free)[0], 12, replace=False)
    for i in idx:
        h = 1e-5
        e = np.zeros_like(x); e[i] = h
        fd = (opt.cost_grad(x + e, False) - opt.cost_grad(x - e, False)) / (2 * h)
        assert g[i] == pytest.approx(fd, rel=1e-5, abs=1e-7 * np.abs(g).max())
    opt.close()


@pytest.mark.parametrize("variant", ["base", "boundary", "negative_od"])
def test_gradient_matches_the_oracles_reverse_mode(ctx, oracle, variant):
    """Device adjoint against the oracle's hand-written reverse mode (oracle/oracle_adjoint.c, itself pinned to central
    differences in tests/test_oracle_adjoint.py): two independent derivations of dJ/dx, compared element by element."""
    kw = dict(boundary=True, spectral_boundary_weight=0.3) if variant == "boundary" else dict(ch4_low=True) if variant == "negative_od" else {}
    model, scenes, cfg, orc = _problem(oracle, seed=5, **kw)
    opt = _opt(ctx, model, scenes, dict(cfg, prior_error=1.0e30))       # the radiative-transfer part of the cost alone
    rs = np.random.RandomState(4)
    x0 = opt.initial_state()
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    if variant == "negative_od":
        sizes = np.cumsum([0] + orc.sizes)
        x[sizes[3]:sizes[4]] += 9.0
    J, g = opt.cost_grad(x)
    J_ref, g_ref = orc.cost_grad_rt(x)
    assert J == pytest.approx(J_ref, rel=1e-10)
    assert np.allclose(g, g_ref, rtol=1e-8, atol=1e-11 * np.abs(g_ref).max())
    opt.close()


def test_same_minimizer_over_device_and_oracle_cost_functions(ctx, oracle):
    """The library's L-BFGS run twice from the same state: over the device's cost function / gradient, and over the CPU
    oracle's (ecckd_opt_set_evaluator: forward cost of oracle_ckd.c, reverse mode of oracle_adjoint.c, dense-inverse prior).
    Same minimizer, two independent implementations of J and dJ/dx: the trajectories stay together, and the optimised
    models give the same heating rates (RMS difference, weighted as plot/calc_hr_error.m:1-23, far below 1e-6 K/day)."""
    model, scenes, cfg, orc = _problem(oracle, seed=7)
    opt = _opt(ctx, model, scenes, cfg)
    niter = 15
    hist_dev, hist_cpu = [], []
    opt.set_progress(lambda it, cost, gnorm: hist_dev.append((it, cost, gnorm)))
    res_dev = opt.minimize(max_iterations=niter, convergence_criterion=0.0, bounded=True)

    def cpu_cost_grad(x):
        J, g = orc.cost_grad_rt(x)
        Jb, gb = orc.cost_prior(x, cfg["prior_error"])
        g = g + gb
        g[np.abs(g) < 1.0e-80] = 0.0                                     # solve_adept.cpp:286
        return J + Jb, np.where(x > -1.0e20, g, 0.0)

    opt.set_evaluator(cpu_cost_grad)
    opt.set_progress(lambda it, cost, gnorm: hist_cpu.append((it, cost, gnorm)))
    res_cpu = opt.minimize(max_iterations=niter, convergence_criterion=0.0, bounded=True)
    opt.set_evaluator(None)
    assert res_dev["iterations"] == res_cpu["iterations"] == niter and res_dev["status"] == res_cpu["status"]
    assert len(hist_dev) == len(hist_cpu) and hist_dev[-1][1] < 0.7 * hist_dev[0][1]
    for (i1, c1, g1), (i2, c2, g2) in zip(hist_dev, hist_cpu):
        assert i1 == i2 and c1 == pytest.approx(c2, rel=1e-7) and g1 == pytest.approx(g2, rel=1e-5)
    moved = np.abs(res_dev["x"] - opt.initial_state()) > 0
    assert np.allclose(res_dev["x"][moved], res_cpu["x"][moved], rtol=0, atol=1e-6)
    # heating rates of the two optimised models on the training profiles
    _, fl_dev = opt.forward(res_dev["x"])
    _, fl_cpu = opt.forward(res_cpu["x"])
    p = np.concatenate([s["pressure_hl"] for s in scenes])
    conv = -(9.80665 / 1004.0) / np.diff(p, axis=1) * 86400.0
    net = lambda fl: (fl[:, 0] - fl[:, 1]).sum(-1)                        # broadband net flux (ncol, nhl), down - up
    hr_dev, hr_cpu = conv * np.diff(net(fl_dev), axis=1), conv * np.diff(net(fl_cpu), axis=1)
    w = np.diff(p ** (1.0 / 3.0), axis=1)                                # calc_hr_error.m:12-22: d(p^(1/3)), normalised per profile
    w = w / w.sum(axis=1, keepdims=True)
    rmse = np.sqrt(np.sum(w * (hr_dev - hr_cpu) ** 2) / p.shape[0])
    assert rmse < 1.0e-6, rmse
    opt.close()


def test_prior_matches_dense_inverse(ctx, oracle):
    """K9 Kronecker-tridiagonal stencil == the reference's dense inv(B) product, incl. the 1e-6 zeroing."""
    for corr in (dict(pressure_corr=0.95, temperature_corr=0.95, conc_corr=0.95),
                 dict(pressure_corr=0.8, temperature_corr=0.5, conc_corr=1e-3)):
        model, scenes, cfg, orc = _problem(oracle, seed=4, flux_weight=0.0, **corr)
        # isolate the prior: evaluate gradient difference between two states with identical RT? simpler:
        opt = _opt(ctx, model, scenes, cfg)
        rs = np.random.RandomState(2)
        x0 = opt.initial_state()
        free = x0 > -1.0e20
        x = x0 + np.where(free, 0.3 * rs.normal(size=x0.size), 0.0)
        J, g = opt.cost_grad(x)
        # same model with an (effectively) infinite prior error: RT part only
        opt_rt = _opt(ctx, model, scenes, dict(cfg, prior_error=1.0e30))
        J_rt, g_rt = opt_rt.cost_grad(x)
        Jb_ref, gb_ref = orc.cost_prior(x, cfg["prior_error"])
        assert J - J_rt == pytest.approx(Jb_ref, rel=1e-9)
        gb = g - g_rt
        scale = np.abs(gb_ref).max()
        # the pinned (zero-coefficient) g point: dx = 0 there, gradient forced to 0 (:283)
        assert np.allclose(gb[free], gb_ref[free], rtol=1e-8, atol=1e-9 * scale)
        opt.close(); opt_rt.close()


def test_bounds_and_coefficients(ctx, oracle):
    model, scenes, cfg, orc = _problem(oracle, seed=6)
    opt = _opt(ctx, model, scenes, cfg)
    x, lo, hi = opt.initial_state(bounds=True)
    free = x > -1.0e20
    co2 = model["gases"][2]
    off = orc.sizes[0] + orc.sizes[1]
    sl = slice(off, off + orc.sizes[2])
    kmin, kmax, k = co2["min_molar_abs"].ravel(), co2["max_molar_abs"].ravel(), co2["molar_abs"].ravel()
    pos = kmin > 0
    assert np.allclose(lo[sl][pos], np.log(kmin[pos])) and np.allclose(hi[sl], np.log(kmax))
    # k_min == 0: x_min = min(3x - 2 x_max, x_max - 1)  (solve_adept.cpp:352-353)
    z = ~pos
    assert z.any()
    assert np.allclose(lo[sl][z], np.minimum(3 * np.log(k[z]) - 2 * np.log(kmax[z]), np.log(kmax[z]) - 1.0))
    assert np.all(lo[free] < x[free]) and np.all(x[free] < hi[free])
    got = opt.coefficients(x, 1, model["gases"][1]["molar_abs"].shape)
    assert np.allclose(got, model["gases"][1]["molar_abs"], rtol=1e-14) and np.all(got[..., 0] == 0.0)
    assert np.array_equal(opt.coefficients(x, 4, model["gases"][4]["molar_abs"].shape), model["gases"][4]["molar_abs"])
    opt.close()


def test_minimize_reduces_cost(ctx, oracle):
    model, scenes, cfg, orc = _problem(oracle, seed=7)
    opt = _opt(ctx, model, scenes, cfg)
    x0 = opt.initial_state()
    J0, g0 = opt.cost_grad(x0)
    res = opt.minimize(max_iterations=150, convergence_criterion=1e-3 * np.linalg.norm(g0), bounded=True)
    assert res["status"] in (0, 2)
    assert res["cost"] < 0.5 * J0          # 150 L-BFGS iterations against a prior-regularised cost
    J1, g1 = opt.cost_grad(res["x"])
    assert J1 == pytest.approx(res["cost"], rel=1e-12)
    _, lo, hi = opt.initial_state(bounds=True)
    free = x0 > -1.0e20
    assert np.all(res["x"][free] >= lo[free]) and np.all(res["x"][free] <= hi[free])
    assert np.all(res["x"][~free] == -1.0e20)
    # the CPU oracle agrees on the cost at the optimum
    assert orc.cost_rt(res["x"]) + orc.cost_prior(res["x"], cfg["prior_error"])[0] == pytest.approx(J1, rel=1e-9)
    opt.close()


# ---- shortwave branch (calc_cost_function_ckd_sw, solve_adept.cpp:172-200) ---------------------------------

def _problem_sw(oracle, seed=0, albedo=(0.15, 0.3, 0.06), boundary=False, ch4_low=False, **over):
    cfg = dict(CFG, **over)
    model = ckd_synth.make_model_sw(seed=seed)
    truth = ckd_synth.make_model_sw(seed=seed)
    rs = np.random.RandomState(seed + 5)
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    ng = model["ng"]
    bw = 0.02 * rs.uniform(size=ng) if boundary else None
    scenes = ckd_synth.make_scenes_sw(model, albedo, boundary_weights=bw, ch4_low=ch4_low)
    orc_truth = ckd_synth.OracleSW(oracle, truth, scenes, cfg)
    for s in scenes:
        bf = orc_truth.band_fluxes(orc_truth.x0, s)
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
        if boundary:
            s["spectral_flux_dn_surf"] = np.ascontiguousarray(orc_truth.fluxes(orc_truth.x0, s)[:, 0, -1, :])
    orc = ckd_synth.OracleSW(oracle, model, scenes, cfg)
    return model, scenes, cfg, orc


def test_sw_forward(ctx, oracle):
    model, scenes, cfg, orc = _problem_sw(oracle)
    opt = _opt(ctx, model, scenes, cfg)
    x0 = opt.initial_state()
    assert np.allclose(x0, orc.x0, rtol=1e-15, atol=0)
    od, fl = opt.forward(x0)
    od_ref = np.concatenate([orc.optical_depth(x0, s) for s in scenes])
    fl_ref = np.concatenate([orc.fluxes(x0, s) for s in scenes])
    assert np.allclose(od, np.maximum(od_ref, 0.0), rtol=1e-12, atol=1e-300)
    assert np.allclose(fl, fl_ref, rtol=1e-10, atol=1e-300)
    assert fl[:, 1].max() > 0
    opt.close()


@pytest.mark.parametrize("variant", ["base", "spectral_only", "direct_only", "mixed_albedo", "boundary", "negative_od"])
def test_sw_cost_and_gradient(ctx, oracle, variant):
    kw = {}
    if variant == "spectral_only":
        kw = dict(broadband_weight=0.0)            # no 1/nband scaling in the shortwave (:243)
    if variant == "direct_only":
        kw = dict(albedo=(0.0, 0.0, -1.0))          # all(albedo <= 0): direct beam only, upwelling zero
    if variant == "mixed_albedo":
        kw = dict(albedo=(0.2, 0.0, 0.1))           # broadband upwelling terms dropped (:252, :264)
    if variant == "boundary":
        kw = dict(boundary=True)
    if variant == "negative_od":
        kw = dict(ch4_low=True)
    model, scenes, cfg, orc = _problem_sw(oracle, seed=3, **kw)
    opt = _opt(ctx, model, scenes, cfg)
    rs = np.random.RandomState(1)
    x0 = opt.initial_state()
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    if variant == "negative_od":
        sizes = np.cumsum([0] + orc.sizes)
        x[sizes[3]:sizes[4]] += 9.0
    J, g = opt.cost_grad(x)
    J_ref = orc.cost_rt(x) + orc.cost_prior(x, cfg["prior_error"])[0]
    assert J == pytest.approx(J_ref, rel=1e-10)
    if variant == "negative_od":
        od = np.concatenate([orc.optical_depth(x, s) for s in scenes])
        assert (od < 0).sum() > 10
    assert np.all(g[~free] == 0.0)
    for trial in range(3):
        d = np.where(free, rs.normal(size=x.size), 0.0)
        d /= np.linalg.norm(d)
        h = 1e-5
        fd = (orc.cost_rt(x + h * d) + orc.cost_prior(x + h * d, cfg["prior_error"])[0]
              - orc.cost_rt(x - h * d) - orc.cost_prior(x - h * d, cfg["prior_error"])[0]) / (2 * h)
        assert np.dot(g, d) == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    idx = rs.choice(np.nonzero(free)[0], 12, replace=False)
    for i in idx:
        h = 1e-5
        e = np.zeros_like(x); e[i] = h
        fd = (opt.cost_grad(x + e, False) - opt.cost_grad(x - e, False)) / (2 * h)
        assert g[i] == pytest.approx(fd, rel=1e-5, abs=1e-7 * np.abs(g).max())
    opt.close()


@pytest.mark.parametrize("variant", ["base", "spectral_only", "direct_only", "mixed_albedo", "boundary", "negative_od"])
def test_sw_gradient_matches_the_oracles_reverse_mode(ctx, oracle, variant):
    """Shortwave device adjoint against the oracle's hand-written shortwave reverse mode (orc_calc_cost_function_ckd_sw_ad,
    pinned to central differences in tests/test_oracle_adjoint.py): the second derivation of dJ/dx that the longwave already
    had, element by element, in every branch of calc_cost_function_ckd_sw."""
    kw = {}
    if variant == "spectral_only":
        kw = dict(broadband_weight=0.0)
    if variant == "direct_only":
        kw = dict(albedo=(0.0, 0.0, -1.0))
    if variant == "mixed_albedo":
        kw = dict(albedo=(0.2, 0.0, 0.1))
    if variant == "boundary":
        kw = dict(boundary=True)
    if variant == "negative_od":
        kw = dict(ch4_low=True)
    model, scenes, cfg, orc = _problem_sw(oracle, seed=5, **kw)
    opt = _opt(ctx, model, scenes, dict(cfg, prior_error=1.0e30))       # the radiative-transfer part of the cost alone
    rs = np.random.RandomState(4)
    x0 = opt.initial_state()
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    if variant == "negative_od":
        sizes = np.cumsum([0] + orc.sizes)
        x[sizes[3]:sizes[4]] += 9.0
    J, g = opt.cost_grad(x)
    J_ref, g_ref = orc.cost_grad_rt(x)
    assert J == pytest.approx(J_ref, rel=1e-10)
    assert np.allclose(g, g_ref, rtol=1e-8, atol=1e-11 * np.abs(g_ref).max())
    opt.close()


def test_sw_minimize_reduces_cost(ctx, oracle):
    model, scenes, cfg, orc = _problem_sw(oracle, seed=7)
    opt = _opt(ctx, model, scenes, cfg)
    x0 = opt.initial_state()
    J0, g0 = opt.cost_grad(x0)
    res = opt.minimize(max_iterations=150, convergence_criterion=1e-3 * np.linalg.norm(g0), bounded=True)
    assert res["status"] in (0, 2)
    assert res["cost"] < 0.5 * J0
    assert orc.cost_rt(res["x"]) + orc.cost_prior(res["x"], cfg["prior_error"])[0] == pytest.approx(res["cost"], rel=1e-9)
    opt.close()


# ---- relative_to fluxes (optimize_lut.cpp:204-254, solve_adept.cpp:118-148) -----------------------------------

@pytest.mark.parametrize("sw", [False, True])
def test_relative_to_fluxes(ctx, oracle, sw):
    """Training on the difference to a reference scene: the CKD fluxes of the relative-to scene at the initial
    coefficients are subtracted from the forward model per g point, the LBL fluxes from the truth."""
    model, scenes, cfg, orc = (_problem_sw if sw else _problem)(oracle, seed=9, boundary=True,
                                                                **({} if sw else dict(spectral_boundary_weight=0.3)))
    Orc = ckd_synth.OracleSW if sw else ckd_synth.Oracle
    base, pert = scenes[0], scenes[1]
    pert = dict(pert, pressure_hl=base["pressure_hl"], temperature_hl=base["temperature_hl"])   # same profiles, other gases
    ref_opt = _opt(ctx, model, [dict(base)], cfg)
    _, fl = ref_opt.forward(ref_opt.initial_state())            # CKD fluxes of the relative-to scene, (ncol, 2, nhl, ng)
    ref_opt.close()
    fl_ref = Orc(oracle, model, [base], cfg).fluxes(orc.x0, base)
    assert np.allclose(fl, fl_ref, rtol=1e-10, atol=1e-300)
    truth = Orc(oracle, model, [pert], cfg)
    bf = truth.band_fluxes(truth.x0 + 0.1, pert) - truth.band_fluxes(truth.x0 + 0.1, base)       # "LBL" difference
    train = dict(pert, flux_dn=np.ascontiguousarray(bf[:, 0]), flux_up=np.ascontiguousarray(bf[:, 1]),
                 relative_flux_dn=np.ascontiguousarray(fl[:, 0]), relative_flux_up=np.ascontiguousarray(fl[:, 1]))
    if "spectral_flux_dn_surf" in train:
        f_p, f_b = truth.fluxes(truth.x0 + 0.1, pert), truth.fluxes(truth.x0 + 0.1, base)
        train["spectral_flux_dn_surf"] = np.ascontiguousarray(f_p[:, 0, -1] - f_b[:, 0, -1])
        if not sw:
            train["spectral_flux_up_toa"] = np.ascontiguousarray(f_p[:, 1, 0] - f_b[:, 1, 0])
    o2 = Orc(oracle, model, [train], cfg)
    opt = _opt(ctx, model, [train], cfg)
    rs = np.random.RandomState(2)
    x0 = opt.initial_state()
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.15 * rs.normal(size=x0.size), 0.0)
    J, g = opt.cost_grad(x)
    assert J == pytest.approx(o2.cost_rt(x) + o2.cost_prior(x, cfg["prior_error"])[0], rel=1e-10)
    # and it differs from the cost without the subtraction
    plain = dict(train, relative_flux_dn=None, relative_flux_up=None)
    assert abs(Orc(oracle, model, [plain], cfg).cost_rt(x) - o2.cost_rt(x)) > 1e-6 * abs(J)
    for trial in range(2):
        d = np.where(free, rs.normal(size=x.size), 0.0)
        d /= np.linalg.norm(d)
        h = 1e-5
        fd = (o2.cost_rt(x + h * d) + o2.cost_prior(x + h * d, cfg["prior_error"])[0]
              - o2.cost_rt(x - h * d) - o2.cost_prior(x - h * d, cfg["prior_error"])[0]) / (2 * h)
        assert np.dot(g, d) == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    opt.close()


# ---- the cell-parallel K8a against the general kernel (two implementations of the same arithmetic) --------------------

@pytest.mark.parametrize("sw", [False, True])
@pytest.mark.parametrize("threads", [None, 128])
def test_cell_parallel_kernel_matches_the_general_one(ctx, oracle, sw, threads, monkeypatch):
    """k_opt_forward_adjoint_cells (exp / division of every cell side by side, one FMA per layer on the sequential wave) and
    k_opt_forward_adjoint (everything on the sequential wave): optical depths identical, fluxes, cost and gradient equal to
    rounding - both follow the same recurrences, only the grouping of the layer's source terms differs (a few ulp)."""
    if threads:                         # (the parameter keeps its old name.)  128 threads would be 2 layer groups: 9 of the 18
                                        # layers per thread, which the cell-parallel kernel does not take (8 cells at most) - both
                                        # runs would use the general kernel; 192: 3 groups, 6 cells per thread (NC = 8).  The
                                        # library reads the variable at every call, and the plan below proves what ran.
        threads = 192
        monkeypatch.setenv("ECCKD_K8A_THREADS", str(threads))
    model, scenes, cfg, orc = (_problem_sw if sw else _problem)(oracle, seed=4, boundary=True, ch4_low=True,
                                                                **({} if sw else dict(spectral_boundary_weight=0.3)))
    opt = _opt(ctx, model, scenes, cfg)
    rs = np.random.RandomState(8)
    x0 = opt.initial_state()
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    sizes = np.cumsum([0] + orc.sizes)
    x[sizes[3]:sizes[4]] += 9.0                                  # negative optical depths: penalty and clamp
    out = {}
    for generic in ("1", "0"):
        monkeypatch.setenv("ECCKD_K8A_GENERIC", generic)
        plan = opt.forward_plan()
        if generic == "1":
            assert not plan["cells"]
        elif threads:
            assert (plan["cells"], plan["nc_template"], plan["lgroups"], plan["threads"]) == (True, 8, 3, 192)
        else:
            assert (plan["cells"], plan["nc_template"], plan["threads"]) == (True, 4, 512 if sw else 1024)
        J, g = opt.cost_grad(x)
        od, fl = opt.forward(x)
        od_u, fl_u = opt.forward(x, unclamped=True)
        out[generic] = (J, g, od, fl, od_u, fl_u)
    a, b = out["1"], out["0"]
    assert (a[2] == 0).sum() > 10                                # clamped cells are in play
    # (the two kernels add the look-up products in the same order, but the compiler fuses multiply and add differently)
    assert np.allclose(a[2], b[2], rtol=1e-13, atol=1e-300) and np.allclose(a[4], b[4], rtol=1e-13, atol=1e-300)
    assert np.allclose(a[3], b[3], rtol=1e-13, atol=1e-300) and np.allclose(a[5], b[5], rtol=1e-13, atol=1e-300, equal_nan=True)
    assert b[0] == pytest.approx(a[0], rel=1e-13)
    assert np.allclose(a[1], b[1], rtol=1e-9, atol=1e-12 * np.abs(a[1]).max())
    assert np.array_equal(a[1] == 0.0, b[1] == 0.0)
    opt.close()


@pytest.mark.parametrize("sw", [False, True])
def test_more_than_64_g_points(ctx, oracle, sw):
    """ng = 70: rows of the tables are 70 long, a wave covers 64 of them - two g chunks per node in K8b, 128-wide layer groups
    in K8a (the narrow-band models of the reference's scripts have 64 ... 128 g points; the other tests use 12).  Cost against
    the oracle, gradient against the oracle's reverse mode, the two K8a kernels against each other."""
    import os
    mk_model = ckd_synth.make_model_sw if sw else ckd_synth.make_model
    model = mk_model(seed=6, ng=70, nband=5)
    truth = mk_model(seed=6, ng=70, nband=5)
    rs = np.random.RandomState(11)
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    cfg = dict(CFG)
    if sw:
        scenes = ckd_synth.make_scenes_sw(model, np.array([0.15, 0.3, 0.06, 0.2, 0.1]))
        Orc = ckd_synth.OracleSW
    else:
        scenes = ckd_synth.make_scenes(model)
        Orc = ckd_synth.Oracle
    t = Orc(oracle, truth, scenes, cfg)
    for s in scenes:
        bf = t.band_fluxes(t.x0, s)
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
    orc = Orc(oracle, model, scenes, cfg)
    opt = _opt(ctx, model, scenes, cfg)
    x0 = opt.initial_state()
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    J, g = opt.cost_grad(x)
    J_rt, g_rt = orc.cost_grad_rt(x)
    J_b, g_b = orc.cost_prior(x, cfg["prior_error"])
    assert J == pytest.approx(J_rt + J_b, rel=1e-10)
    g_ref = np.where(free, g_rt + g_b, 0.0)
    assert np.allclose(g, g_ref, rtol=1e-8, atol=1e-11 * np.abs(g_ref).max())
    os.environ["ECCKD_K8A_GENERIC"] = "1"
    try:
        J2, g2 = opt.cost_grad(x)
    finally:
        del os.environ["ECCKD_K8A_GENERIC"]
    assert J2 == pytest.approx(J, rel=1e-13) and np.allclose(g2, g, rtol=1e-9, atol=1e-12 * np.abs(g).max())
    res = opt.minimize(max_iterations=25, convergence_criterion=0.0, bounded=True)
    assert res["status"] in (0, 2) and res["cost"] < J
    opt.close()
