"""The optimiser under the longwave zenith-angle quadrature (ecckd_opt_create_angles, api.Optimizer(..., nangle=N)):
k_opt_forward_adjoint_lw_angles against the numpy float64 restatement of tests/opt_lw_angles_ref.py - forward fluxes (also
against the g-point kernel ecckd_rt_lw_gpoints), cost, the hand-derived adjoint against central and Richardson differences of the
NUMPY cost, both branches of the layer term, clamped cells, every term of the longwave cost, the Lambertian surface, the block
sizes, the minimiser, reproducibility and the refusals."""
import numpy as np
import pytest

import ckd_synth
import opt_lw_angles_ref as olr

pytestmark = pytest.mark.gpu

CFG = dict(flux_weight=0.2, flux_profile_weight=0.05, broadband_weight=0.4, spectral_boundary_weight=0.0,
           negative_od_penalty=1.0e4, pressure_weight_power=0.5, prior_error=40.0, pressure_corr=0.95,
           temperature_corr=0.95, conc_corr=0.9, cap_relative_linear=0.0)


def _bands(model, f):
    return np.stack([f[:, :, :, model["iband_per_g"] == b].sum(-1) for b in range(model["nband"])], axis=-1)


def _problem(oracle, nangle, seed=3, ng=12, nband=3, nlay=18, nscene=2, ncol=2, ch4_low=False, boundary=False, emissivity=None, top_layer_pa=None,
             absorb=30.0, **over):
    """A training problem whose truth is a perturbed model's nangle-angle fluxes from the numpy oracle.
    absorb: the gases of ckd_synth absorb that many times as strongly.  The reference's layer term 1 - eps / (sec tau) loses
    digits as the layer thins - one unit in the last place of the exponential is 1e-16 / (sec tau)^2 of the term - and the
    fluxes are held to 1e-10 of a numpy restatement whose exponential is another implementation: at 1 the 4 Pa top layer of
    ckd_synth's columns has sec tau = 4e-5 at its weakest g point, and the two differed by 3e-10 there; at 30 it has 1e-3."""
    cfg = dict(CFG, **over)
    model = ckd_synth.make_model(seed=seed, ng=ng, nband=nband)
    truth = ckd_synth.make_model(seed=seed, ng=ng, nband=nband)
    for m in (model, truth):
        for g in m["gases"]:
            for k in ("molar_abs", "min_molar_abs", "max_molar_abs"):
                g[k] = g[k] * absorb
    rs = np.random.RandomState(seed + 5)
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    scenes = ckd_synth.make_scenes(model, ch4_low=ch4_low, nscene=nscene, ncol=ncol, nlay=nlay)
    if nlay == 1:
        # ckd_synth's single layer would be the 4 Pa between 1 and 5 Pa: a heating rate per unit flux of 1 / (4 Pa), so large
        # that the float64 rounding of the NUMPY cost drowns its own finite differences.  The one layer spans the column.
        for s in scenes:
            s["pressure_hl"][:, 1] = 101325.0 - 2000.0 * np.arange(s["pressure_hl"].shape[0])
    if top_layer_pa is not None:
        for s in scenes:                                             # an almost empty top layer: the thin branch of the layer term
            s["pressure_hl"][:, 0] = s["pressure_hl"][:, 1] - top_layer_pa
    if emissivity is not None:
        for s in scenes:
            s["surf_emissivity"] = np.tile(np.asarray(emissivity, dtype=np.float64)[:nband], (s["pressure_hl"].shape[0], 1))
    sec, wgt = olr.nodes(nangle)
    orc_truth = olr.OracleLwAngles(oracle, truth, scenes, cfg, sec, wgt)
    for s in scenes:
        f = orc_truth.fluxes(orc_truth.x0, s)
        bf = _bands(model, f)
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
        if boundary:
            s["spectral_flux_dn_surf"] = np.ascontiguousarray(f[:, 0, -1, :])
            s["spectral_flux_up_toa"] = np.ascontiguousarray(f[:, 1, 0, :])
    return model, scenes, cfg, olr.OracleLwAngles(oracle, model, scenes, cfg, sec, wgt)


def _opt(ctx, model, scenes, cfg, nangle):
    from ecckd_amd import api
    return api.Optimizer(ctx, model, scenes, nangle=nangle, **cfg)


def _state(opt, orc, seed, negative_od=False):
    rs = np.random.RandomState(seed)
    x0 = opt.initial_state()
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    if negative_od:
        sizes = np.cumsum([0] + orc.sizes)
        x[sizes[3]:sizes[4]] += 6.0          # ch4 below its reference: about half of the cells turn negative
    return x, free, rs


def _assert_off_kinks(orc, x, scenes):
    """No finite difference (a relative change of the coefficients of 1e-5) straddles a kink: no (cell, angle) has eps within a
    relative 1e-3 of the thin-layer threshold, and no cell changes its clamp state when the optical depth of every gas is
    scaled by 1 - 1e-3 or 1 + 1e-3, each gas on its own (|tau| > 1e-3 sum |tau_gas|)."""
    for s in scenes:
        od, od_abs = orc.gas_optical_depths(x, s)
        assert np.allclose(od, orc.optical_depth(x, s), rtol=1e-12, atol=1e-14 * od_abs.max())
        assert np.all(np.abs(od) > 1e-3 * od_abs)
        eps, _ = olr.layer_terms(np.maximum(od, 0.0), orc.sec)
        assert np.all(np.abs(eps[:, od > 0.0] - olr.THIN_EPS) > 1e-3 * olr.THIN_EPS)


def _cost(orc, cfg, x):
    return orc.cost_rt(x) + orc.cost_prior(x, cfg["prior_error"])[0]


FD_STEP = 1.0e-4


def _richardson(f, h=FD_STEP):
    """d f(t) / dt at 0 from central differences at h and h / 2, extrapolated: the error is O(h^4).  The step is large for a
    float64 difference because the numpy cost carries the rounding of its own heating rates - the 4 Pa of the top layer turn one
    unit in the last place of a flux into 3e-11 K / day - which measured 2e-12 on a cost of 3: 2e-7 in a difference at
    h = 1e-5, 2e-8 here."""
    f1 = (f(h) - f(-h)) / (2 * h)
    f2 = (f(0.5 * h) - f(-0.5 * h)) / h
    return f1, (4.0 * f2 - f1) / 3.0


def _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs, ncoord=12):
    _assert_off_kinks(orc, x, scenes)
    J, g = opt.cost_grad(x)
    J2, g2 = opt.cost_grad(x)
    assert J == J2 and np.array_equal(g, g2)                                 # bit-identical run to run
    J_ref = _cost(orc, cfg, x)
    print(f"cost {J:.17g} numpy {J_ref:.17g} rel {abs(J - J_ref) / abs(J_ref):.3g}")
    assert J == pytest.approx(J_ref, rel=olr.COST_REL_TOL)
    assert np.all(g[~free] == 0.0)
    for trial in range(3):
        d = np.where(free, rs.normal(size=x.size), 0.0)
        d /= np.linalg.norm(d)
        central, fd = _richardson(lambda t: _cost(orc, cfg, x + t * d))
        print(f"direction {trial}: g.d {np.dot(g, d):.12g} central {central:.12g} Richardson {fd:.12g}")
        assert np.dot(g, d) == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    idx = rs.choice(np.nonzero(free)[0], min(ncoord, int(free.sum())), replace=False)
    for i in idx:
        e = np.zeros_like(x); e[i] = 1.0
        central, fd = _richardson(lambda t: _cost(orc, cfg, x + t * e))
        print(f"coordinate {i}: g {g[i]:.12g} central {central:.12g} Richardson {fd:.12g}")
        assert g[i] == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    return J, g


def _check_forward(ctx, opt, orc, scenes, x, nangle, gpoint_kernel=True):
    """the fluxes against the numpy restatement and, at unit emissivity, against ecckd_rt_lw_gpoints on the handle's own od"""
    from ecckd_amd import api
    od, fl = opt.forward(x)
    c0 = 0
    for s in scenes:
        ncol = s["pressure_hl"].shape[0]
        od_ref = np.maximum(orc.optical_depth(x, s), 0.0)
        assert np.allclose(od[c0:c0 + ncol], od_ref, rtol=1e-12, atol=1e-300)
        ref = orc.fluxes(x, s)
        print(f"forward against numpy: {np.abs(fl[c0:c0 + ncol] / np.where(ref != 0, ref, 1.0) - 1.0)[ref != 0].max():.3g}")
        assert np.allclose(fl[c0:c0 + ncol], ref, rtol=1e-10, atol=1e-300)
        if gpoint_kernel:
            planck = np.stack([orc.planck(s["temperature_hl"][c]) for c in range(ncol)])
            dn, up = api.rt_lw_gpoints(ctx, planck, od[c0:c0 + ncol], nangle=nangle)
            big = np.abs(ref).max()
            assert np.allclose(fl[c0:c0 + ncol, 0], dn, rtol=1e-10, atol=1e-14 * big)
            assert np.allclose(fl[c0:c0 + ncol, 1], up, rtol=1e-10, atol=1e-14 * big)
        c0 += ncol
    return fl


# ---- shapes: one layer, top and surface adjacent, lengths that are no multiple of a chunk or of the layer groups; g points below,
#      at and above one wave; one band and several; three block sizes; one angle that is not 1.66, a count that does not divide
#      the layer groups, the usual four and the maximum (more angles than layer groups).  Every value of every parameter of the
#      product nlay x ng x nband x block x nangle appears; the product itself (288 cases) is trimmed to these.
SHAPES = [(1, 5, 1, None, 1), (1, 64, 3, 192, 4), (2, 70, 1, 64, 3), (2, 5, 3, None, 16), (2, 64, 3, None, 1), (9, 64, 1, 64, 16),
          (9, 70, 3, None, 4), (9, 5, 3, 192, 3), (17, 64, 3, None, 4), (17, 70, 3, 192, 16), (17, 5, 1, 64, 1), (17, 64, 1, 192, 3)]


@pytest.mark.parametrize("nlay,ng,nband,threads,nangle", SHAPES)
def test_shapes(ctx, oracle, nlay, ng, nband, threads, nangle, monkeypatch):
    if threads:
        monkeypatch.setenv("ECCKD_K8A_THREADS", str(threads))
    model, scenes, cfg, orc = _problem(oracle, nangle, seed=3, ng=ng, nband=nband, nlay=nlay, nscene=1, ncol=2)
    opt = _opt(ctx, model, scenes, cfg, nangle)
    assert opt.nangle == nangle
    plan = opt.forward_plan()
    ngpad = (ng + 63) // 64 * 64
    assert plan["kernel"] == "lw_angles" and not plan["cells"] and not plan["rayleigh"] and plan["nc_template"] == 0 and plan["nb"] == 0
    assert plan["ngpad"] == ngpad and plan["threads"] == ngpad * max(1, (threads or 1024) // ngpad)
    x, free, rs = _state(opt, orc, 6)
    _check_forward(ctx, opt, orc, scenes, x, nangle)
    _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs)
    opt.close()


VARIANTS = ["base", "thin_top_layer", "negative_od", "boundary", "no_profile_term", "spectral_only", "emissivity"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_cost_and_gradient(ctx, oracle, variant):
    """every term of the longwave cost, both branches of the layer term, clamped cells and the Lambertian coupling, at 4 angles on
    two scenes (the second lacks a gas of the model)"""
    nangle, kw = 4, {}
    if variant == "thin_top_layer":
        kw = dict(top_layer_pa=0.1, absorb=1.0)
    if variant == "negative_od":
        # (the clamped cells reach -1e6: a penalty of 1e4 per squared optical depth would be 1e15 beside a transfer cost of 20,
        # and the relative tolerances would see it alone; at 1e-11 the two shares are alike)
        kw = dict(ch4_low=True, negative_od_penalty=1.0e-11)
    if variant == "boundary":
        kw = dict(boundary=True, spectral_boundary_weight=0.3)
    if variant == "no_profile_term":
        kw = dict(flux_profile_weight=0.0)
    if variant == "spectral_only":
        kw = dict(broadband_weight=0.0)
    if variant == "emissivity":
        # (a tenth of ckd_synth's absorption: the window g points see the surface, so the reflected downwelling flux is a part
        # of the cost - at thirty times, as elsewhere in this file, the atmosphere is opaque and a grey surface changes the cost
        # by 1e-11 of itself, which no gradient check would see)
        kw = dict(emissivity=(0.7, 0.95, 1.0), boundary=True, spectral_boundary_weight=0.3, absorb=0.1)
    model, scenes, cfg, orc = _problem(oracle, nangle, seed=3, **kw)
    assert scenes[1]["gas_present"].min() == 0                                # a gas absent from a scene
    opt = _opt(ctx, model, scenes, cfg, nangle)
    x, free, rs = _state(opt, orc, 1, negative_od=variant == "negative_od")
    if variant == "thin_top_layer":
        # the top layer holds 0.1 Pa: its weak g points take the thin branch at every angle, its strong ones the thick one, and
        # some change branch between the angles
        for s in scenes:
            eps, _ = olr.layer_terms(np.maximum(orc.optical_depth(x, s), 0.0)[:, 0], orc.sec)
            thick = eps > olr.THIN_EPS
            assert thick.any() and (~thick).any() and np.any(thick.any(axis=0) & ~thick.all(axis=0))
    if variant == "negative_od":
        neg = np.concatenate([orc.optical_depth(x, s).ravel() for s in scenes]) < 0
        assert 0.3 < neg.mean() < 0.7
    if variant not in ("thin_top_layer", "emissivity"):
        # (in those two the fluxes of the top levels are sums of terms with five digits fewer than a double, see _problem: cost
        # and gradient, which take them absolutely, are held to their bounds below)
        _check_forward(ctx, opt, orc, scenes, x, nangle)
    if variant == "emissivity":
        # the surface rule on the device's own angle-summed fluxes
        _, fl = opt.forward(x)
        c0 = 0
        for s in scenes:
            for c in range(s["pressure_hl"].shape[0]):
                es, b = orc.emissivity_g(s, c), orc.planck(s["temperature_hl"][c])[-1]
                assert np.allclose(fl[c0 + c, 1, -1], es * b + (1.0 - es) * fl[c0 + c, 0, -1], rtol=1e-12, atol=0)
            c0 += s["pressure_hl"].shape[0]
    J, g = _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs)
    if variant == "emissivity":
        # the reflected downwelling flux is a part of the cost that the gradient has to carry: with a black surface it differs
        black = olr.OracleLwAngles(oracle, model, [dict(s, surf_emissivity=None) for s in scenes], cfg, orc.sec, orc.wgt)
        assert abs(black.cost_rt(x) - orc.cost_rt(x)) > 1e-6 * abs(J)
    opt.close()


def test_relative_to_fluxes(ctx, oracle):
    nangle = 4
    model, scenes, cfg, orc = _problem(oracle, nangle, seed=9, boundary=True, spectral_boundary_weight=0.3)
    base, pert = scenes[0], scenes[1]
    pert = dict(pert, pressure_hl=base["pressure_hl"], temperature_hl=base["temperature_hl"])   # same profiles, other gases
    ref_opt = _opt(ctx, model, [dict(base)], cfg, nangle)
    _, fl = ref_opt.forward(ref_opt.initial_state(), unclamped=True)        # the relative-to scene through an angle handle
    ref_opt.close()
    fl_ref = olr.OracleLwAngles(oracle, model, [base], cfg, orc.sec, orc.wgt).fluxes(orc.x0, base, unclamped=True)
    assert np.allclose(fl, fl_ref, rtol=1e-10, atol=1e-300)
    truth = olr.OracleLwAngles(oracle, model, [pert], cfg, orc.sec, orc.wgt)
    f_p, f_b = truth.fluxes(truth.x0 + 0.1, pert), truth.fluxes(truth.x0 + 0.1, base)
    bf = _bands(model, f_p) - _bands(model, f_b)
    train = dict(pert, flux_dn=np.ascontiguousarray(bf[:, 0]), flux_up=np.ascontiguousarray(bf[:, 1]),
                 relative_flux_dn=np.ascontiguousarray(fl[:, 0]), relative_flux_up=np.ascontiguousarray(fl[:, 1]),
                 spectral_flux_dn_surf=np.ascontiguousarray(f_p[:, 0, -1] - f_b[:, 0, -1]),
                 spectral_flux_up_toa=np.ascontiguousarray(f_p[:, 1, 0] - f_b[:, 1, 0]))
    o2 = olr.OracleLwAngles(oracle, model, [train], cfg, orc.sec, orc.wgt)
    opt = _opt(ctx, model, [train], cfg, nangle)
    x, free, rs = _state(opt, o2, 2)
    J, g = _check_cost_and_gradient(opt, o2, cfg, [train], x, free, rs)
    plain = dict(train, relative_flux_dn=None, relative_flux_up=None)
    assert abs(olr.OracleLwAngles(oracle, model, [plain], cfg, orc.sec, orc.wgt).cost_rt(x) - o2.cost_rt(x)) > 1e-6 * abs(J)
    opt.close()


def test_nangle_zero_is_the_two_stream_handle(ctx, oracle):
    from ecckd_amd import api
    model, scenes, cfg, orc = _problem(oracle, 4, seed=3, boundary=True, spectral_boundary_weight=0.3)
    a, b = api.Optimizer(ctx, model, scenes, **cfg), _opt(ctx, model, scenes, cfg, 0)
    assert a.nangle == 0 and b.nangle == 0 and a.forward_plan() == b.forward_plan() and a.forward_plan()["kernel"] == "cells"
    x, _, _ = _state(a, orc, 4)
    (Ja, ga), (Jb, gb) = a.cost_grad(x), b.cost_grad(x)
    assert Ja == Jb and np.array_equal(ga, gb)
    # and it is the two-stream model: the single angle 1.66 of the numpy restatement
    two = olr.OracleLwAngles(oracle, model, scenes, cfg, [1.66], [1.0])
    assert Ja == pytest.approx(_cost(two, cfg, x), rel=olr.COST_REL_TOL)
    # one angle of the quadrature (sec = 2) is another model
    c = _opt(ctx, model, scenes, cfg, 1)
    assert abs(c.cost_grad(x, False) - Ja) > 1e-6 * abs(Ja)
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("nangle", [3, 16])
def test_block_sizes_agree(ctx, oracle, nangle, monkeypatch):
    """the default, 192 and 64 threads on one handle: 16, 3 and 1 layer groups share the angles and the cells differently, and
    agree as the existing kernels do across block sizes (tests/test_optimize_edges_gpu.py)"""
    model, scenes, cfg, orc = _problem(oracle, nangle, seed=3, boundary=True, spectral_boundary_weight=0.3)
    opt = _opt(ctx, model, scenes, cfg, nangle)
    x, _, _ = _state(opt, orc, 5)
    out = {}
    for threads in (None, 192, 64):
        if threads:
            monkeypatch.setenv("ECCKD_K8A_THREADS", str(threads))
        assert opt.forward_plan()["threads"] == 64 * ((threads or 1024) // 64) and opt.forward_plan()["lgroups"] == (threads or 1024) // 64
        out[threads] = opt.cost_grad(x)
        again = opt.cost_grad(x)
        assert out[threads][0] == again[0] and np.array_equal(out[threads][1], again[1])
    J0, g0 = out[None]
    for threads in (192, 64):
        J, g = out[threads]
        assert J == pytest.approx(J0, rel=1e-13)
        assert np.allclose(g, g0, rtol=1e-9, atol=1e-12 * np.abs(g0).max())
    opt.close()


def test_minimize_under_the_quadrature_beats_two_stream_training(ctx, oracle):
    """40 iterations at nangle = 4 on the 12-g, 18-layer problem: the cost falls, and ends below that of the same start trained
    two-stream for 40 iterations and then scored under the quadrature - the two-stream bias the key exists to remove"""
    model, scenes, cfg, orc = _problem(oracle, 4, seed=7)
    opt4, opt0 = _opt(ctx, model, scenes, cfg, 4), _opt(ctx, model, scenes, cfg, 0)
    x0 = opt4.initial_state()
    J_start = opt4.cost_grad(x0, False)
    res4 = opt4.minimize(max_iterations=40, convergence_criterion=0.0, bounded=True)
    res0 = opt0.minimize(max_iterations=40, convergence_criterion=0.0, bounded=True)
    assert res4["status"] < 6 and res0["status"] < 6
    J4 = opt4.cost_grad(res4["x"], False)
    J0_scored = opt4.cost_grad(res0["x"], False)
    print(f"start {J_start:.6g}; trained at nangle=4: {J4:.6g}; trained two-stream, scored at nangle=4: {J0_scored:.6g} "
          f"(its own two-stream cost {res0['cost']:.6g})")
    assert J4 == pytest.approx(res4["cost"], rel=1e-12) and J4 < J_start
    assert J4 < J0_scored
    assert _cost(orc, cfg, res4["x"]) == pytest.approx(J4, rel=1e-9)
    opt4.close(); opt0.close()


@pytest.mark.parametrize("case", ["negative", "seventeen", "shortwave_model", "rayleigh_scattering"])
def test_refusals(ctx, oracle, case):
    from ecckd_amd import EcckdError, api
    model, scenes, cfg, orc = _problem(oracle, 4, seed=1)
    kw = dict(nangle=4)
    if case == "negative":
        kw = dict(nangle=-1)
    if case == "seventeen":
        kw = dict(nangle=17)
    if case in ("shortwave_model", "rayleigh_scattering"):
        model = ckd_synth.make_model_sw(seed=1)
        scenes = ckd_synth.make_scenes_sw(model, np.array([0.15, 0.3, 0.06]))
        for s in scenes:
            shape = s["pressure_hl"].shape + (model["nband"],)
            s["flux_dn"], s["flux_up"] = np.ones(shape), np.ones(shape)
        if case == "rayleigh_scattering":
            kw = dict(nangle=4, rayleigh_scattering=True)
    with pytest.raises(EcckdError) as e:
        api.Optimizer(ctx, model, scenes, **kw, **cfg)
    assert e.value.code == 147 and "nangle" in str(e.value)                # ECCKD_PARAMETER_ERROR, the message names the key
    # the context is as usable as before: nothing was launched or left behind
    m2, s2, c2, o2 = _problem(oracle, 4, seed=1)
    opt = _opt(ctx, m2, s2, c2, 4)
    assert np.isfinite(opt.cost_grad(opt.initial_state(), False))
    opt.close()
