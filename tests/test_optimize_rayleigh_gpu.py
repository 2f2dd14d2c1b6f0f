"""The optimiser with the Rayleigh-scattering two-stream transfer (ECCKD_OPT_RAYLEIGH_SCATTERING, api.Optimizer(...,
rayleigh_scattering=True)): k_opt_forward_adjoint_rayleigh against the numpy float64 restatement of tests/opt_rayleigh_ref.py -
forward fluxes, cost, the hand-derived adjoint against central differences of the NUMPY cost, every branch of rayleigh_layer
and of the shortwave cost, the minimiser, reproducibility and the refusals."""
import numpy as np
import pytest

import ckd_synth
import opt_rayleigh_ref as orr
import rayleigh_ref

pytestmark = pytest.mark.gpu

CFG = dict(flux_weight=0.2, flux_profile_weight=0.05, broadband_weight=0.4, spectral_boundary_weight=0.0,
           negative_od_penalty=1.0e4, pressure_weight_power=0.5, prior_error=4.0, pressure_corr=0.95,
           temperature_corr=0.95, conc_corr=0.9, cap_relative_linear=0.0)
MU0 = (1.0, 0.5, 0.25, 0.1)          # 0.5 sits on the resonance k mu0 = 1 of weakly scattering layers
FLUX_ABS = 1.0e-9                    # per unit incoming mu0 * ssi_g: tests/test_lbl_fluxes_sw_rayleigh_gpu.py


def _problem(oracle, seed=0, albedo=(0.15, 0.3, 0.06), boundary=False, ch4_low=False, ng=12, nband=3, nlay=18, nscene=2, ncol=2,
             rayleigh=None, absorb=1.0, mu0=MU0, **over):
    """A scattering training problem: the truth is a perturbed model's scattering fluxes (total dn, up)."""
    cfg = dict(CFG, **over)
    model = ckd_synth.make_model_sw(seed=seed, ng=ng, nband=nband)
    truth = ckd_synth.make_model_sw(seed=seed, ng=ng, nband=nband)
    rs = np.random.RandomState(seed + 5)
    for m in (model, truth):
        if rayleigh is not None:
            m["rayleigh_molar_scattering"] = rayleigh(m["rayleigh_molar_scattering"])
        for g in m["gases"]:
            for k in ("molar_abs", "min_molar_abs", "max_molar_abs"):
                g[k] = g[k] * absorb
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    bw = 0.02 * rs.uniform(size=ng) if boundary else None
    scenes = ckd_synth.make_scenes_sw(model, np.asarray(albedo, dtype=np.float64)[:nband], mu0=mu0, boundary_weights=bw,
                                      ch4_low=ch4_low, nscene=nscene, ncol=ncol, nlay=nlay)
    if nlay == 1:
        # ckd_synth's single layer would be the 4 Pa between 1 and 5 Pa: a heating rate per unit flux of 1 / (4 Pa), so large
        # that the float64 rounding of the NUMPY cost drowns its own finite differences.  The one layer spans the column.
        for s in scenes:
            s["pressure_hl"][:, 1] = 101325.0 - 2000.0 * (np.arange(s["pressure_hl"].shape[0]) // len(mu0))
    orc_truth = orr.OracleRayleigh(oracle, truth, scenes, cfg)
    for s in scenes:
        f = orc_truth.fluxes(orc_truth.x0, s)
        bf = np.stack([f[:, :, :, model["iband_per_g"] == b].sum(-1) for b in range(nband)], axis=-1)
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
        if boundary:
            s["spectral_flux_dn_surf"] = np.ascontiguousarray(f[:, 0, -1, :])
    return model, scenes, cfg, orr.OracleRayleigh(oracle, model, scenes, cfg)


def _opt(ctx, model, scenes, cfg, scattering=True):
    from ecckd_amd import api
    return api.Optimizer(ctx, model, scenes, rayleigh_scattering=scattering, **cfg)


def _state(opt, orc, seed, negative_od=False):
    rs = np.random.RandomState(seed)
    x0 = opt.initial_state()
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    if negative_od:
        sizes = np.cumsum([0] + orc.sizes)
        x[sizes[3]:sizes[4]] += 6.0          # ch4 below its reference: about half of the cells turn negative
    return x, free, rs


def _assert_off_branch_edges(orc, x, scenes):
    """No cell within 1e-3 (relative) of an edge of rayleigh_layer's branches, so that no finite difference (a relative change
    of the optical depths of 1e-5) straddles a kink: the distance of |1 - k mu0| from the edge 1e-4 of the resonance band, and
    the branch every cell takes - inside the band or not, each clamp of Rdir / Tdd below, between or at its bounds - is the
    same with all gas optical depths 1e-3 smaller and 1e-3 larger."""
    for s in scenes:
        t = orc.layer_terms(x, s)
        edge = np.abs(np.abs(1.0 - t["km"]) - rayleigh_ref.RESONANCE_H)
        assert np.all(edge[t["scat"]] > 1e-3 * rayleigh_ref.RESONANCE_H)
        for scale in (1.0 - 1e-3, 1.0 + 1e-3):
            assert np.array_equal(orc.layer_terms(x, s, scale)["branch"], t["branch"])


def _cost(orc, cfg, x):
    return orc.cost_rt(x) + orc.cost_prior(x, cfg["prior_error"])[0]


def _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs, ncoord=12):
    """checks 3, 4 and 7 of the issue at state x"""
    _assert_off_branch_edges(orc, x, scenes)
    J, g = opt.cost_grad(x)
    J2, g2 = opt.cost_grad(x)
    assert J == J2 and np.array_equal(g, g2)                                 # bit-identical run to run
    J_ref = _cost(orc, cfg, x)
    print(f"cost {J:.17g} numpy {J_ref:.17g} rel {abs(J - J_ref) / abs(J_ref):.3g}")
    assert J == pytest.approx(J_ref, rel=orr.COST_REL_TOL)
    assert np.all(g[~free] == 0.0)
    for trial in range(3):
        d = np.where(free, rs.normal(size=x.size), 0.0)
        d /= np.linalg.norm(d)
        h = 1e-5
        fd = (_cost(orc, cfg, x + h * d) - _cost(orc, cfg, x - h * d)) / (2 * h)
        print(f"direction {trial}: g.d {np.dot(g, d):.12g} fd {fd:.12g}")
        assert np.dot(g, d) == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    idx = rs.choice(np.nonzero(free)[0], min(ncoord, int(free.sum())), replace=False)
    for i in idx:
        h = 1e-5
        e = np.zeros_like(x); e[i] = h
        f1 = (_cost(orc, cfg, x + e) - _cost(orc, cfg, x - e)) / (2 * h)
        f2 = (_cost(orc, cfg, x + 0.5 * e) - _cost(orc, cfg, x - 0.5 * e)) / h
        fd = (4.0 * f2 - f1) / 3.0                                           # Richardson: h and h / 2
        print(f"coordinate {i}: g {g[i]:.12g} fd {fd:.12g}")
        assert g[i] == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    return J, g


def _check_forward(ctx, opt, orc, scenes, x):
    """check 1: the fluxes against the numpy restatement, the exact solver and the g-point kernel of the parent"""
    from ecckd_amd import api
    od, fl = opt.forward(x)
    c0 = 0
    for s in scenes:
        ncol = s["pressure_hl"].shape[0]
        ta, tr = np.maximum(orc.tau_abs_raw(x, s), 0.0), orc.tau_ray(s)
        assert np.allclose(od[c0:c0 + ncol], ta + tr, rtol=1e-12, atol=1e-300)
        ref = orc.fluxes(x, s)
        inc = (np.asarray(s["mu0"])[:, None] * orc.ssi(s)[None, :])[:, None, None, :]
        err = np.abs(fl[c0:c0 + ncol] - ref) / inc
        print(f"forward against numpy: {err.max():.3g} per unit incoming")
        assert err.max() <= FLUX_ABS
        alb = orc.albedo_g(s)
        for c in range(ncol):
            mu0 = float(s["mu0"][c])
            for g in range(0, ta.shape[2], max(1, ta.shape[2] // 4)):           # the exact solver is one column and g at a time
                d, v, u = rayleigh_ref.two_stream_exact(ta[c, :, g], tr[c, :, g], mu0, alb[g], 1.0)
                got = fl[c0 + c, :, :, g] / (mu0 * orc.ssi(s)[g])
                assert np.abs(got[0] - (d + v) / mu0).max() <= rayleigh_ref.EXACT_BOUND
                assert np.abs(got[1] - u / mu0).max() <= rayleigh_ref.EXACT_BOUND
            for a in np.unique(alb):                                              # the parent's kernel takes a scalar albedo
                gs = np.nonzero(alb == a)[0]
                _, dn, up = api.rt_sw_gpoints_rayleigh(ctx, mu0, a, orc.ssi(s)[None, gs], ta[c:c + 1][:, :, gs], tr[c:c + 1][:, :, gs])
                scale = (mu0 * orc.ssi(s))[gs]
                assert np.all(np.abs(fl[c0 + c, 0][:, gs] - dn[0]) <= FLUX_ABS * scale[None, :])
                assert np.all(np.abs(fl[c0 + c, 1][:, gs] - up[0]) <= FLUX_ABS * scale[None, :])
        c0 += ncol
    return fl


# ---- shapes: one layer, top and surface adjacent, lengths that are no multiple of a chunk or layer-group count; g points below,
#      at and above one wave; one band and several; two block sizes ----
@pytest.mark.parametrize("threads", [None, 192])
@pytest.mark.parametrize("nband", [1, 3])
@pytest.mark.parametrize("ng", [5, 64, 70])
@pytest.mark.parametrize("nlay", [1, 2, 9, 17])
def test_shapes(ctx, oracle, nlay, ng, nband, threads, monkeypatch):
    if threads:
        monkeypatch.setenv("ECCKD_K8A_THREADS", str(threads))
    model, scenes, cfg, orc = _problem(oracle, seed=3, ng=ng, nband=nband, nlay=nlay, nscene=1, ncol=2)
    opt = _opt(ctx, model, scenes, cfg)
    plan = opt.forward_plan()
    ngpad = (ng + 63) // 64 * 64
    assert plan["kernel"] == "rayleigh" and plan["rayleigh"] and not plan["cells"]
    assert plan["ngpad"] == ngpad and plan["threads"] == ngpad * max(1, (threads or 512) // ngpad)
    x, free, rs = _state(opt, orc, 6)          # (a seed that keeps every shape off the branch edges)
    _check_forward(ctx, opt, orc, scenes, x)
    _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs)
    opt.close()


def test_more_level_band_slots_than_threads(ctx, oracle, monkeypatch):
    """ECCKD_K8A_THREADS = 64, 9 bands, 8 layers: 81 (half level, band) slots on one wave, so the band sums, the residuals and
    the seeds of the cost phase each take a second round of the block; one layer group"""
    monkeypatch.setenv("ECCKD_K8A_THREADS", "64")
    model, scenes, cfg, orc = _problem(oracle, seed=3, ng=12, nband=9, nlay=8, nscene=1, ncol=2, albedo=np.linspace(0.3, 0.06, 9))
    opt = _opt(ctx, model, scenes, cfg)
    plan = opt.forward_plan()
    assert plan["kernel"] == "rayleigh" and plan["threads"] == 64 and plan["lgroups"] == 1
    x, free, rs = _state(opt, orc, 6)
    _check_forward(ctx, opt, orc, scenes, x)
    _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs)
    opt.close()


def test_degenerate_limit_matches_the_plain_shortwave_handle(ctx, oracle):
    """rayleigh_molar_scattering = 0: no diffuse light, the scattering handle's total downwelling is the plain handle's direct
    beam and the upwelling fluxes agree (the w = 0 branch of rayleigh_layer is the no-scattering transfer)"""
    model, scenes, cfg, orc = _problem(oracle, seed=2, rayleigh=lambda r: 0.0 * r)
    a, b = _opt(ctx, model, scenes, cfg), _opt(ctx, model, scenes, cfg, scattering=False)
    x, _, _ = _state(a, orc, 3)
    (od_a, fl_a), (od_b, fl_b) = a.forward(x), b.forward(x)
    assert np.array_equal(od_a, od_b)
    assert np.allclose(fl_a, fl_b, rtol=1e-10, atol=1e-300) and fl_b[:, 1].max() > 0
    a.close(); b.close()


VARIANTS = ["base", "spectral_only", "mixed_albedo", "albedo_zero", "one_g_without_rayleigh", "boundary", "negative_od", "resonance"]


def _variant_problem(oracle, variant, seed):
    kw = {}
    if variant == "spectral_only":
        kw = dict(broadband_weight=0.0)
    if variant == "mixed_albedo":
        kw = dict(albedo=(0.2, 0.0, 0.1))           # the broadband upwelling terms are dropped (:252, :264)
    if variant == "albedo_zero":
        kw = dict(albedo=(0.0, 0.0, 0.0))           # the upwelling is backscattered light alone
    if variant == "one_g_without_rayleigh":
        kw = dict(rayleigh=lambda r: np.where(np.arange(r.size) == 4, 0.0, r))
    if variant == "boundary":
        kw = dict(boundary=True)
    if variant == "negative_od":
        kw = dict(ch4_low=True)
    if variant == "resonance":                      # strong absorption, weak scattering: cells with w < 1.6e-4 at mu0 = 0.5 are inside
        kw = dict(rayleigh=lambda r: 1.0e-3 * r, absorb=30.0, mu0=(0.5, 0.5, 1.0, 0.25))
    return _problem(oracle, seed=seed, **kw)


@pytest.mark.parametrize("variant", VARIANTS)
def test_cost_and_gradient(ctx, oracle, variant):
    model, scenes, cfg, orc = _variant_problem(oracle, variant, seed=3)
    opt = _opt(ctx, model, scenes, cfg)
    x, free, rs = _state(opt, orc, 1, negative_od=variant == "negative_od")
    # every variant touches its branch
    terms = [orc.layer_terms(x, s) for s in scenes]
    if variant == "mixed_albedo":
        assert not np.all(scenes[0]["albedo"] > 0) and np.any(scenes[0]["albedo"] > 0)
    if variant == "one_g_without_rayleigh":
        assert all((~t["scat"][:, :, 4]).all() and t["scat"][:, :, 5].all() for t in terms)
    if variant == "negative_od":
        neg = np.concatenate([orc.tau_abs_raw(x, s).ravel() for s in scenes]) < 0
        assert neg.sum() > 10 and (~neg).sum() > 10          # clamped cells (penalty gradient alone) next to unclamped ones
    if variant == "resonance":
        inside = sum(int((t["scat"] & (np.abs(1.0 - t["km"]) < rayleigh_ref.RESONANCE_H)).sum()) for t in terms)
        assert inside >= 10, inside
    J, g = _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs)
    if variant == "albedo_zero":
        fl = _check_forward(ctx, opt, orc, scenes, x)
        assert fl[:, 1, 0].min() > 0.0                # light comes back from a black surface: it was scattered
    opt.close()


def test_cells_at_an_active_clamp(ctx, oracle):
    """The clamps of Rdir / Tdd are guards against rounding: over 1e-8 <= tau <= 300, 1e-8 <= w <= 1 - 1e-12 and mu0 from 0.05
    to 1 the numpy terms reach none of them but the upper bound of Tdd, 1 - Tdir - Rdir, and that only at conservative
    scattering, 1 - w <= 1e-8, where the closed form's cancellation (k -> 0) leaves Tdd up to 1e-12 above it in about a tenth
    of the cells.  One g point whose gases absorb 1e-12 as much puts cells there: rayleigh_layer_d's clamp branch runs.  Which
    cells are clamped is then a matter of the last bit, so the finite differences of the other tests cannot be taken here (their
    assertion on the clamp states would not hold, and must not be waived); the fluxes, the cost and the reproducibility are
    held to the same bounds, and the gradient is finite with its fixed elements at zero."""
    absorb = np.where(np.arange(12) == 7, 1.0e-12, 1.0)
    model, scenes, cfg, orc = _problem(oracle, seed=3, absorb=absorb)
    opt = _opt(ctx, model, scenes, cfg)
    x, free, rs = _state(opt, orc, 1)
    terms = [orc.layer_terms(x, s) for s in scenes]
    active = sum(int((t["branch"][1:] != 0).sum()) for t in terms)
    assert active > 0 and all((t["branch"][1:, :, :, np.arange(12) != 7] == 0).all() for t in terms), active
    assert max(t["w"][:, :, 7].min() for t in terms) > 1.0 - 1.0e-8
    _check_forward(ctx, opt, orc, scenes, x)
    J, g = opt.cost_grad(x)
    J2, g2 = opt.cost_grad(x)
    assert J == J2 and np.array_equal(g, g2)
    J_ref = _cost(orc, cfg, x)
    print(f"cost {J:.17g} numpy {J_ref:.17g} rel {abs(J - J_ref) / abs(J_ref):.3g}; {active} clamped terms")
    assert J == pytest.approx(J_ref, rel=orr.COST_REL_TOL)
    assert np.all(np.isfinite(g)) and np.all(g[~free] == 0.0) and np.any(g != 0.0)
    opt.close()


def test_relative_to_fluxes(ctx, oracle):
    model, scenes, cfg, orc = _problem(oracle, seed=9, boundary=True)
    base, pert = scenes[0], scenes[1]
    pert = dict(pert, pressure_hl=base["pressure_hl"], temperature_hl=base["temperature_hl"])   # same profiles, other gases
    ref_opt = _opt(ctx, model, [dict(base)], cfg)
    _, fl = ref_opt.forward(ref_opt.initial_state())            # fluxes of the relative-to scene through a scattering handle
    ref_opt.close()
    fl_ref = orr.OracleRayleigh(oracle, model, [base], cfg).fluxes(orc.x0, base)
    assert np.abs(fl - fl_ref).max() <= FLUX_ABS * 1361.0
    truth = orr.OracleRayleigh(oracle, model, [pert], cfg)
    nband = model["nband"]
    bands = lambda f: np.stack([f[:, :, :, model["iband_per_g"] == b].sum(-1) for b in range(nband)], axis=-1)
    f_p, f_b = truth.fluxes(truth.x0 + 0.1, pert), truth.fluxes(truth.x0 + 0.1, base)
    bf = bands(f_p) - bands(f_b)
    train = dict(pert, flux_dn=np.ascontiguousarray(bf[:, 0]), flux_up=np.ascontiguousarray(bf[:, 1]),
                 relative_flux_dn=np.ascontiguousarray(fl[:, 0]), relative_flux_up=np.ascontiguousarray(fl[:, 1]),
                 spectral_flux_dn_surf=np.ascontiguousarray(f_p[:, 0, -1] - f_b[:, 0, -1]))
    o2 = orr.OracleRayleigh(oracle, model, [train], cfg)
    opt = _opt(ctx, model, [train], cfg)
    x, free, rs = _state(opt, o2, 2)
    J, g = _check_cost_and_gradient(opt, o2, cfg, [train], x, free, rs)
    plain = dict(train, relative_flux_dn=None, relative_flux_up=None)
    assert abs(orr.OracleRayleigh(oracle, model, [plain], cfg).cost_rt(x) - o2.cost_rt(x)) > 1e-6 * abs(J)
    opt.close()


def test_minimize_reduces_cost(ctx, oracle):
    model, scenes, cfg, orc = _problem(oracle, seed=7)
    opt = _opt(ctx, model, scenes, cfg)
    x0 = opt.initial_state()
    J0, g0 = opt.cost_grad(x0)
    res = opt.minimize(max_iterations=150, convergence_criterion=1e-3 * np.linalg.norm(g0), bounded=True)
    assert res["status"] in (0, 2)
    assert res["cost"] < 0.5 * J0
    assert _cost(orc, cfg, res["x"]) == pytest.approx(res["cost"], rel=1e-9)
    opt.close()


@pytest.mark.parametrize("case", ["longwave_model", "no_rayleigh_coefficient", "scene_without_albedo"])
def test_refusals(ctx, oracle, case):
    from ecckd_amd import EcckdError
    model, scenes, cfg, orc = _problem(oracle, seed=1)
    if case == "longwave_model":
        model = ckd_synth.make_model(seed=1)
    if case == "no_rayleigh_coefficient":
        model = dict(model, rayleigh_molar_scattering=None)
    if case == "scene_without_albedo":
        scenes = [dict(s, albedo=None) for s in scenes]
    with pytest.raises(EcckdError) as e:
        _opt(ctx, model, scenes, cfg)
    assert e.value.code == 147                                             # ECCKD_PARAMETER_ERROR
    # the context is as usable as before: nothing was launched or left behind
    m2, s2, c2, o2 = _problem(oracle, seed=1)
    opt = _opt(ctx, m2, s2, c2)
    assert np.isfinite(opt.cost_grad(opt.initial_state(), False))
    opt.close()
