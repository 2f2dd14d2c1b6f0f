"""The per-g flux-profile term of the optimiser (ecckd_opt_set_gpoint_truth, api.Optimizer.set_gpoint_truth): every column adds
    J_gp = w sum_i hw_i sum_g [((dn[i][g] - rel_dn) - T_dn[i][g])^2 + ((up[i][g] - rel_up) - T_up[i][g])^2]
over all half levels, hw_i the mean of the normalised layer weights on either side of level i.  The reference is the numpy
restatement of tests/opt_lw_angles_ref.py (sec = [1.66], wgt = [1] is the two-stream cost) with this formula added on top of
cost_rt; the three kernels that carry the term - cell-parallel, general (ECCKD_K8A_GENERIC=1) and the angle quadrature - are
held to it, to each other and to themselves across block sizes."""
import numpy as np
import pytest

import ckd_synth
import opt_lw_angles_ref as olr
import test_optimize_lw_angles_gpu as base                       # its problem builder, kink condition and Richardson differences

pytestmark = pytest.mark.gpu

WEIGHT = 0.1                                                     # spectral_boundary_weight of the reference's longwave scripts


def scaled_weight(orc, cfg, x, truth, share=0.3):
    """The weight at which the term is `share` of the rest of the numpy cost at x.  The synthetic problems' cost is led by the
    heating rates (their weight is (86400 s)^2): at 0.1 the term is 1e-6 of it, 1e-8 in the one-layer column, and neither the cost
    nor the gradient check would see whether the kernels carry it.  An input of the tests, chosen from the reference alone."""
    return share * base._cost(orc, cfg, x) / gp_cost(orc, cfg, x, 1.0, truth)


# The step of the Richardson differences.  base._assert_off_kinks covers a change of every gas's optical depth by a factor within
# 1 -+ 1e-3, and exp(9e-4) - 1 = 9.004e-4, so no difference straddles a clamp or the thin-layer kink up to this step.  It is nine
# times base.FD_STEP because the rounding of the numpy cost, divided by the step, is the error of the difference: with the term
# at a third of the cost the one-layer column of 65 g points measured 1.7e-6 between the central and the extrapolated difference
# at 1e-4 (the device's derivative lay between the two), twice the absolute bound 1e-9 |J|; the truncation error is O(h^4) and
# was below 1e-11 at 1e-4 wherever the two differences agreed.
FD_STEP = 9.0e-4


def layer_weights(cfg, p):
    pw = cfg["pressure_weight_power"]
    lw = (np.sqrt(p[1:]) - np.sqrt(p[:-1])) if pw == 0.5 else (p[1:] ** pw - p[:-1] ** pw)
    return lw / lw.sum()


def level_weights(lw):
    """hw_i = 0.5 (lw[i-1] + lw[i]), half of the one layer at the two ends"""
    hw = np.zeros(lw.size + 1)
    hw[:-1] += 0.5 * lw
    hw[1:] += 0.5 * lw
    return hw


def gp_cost(orc, cfg, x, weight, truth):
    """the formula of the issue in numpy, from the restatement's own per-g fluxes"""
    J, c0 = 0.0, 0
    for s in orc.scenes:
        fl = orc.fluxes(x, s)
        rd, ru = s.get("relative_flux_dn"), s.get("relative_flux_up")
        for c in range(fl.shape[0]):
            hw = level_weights(layer_weights(cfg, s["pressure_hl"][c]))
            dn = fl[c, 0] - (rd[c] if rd is not None else 0.0)
            up = fl[c, 1] - (ru[c] if ru is not None else 0.0)
            J += weight * np.sum(hw[:, None] * ((dn - truth[c0 + c, 0]) ** 2 + (up - truth[c0 + c, 1]) ** 2))
        c0 += fl.shape[0]
    return float(J)


def total_cost(orc, cfg, x, weight, truth):
    return base._cost(orc, cfg, x) + (gp_cost(orc, cfg, x, weight, truth) if weight > 0.0 else 0.0)


def per_g_rms(fl, rel, truth):
    return float(np.sqrt(np.mean(((fl - rel) - truth) ** 2)))


def rel_of(scenes, nhl, ng):
    out = []
    for s in scenes:
        n = s["pressure_hl"].shape[0]
        if s.get("relative_flux_dn") is None:
            out.append(np.zeros((n, 2, nhl, ng)))
        else:
            out.append(np.stack([s["relative_flux_dn"], s["relative_flux_up"]], axis=1))
    return np.concatenate(out, axis=0)


def problem(oracle, nangle, relative=False, **kw):
    """base._problem (its band truth is a perturbed model's) with the oracle of `nangle` (0: two-stream, the single angle 1.66),
    optional relative fluxes (a third of the model's own at its first guess: any array serves, the cost only subtracts it) and
    a per-g truth: the restatement's fluxes of another state, minus the relative fluxes."""
    model, scenes, cfg, orc = base._problem(oracle, max(nangle, 1), **kw)
    sec, wgt = ([1.66], [1.0]) if nangle == 0 else olr.nodes(nangle)
    orc = olr.OracleLwAngles(oracle, model, scenes, cfg, sec, wgt)
    if relative:
        for s in scenes:
            f = orc.fluxes(orc.x0, s) / 3.0
            s["relative_flux_dn"], s["relative_flux_up"] = np.ascontiguousarray(f[:, 0]), np.ascontiguousarray(f[:, 1])
            bf = base._bands(model, f)
            s["flux_dn"], s["flux_up"] = s["flux_dn"] - bf[:, 0], s["flux_up"] - bf[:, 1]
    rs = np.random.RandomState(11)
    xt = orc.x0 + np.where(orc.x0 > -1.0e20, 0.15 * rs.normal(size=orc.x0.size), 0.0)
    truth = np.concatenate([orc.fluxes(xt, s) for s in scenes], axis=0)
    truth = truth - rel_of(scenes, truth.shape[2], truth.shape[3])
    return model, scenes, cfg, orc, np.ascontiguousarray(truth)


def handle(ctx, model, scenes, cfg, nangle, truth=None, weight=0.0):
    from ecckd_amd import api
    return api.Optimizer(ctx, model, scenes, nangle=nangle, gpoint_truth=truth, gpoint_profile_weight=weight, **cfg)


KERNELS = {"cells": (0, False), "general": (0, True), "angles1": (1, False), "angles3": (3, False)}


def select(monkeypatch, kernel, threads=None):
    nangle, generic = KERNELS[kernel]
    if generic:
        monkeypatch.setenv("ECCKD_K8A_GENERIC", "1")
    if threads:
        monkeypatch.setenv("ECCKD_K8A_THREADS", str(threads))
    return nangle


def check(opt, orc, cfg, scenes, x, free, rs, truth, ndir=2, ncoord=4):
    """base agreement first, then cost and gradient with the term against numpy"""
    base._assert_off_kinks(orc, x, scenes)
    weight = scaled_weight(orc, cfg, x, truth)
    opt.set_gpoint_truth(0.0, None)
    J_plain = opt.cost_grad(x, False)
    ref_plain = base._cost(orc, cfg, x)
    print(f"without the term: {J_plain:.17g} numpy {ref_plain:.17g}")
    assert J_plain == pytest.approx(ref_plain, rel=olr.COST_REL_TOL)          # the restatement agrees before it is extended
    opt.set_gpoint_truth(weight, truth)
    J, g = opt.cost_grad(x)
    J2, g2 = opt.cost_grad(x)
    assert J == J2 and np.array_equal(g, g2)                                  # bit-identical run to run
    J_ref = total_cost(orc, cfg, x, weight, truth)
    term = gp_cost(orc, cfg, x, weight, truth)
    print(f"with the term: {J:.17g} numpy {J_ref:.17g} rel {abs(J - J_ref) / abs(J_ref):.3g}; the term {term:.6g}")
    assert J == pytest.approx(J_ref, rel=olr.COST_REL_TOL)
    assert term > 0.2 * abs(J_ref)                                            # the term is a part of the cost that the checks see
    assert np.all(g[~free] == 0.0)
    for trial in range(ndir):
        d = np.where(free, rs.normal(size=x.size), 0.0)
        d /= np.linalg.norm(d)
        central, fd = base._richardson(lambda t: total_cost(orc, cfg, x + t * d, weight, truth), FD_STEP)
        print(f"direction {trial}: g.d {np.dot(g, d):.12g} central {central:.12g} Richardson {fd:.12g}")
        assert np.dot(g, d) == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    for i in rs.choice(np.nonzero(free)[0], min(ncoord, int(free.sum())), replace=False):
        e = np.zeros_like(x); e[i] = 1.0
        central, fd = base._richardson(lambda t: total_cost(orc, cfg, x + t * e, weight, truth), FD_STEP)
        print(f"coordinate {i}: g {g[i]:.12g} central {central:.12g} Richardson {fd:.12g}")
        assert g[i] == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    return J, g


VARIANTS = ["base", "relative", "negative_od", "boundary"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_cost_and_gradient(ctx, oracle, kernel, variant, monkeypatch):
    """the term beside every other term of the longwave cost, with relative fluxes, clamped cells and the per-g boundary term, on
    two scenes (the second lacks a gas of the model)"""
    nangle = select(monkeypatch, kernel)
    kw = {}
    if variant == "negative_od":
        kw = dict(ch4_low=True, negative_od_penalty=1.0e-11)                  # (see test_optimize_lw_angles_gpu.test_cost_and_gradient)
    if variant == "boundary":
        kw = dict(boundary=True, spectral_boundary_weight=0.3)
    model, scenes, cfg, orc, truth = problem(oracle, nangle, relative=variant == "relative", seed=3, **kw)
    opt = handle(ctx, model, scenes, cfg, nangle)
    assert opt.forward_plan()["kernel"] == {"cells": "cells", "general": "general"}.get(kernel, "lw_angles")
    x, free, rs = base._state(opt, orc, 1, negative_od=variant == "negative_od")
    if variant == "negative_od":
        neg = np.concatenate([orc.optical_depth(x, s).ravel() for s in scenes]) < 0
        assert 0.3 < neg.mean() < 0.7
    check(opt, orc, cfg, scenes, x, free, rs, truth)
    opt.close()


# nlay: the chunk of eight layers of the recurrences, its tail, and the one-layer column where hw = (0.5, 0.5); ng below, at and
# above one wave; one band and three; 64 threads and the default; always 2 scenes of 2 columns (the column offset across scenes).
# Every value of every parameter appears; at 64 threads the seven- and eight-layer columns run the eight-cells-per-thread instance.
EDGE_SHAPES = [(1, 3, 1, None), (1, 65, 3, 64), (7, 3, 3, 64), (7, 64, 1, None), (8, 64, 3, 64), (8, 65, 1, None), (9, 3, 1, None),
               (9, 64, 3, 64), (17, 65, 3, None), (17, 3, 3, 64)]


@pytest.mark.parametrize("nlay,ng,nband,threads", EDGE_SHAPES)
@pytest.mark.parametrize("kernel", ["cells", "general", "angles3"])
def test_edge_shapes(ctx, oracle, kernel, nlay, ng, nband, threads, monkeypatch):
    nangle = select(monkeypatch, kernel, threads)
    model, scenes, cfg, orc, truth = problem(oracle, nangle, seed=3, ng=ng, nband=nband, nlay=nlay, nscene=2, ncol=2)
    assert truth.shape == (4, 2, nlay + 1, ng)
    if nlay == 1:
        assert np.array_equal(level_weights(layer_weights(cfg, scenes[0]["pressure_hl"][0])), [0.5, 0.5])
    opt = handle(ctx, model, scenes, cfg, nangle)
    plan = opt.forward_plan()
    ngpad = (ng + 63) // 64 * 64
    if kernel == "cells" and (threads is None or (ngpad == 64 and nlay <= 8)):
        assert plan["kernel"] == "cells" and plan["nc_template"] == (8 if threads and nlay > 4 else 4)
    if kernel == "general":
        assert plan["kernel"] == "general"
    if kernel == "angles3":
        assert plan["kernel"] == "lw_angles"
    x, free, rs = base._state(opt, orc, 6)
    check(opt, orc, cfg, scenes, x, free, rs, truth, ndir=1, ncoord=3)
    opt.close()


def test_kernels_and_block_sizes_agree(ctx, oracle, monkeypatch):
    """with the term: cell-parallel against general, and each of the three kernels across block sizes, at the tolerance the
    kernels have always been held to across block sizes"""
    out = {}
    for nangle in (0, 3):
        model, scenes, cfg, orc, truth = problem(oracle, nangle, seed=3, boundary=True, spectral_boundary_weight=0.3, relative=True)
        opt = handle(ctx, model, scenes, cfg, nangle)
        x, _, _ = base._state(opt, orc, 5)
        opt.set_gpoint_truth(scaled_weight(orc, cfg, x, truth), truth)
        for generic in ((False, True) if nangle == 0 else (False,)):
            for threads in (None, 192, 64):
                monkeypatch.delenv("ECCKD_K8A_THREADS", raising=False)
                monkeypatch.delenv("ECCKD_K8A_GENERIC", raising=False)
                if threads:
                    monkeypatch.setenv("ECCKD_K8A_THREADS", str(threads))
                if generic:
                    monkeypatch.setenv("ECCKD_K8A_GENERIC", "1")
                kernel = opt.forward_plan()["kernel"]
                assert kernel == ("lw_angles" if nangle else "general" if generic else kernel)
                out[(nangle, generic, threads)] = (kernel,) + opt.cost_grad(x)
        opt.close()
    assert out[(0, False, None)][0] == "cells" and out[(0, False, 192)][0] == "cells"
    for nangle, ref_key in ((0, (0, False, None)), (3, (3, False, None))):
        _, J0, g0 = out[ref_key]
        for key, (kernel, J, g) in out.items():
            if key[0] != nangle or key == ref_key:
                continue
            print(key, kernel, J, J0, np.abs(g - g0).max() / np.abs(g0).max())
            assert J == pytest.approx(J0, rel=1e-13)
            assert np.allclose(g, g0, rtol=1e-9, atol=1e-12 * np.abs(g0).max())


@pytest.mark.parametrize("kernel", ["cells", "general", "angles3"])
def test_term_vanishes_on_its_own_fluxes(ctx, oracle, kernel, monkeypatch):
    nangle = select(monkeypatch, kernel)
    model, scenes, cfg, orc, truth = problem(oracle, nangle, seed=3, relative=True)
    opt = handle(ctx, model, scenes, cfg, nangle)
    x, _, _ = base._state(opt, orc, 2)
    J0, g0 = opt.cost_grad(x)
    _, fl = opt.forward(x)
    # (the weight at which the term is a third of the cost on the problem's truth; on the handle's own fluxes it leaves nothing)
    opt.set_gpoint_truth(scaled_weight(orc, cfg, x, truth), fl - rel_of(scenes, fl.shape[2], fl.shape[3]))
    J, g = opt.cost_grad(x)
    assert J == pytest.approx(J0, rel=olr.COST_REL_TOL)
    assert np.allclose(g, g0, rtol=1e-9, atol=1e-12 * np.abs(g0).max())
    opt.close()


@pytest.mark.parametrize("kernel", ["cells", "general", "angles3"])
def test_removing_the_term_restores_the_handle(ctx, oracle, kernel, monkeypatch):
    nangle = select(monkeypatch, kernel)
    model, scenes, cfg, orc, truth = problem(oracle, nangle, seed=3, boundary=True, spectral_boundary_weight=0.3)
    fresh = handle(ctx, model, scenes, cfg, nangle)
    x, _, _ = base._state(fresh, orc, 2)
    weight = scaled_weight(orc, cfg, x, truth)
    opt = handle(ctx, model, scenes, cfg, nangle, truth, weight)
    Jf, gf = fresh.cost_grad(x)
    J1, g1 = opt.cost_grad(x)
    assert J1 != Jf and not np.array_equal(g1, gf)
    opt.set_gpoint_truth(0, None)
    J2, g2 = opt.cost_grad(x)
    assert J2 == Jf and np.array_equal(g2, gf)                               # bit-identical to a handle that never had the term
    assert opt.forward_plan() == fresh.forward_plan()
    opt.set_gpoint_truth(weight, truth)                                       # and back
    J3, g3 = opt.cost_grad(x)
    assert J3 == J1 and np.array_equal(g3, g1)
    opt.set_gpoint_truth(-1.0, truth)                                         # a weight <= 0 removes it as well
    assert opt.cost_grad(x, False) == Jf
    opt.close(); fresh.close()


@pytest.mark.parametrize("kernel", ["cells", "general", "angles3"])
def test_linear_in_the_weight(ctx, oracle, kernel, monkeypatch):
    nangle = select(monkeypatch, kernel)
    model, scenes, cfg, orc, truth = problem(oracle, nangle, seed=3)
    opt = handle(ctx, model, scenes, cfg, nangle)
    x, _, _ = base._state(opt, orc, 2)
    J0 = opt.cost_grad(x, False)
    weight = scaled_weight(orc, cfg, x, truth)
    opt.set_gpoint_truth(weight, truth)
    J1 = opt.cost_grad(x, False)
    opt.set_gpoint_truth(2 * weight, truth)
    J2 = opt.cost_grad(x, False)
    term = J1 - J0
    # (J0 is rounded at 1e-16 of itself and enters both differences: the term is a third of it, so 1e-10 of the term bounds the term)
    assert term > 0.2 * abs(J0)
    assert (J2 - J0) == pytest.approx(2.0 * term, rel=1e-10)
    opt.close()


@pytest.mark.parametrize("case", ["shortwave", "rayleigh_scattering", "optimize_rayleigh", "nan_truth", "inf_weight", "wrong_shape",
                                  "weight_without_truth", "truth_without_weight"])
def test_refusals(ctx, oracle, case):
    from ecckd_amd import EcckdError, api
    if case in ("shortwave", "rayleigh_scattering", "optimize_rayleigh"):
        model = ckd_synth.make_model_sw(seed=1)
        scenes = ckd_synth.make_scenes_sw(model, np.array([0.15, 0.3, 0.06]))
        for s in scenes:
            shape = s["pressure_hl"].shape + (model["nband"],)
            s["flux_dn"], s["flux_up"] = np.ones(shape), np.ones(shape)
        kw = {"rayleigh_scattering": dict(rayleigh_scattering=True), "optimize_rayleigh": dict(optimize_rayleigh=True)}.get(case, {})
        opt = api.Optimizer(ctx, model, scenes, **kw, **base.CFG)
        with pytest.raises(EcckdError) as e:
            opt.set_gpoint_truth(WEIGHT, np.ones((opt.ncol, 2, opt.nlay + 1, opt.ng)))
        assert e.value.code == 147 and "ecckd_opt_set_gpoint_truth" in str(e.value)
        assert np.isfinite(opt.cost_grad(opt.initial_state(), False))         # the handle is as usable as before
        opt.close()
        return
    model, scenes, cfg, orc, truth = problem(oracle, 0, seed=1)
    if case == "weight_without_truth":
        with pytest.raises(ValueError):
            handle(ctx, model, scenes, cfg, 0, None, WEIGHT)
        return
    if case == "truth_without_weight":
        with pytest.raises(ValueError):
            handle(ctx, model, scenes, cfg, 0, truth, 0.0)
        return
    opt = handle(ctx, model, scenes, cfg, 0)
    J0 = opt.cost_grad(opt.initial_state(), False)
    if case == "nan_truth":
        bad = truth.copy()
        bad[-1, -1, -1, -1] = np.nan
        with pytest.raises(EcckdError) as e:
            opt.set_gpoint_truth(WEIGHT, bad)
        assert e.value.code == 147 and "not finite" in str(e.value)
    if case == "inf_weight":
        with pytest.raises(EcckdError) as e:
            opt.set_gpoint_truth(np.inf, truth)
        assert e.value.code == 147 and "not finite" in str(e.value)
    if case == "wrong_shape":
        with pytest.raises(ValueError):
            opt.set_gpoint_truth(WEIGHT, truth[:, :, :-1])
        with pytest.raises(ValueError):
            opt.set_gpoint_truth(WEIGHT, truth.reshape(-1))
    assert opt.cost_grad(opt.initial_state(), False) == J0                    # a refused call leaves the handle without the term
    opt.close()


@pytest.mark.parametrize("nangle", [0, 3])
def test_training(ctx, oracle, nangle):
    """Truth: the device's own forward model at a perturbed state of the model, so band fluxes, boundary fluxes and per-g profiles
    are consistent with one another and the model can reach them.  The perturbation is +0.4 and -0.4 in ln k on alternating g
    points, all nodes of all gases alike: the errors of neighbouring g points of a band have opposite signs, which is what the
    band sums let cancel and the term sees (the issue's motive).  40 iterations from the first guess, with and without the term:
    the per-g flux RMS against the truth falls from its starting value and ends lower with the term.  The RMS of the two end
    states is formed a second time from the numpy restatement's fluxes, and orders the same way there."""
    model, scenes, cfg, orc, _ = problem(oracle, nangle, seed=7)
    cfg = dict(cfg, spectral_boundary_weight=0.0)
    probe = handle(ctx, model, scenes, cfg, nangle)
    x0 = probe.initial_state()
    ng = probe.ng
    sign = np.where(np.arange(ng) % 2 == 0, 1.0, -1.0)
    xt = np.where(x0 > -1.0e20, x0 + 0.4 * np.tile(sign, x0.size // ng), x0)
    _, truth = probe.forward(xt)
    probe.close()
    c0 = 0
    for s in scenes:
        n = s["pressure_hl"].shape[0]
        bf = base._bands(model, truth[c0:c0 + n])
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
        c0 += n
    zero = np.zeros_like(truth)
    ends = {}
    for with_term in (False, True):
        opt = handle(ctx, model, scenes, cfg, nangle)
        start = per_g_rms(opt.forward(x0)[1], zero, truth)
        if with_term:
            # the weight at which the term starts as large as the rest of the cost (at 0.1 it would be 1e-6 of it, see scaled_weight)
            J_plain = opt.cost_grad(x0, False)
            opt.set_gpoint_truth(1.0, truth)
            opt.set_gpoint_truth(J_plain / (opt.cost_grad(x0, False) - J_plain), truth)
        res = opt.minimize(max_iterations=40, convergence_criterion=0.0, bounded=True)
        assert res["status"] < 6
        ends[with_term] = (per_g_rms(opt.forward(res["x"])[1], zero, truth), res["x"])
        opt.close()
    orc = olr.OracleLwAngles(oracle, model, scenes, cfg, orc.sec, orc.wgt)
    numpy_rms = {k: per_g_rms(np.concatenate([orc.fluxes(v[1], s) for s in scenes], axis=0), zero, truth) for k, v in ends.items()}
    print(f"per-g flux RMS: start {start:.6g}, without the term {ends[False][0]:.6g}, with it {ends[True][0]:.6g}; numpy {numpy_rms}")
    assert ends[False][0] < start and ends[True][0] < start
    assert ends[True][0] < ends[False][0]
    assert numpy_rms[True] < numpy_rms[False]
