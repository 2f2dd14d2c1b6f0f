"""The optimiser with optimised Rayleigh coefficients (ECCKD_OPT_RAYLEIGH_ACTIVE, api.Optimizer(..., optimize_rayleigh=True)),
on both shortwave forward models: the plain handle (Rayleigh one more absorber before the clamp; reference: the C oracle's
cost) and the scattering handle (tau_ray beside tau_abs in the two-stream layer terms; reference: the numpy cost of
tests/opt_rayleigh_ref.py), both through tests/opt_rayleigh_active_ref.py.  The gradient is always compared with differences
of the REFERENCE's cost, never with the code under test."""
import numpy as np
import pytest

import ckd_synth
import opt_rayleigh_active_ref as oar
import opt_rayleigh_ref as orr
import rayleigh_ref

pytestmark = pytest.mark.gpu

CFG = dict(flux_weight=0.2, flux_profile_weight=0.05, broadband_weight=0.4, spectral_boundary_weight=0.0,
           negative_od_penalty=1.0e4, pressure_weight_power=0.5, prior_error=4.0, pressure_corr=0.95,
           temperature_corr=0.95, conc_corr=0.9, cap_relative_linear=0.0)
MU0 = (1.0, 0.5, 0.25, 0.1)          # 0.5 sits on the resonance k mu0 = 1 of weakly scattering layers
HANDLES = ["plain", "scattering"]
MIN_X = -1.0e20


def _ref(handle):
    return oar.ScatteringActive if handle == "scattering" else oar.PlainActive


def _band_fluxes(model, f, nband):
    return np.stack([f[:, :, :, model["iband_per_g"] == b].sum(-1) for b in range(nband)], axis=-1)


def _problem(oracle, handle, seed=0, albedo=(0.15, 0.3, 0.06), boundary=False, ch4_low=False, ng=12, nband=3, nlay=18, nscene=2, ncol=2,
             rayleigh=None, absorb=1.0, mu0=MU0, ray_sigma=0.0, gases_active=True, truth_ray=0.25, **over):
    """A training problem of either handle: the truth is a perturbed model's fluxes - the gases' coefficients times
    exp(0.25 N(0, 1)) (left alone when no gas is active) and the Rayleigh coefficients times exp(truth_ray N(0, 1))."""
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
            g["active"] = bool(gases_active)
    if gases_active:
        for g in truth["gases"]:
            g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    truth["rayleigh_molar_scattering"] = truth["rayleigh_molar_scattering"] * np.exp(truth_ray * rs.normal(size=ng))
    bw = 0.02 * rs.uniform(size=ng) if boundary else None
    scenes = ckd_synth.make_scenes_sw(model, np.asarray(albedo, dtype=np.float64)[:nband], mu0=mu0, boundary_weights=bw,
                                      ch4_low=ch4_low, nscene=nscene, ncol=ncol, nlay=nlay)
    if nlay == 1:
        # (as tests/test_optimize_rayleigh_gpu.py: the one layer spans the column, not the 4 Pa at the top)
        for s in scenes:
            s["pressure_hl"][:, 1] = 101325.0 - 2000.0 * (np.arange(s["pressure_hl"].shape[0]) // len(mu0))
    orc_truth = _ref(handle)(oracle, truth, scenes, cfg)
    for s in scenes:
        f = orc_truth.fluxes(orc_truth.x0, s)
        bf = _band_fluxes(model, f, nband)
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
        if boundary:
            s["spectral_flux_dn_surf"] = np.ascontiguousarray(f[:, 0, -1, :])
    return model, scenes, cfg, _ref(handle)(oracle, model, scenes, cfg, ray_sigma=ray_sigma), truth


def _opt(ctx, model, scenes, cfg, handle, active=True, ray_sigma=0.0):
    from ecckd_amd import api
    kw = dict(optimize_rayleigh=True, rayleigh_prior_error=ray_sigma) if active else {}
    return api.Optimizer(ctx, model, scenes, rayleigh_scattering=handle == "scattering", **kw, **cfg)


def _state(opt, orc, seed, negative_od=False):
    rs = np.random.RandomState(seed)
    x0 = opt.initial_state()
    assert np.allclose(x0, orc.x0, rtol=1e-14, atol=0.0)
    free = x0 > MIN_X
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    if negative_od:
        sizes = np.cumsum([0] + orc.sizes)
        x[sizes[3]:sizes[4]] += 6.0          # ch4 below its reference: about half of the cells turn negative
    return x, free, rs


def _assert_off_branch_edges(orc, x, scenes, but_conservative=False):
    """The branch-edge check of tests/test_optimize_rayleigh_gpu.py - no cell within 1e-3 (relative) of an edge of
    rayleigh_layer's branches - with the gas optical depths AND, since the new coordinates move w through tau_ray, the Rayleigh
    optical depths scaled by 1 -+ 1e-3.  but_conservative: the cells whose gas optical depth was clamped (w = 1 exactly) are
    left out; returns how many of them sit at a clamp of Rdir / Tdd."""
    at_clamp = 0
    for s in scenes:
        t = orc.layer_terms(x, s)
        keep = np.ones(t["scat"].shape, dtype=bool)
        if but_conservative:
            keep = orc.tau_abs_raw(x, s) >= 0.0
            at_clamp += int((t["branch"][1:][:, ~keep] != 0).sum())
        edge = np.abs(np.abs(1.0 - t["km"]) - rayleigh_ref.RESONANCE_H)
        assert np.all(edge[t["scat"] & keep] > 1e-3 * rayleigh_ref.RESONANCE_H)
        for scale in (1.0 - 1e-3, 1.0 + 1e-3):
            assert np.array_equal(orc.layer_terms(x, s, scale)["branch"][:, keep], t["branch"][:, keep])
            orc.ray_scale = scale
            try:
                assert np.array_equal(orc.layer_terms(x, s)["branch"][:, keep], t["branch"][:, keep])
            finally:
                orc.ray_scale = 1.0
    return at_clamp


def _cost(orc, cfg, x):
    return orc.cost_rt(x) + orc.cost_prior(x, cfg["prior_error"])[0]


def _richardson(orc, cfg, x, i, h=1e-5):
    e = np.zeros_like(x); e[i] = h
    f1 = (_cost(orc, cfg, x + e) - _cost(orc, cfg, x - e)) / (2 * h)
    f2 = (_cost(orc, cfg, x + 0.5 * e) - _cost(orc, cfg, x - 0.5 * e)) / h
    return (4.0 * f2 - f1) / 3.0                                             # h and h / 2


def _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs, handle, ncoord=12, but_conservative=False):
    """cost to orr.COST_REL_TOL; the gradient against three central differences along random directions and Richardson
    differences per coordinate - 12 gas coordinates and the tail's (all ng of them at ng = 5, else 12) - at rel = 2e-6,
    abs = 1e-9 |J|; pinned elements exactly 0; two evaluations bit-identical"""
    if handle == "scattering":
        at_clamp = _assert_off_branch_edges(orc, x, scenes, but_conservative)
        if but_conservative:
            print(f"{at_clamp} layer terms of clamped cells (w = 1) sit at a clamp of Rdir / Tdd")
    J, g = opt.cost_grad(x)
    J2, g2 = opt.cost_grad(x)
    assert J == J2 and np.array_equal(g, g2)                                 # bit-identical run to run
    J_ref = _cost(orc, cfg, x)
    print(f"cost {J:.17g} reference {J_ref:.17g} rel {abs(J - J_ref) / abs(J_ref):.3g}")
    assert J == pytest.approx(J_ref, rel=orr.COST_REL_TOL)
    assert np.all(g[~free] == 0.0) and np.all(np.isfinite(g))
    ng, nx = orc.ng, x.size
    tail = np.arange(nx - ng, nx)
    for trial in range(3):
        d = np.where(free, rs.normal(size=nx), 0.0)
        d[tail] *= np.sqrt((nx - ng) / ng) if nx > ng else 1.0               # the tail weighs as much as the gases in the direction
        d /= np.linalg.norm(d)
        h = 1e-5
        fd = (_cost(orc, cfg, x + h * d) - _cost(orc, cfg, x - h * d)) / (2 * h)
        print(f"direction {trial}: g.d {np.dot(g, d):.12g} fd {fd:.12g}")
        assert np.dot(g, d) == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    gas_free = np.nonzero(free[:nx - ng])[0]
    idx = list(rs.choice(gas_free, min(ncoord, gas_free.size), replace=False)) if gas_free.size else []
    tail_free = tail[free[tail]]
    idx += list(tail_free if ng <= 5 else rs.choice(tail_free, min(12, tail_free.size), replace=False))
    for i in idx:
        fd = _richardson(orc, cfg, x, i)
        print(f"coordinate {i}{' (tail)' if i >= nx - ng else ''}: g {g[i]:.12g} fd {fd:.12g}")
        assert g[i] == pytest.approx(fd, rel=2e-6, abs=1e-9 * abs(J))
    return J, g


# ---- 1. layout ----
def test_layout(ctx, oracle):
    model, scenes, cfg, orc, _ = _problem(oracle, "plain", seed=3, rayleigh=lambda r: np.where(np.arange(r.size) == 4, 0.0, r))
    assert all(g.get("min_molar_abs") is not None for g in model["gases"])       # min / max tables present
    ng = model["ng"]
    b = _opt(ctx, model, scenes, cfg, "plain")
    xb, lo, hi = b.initial_state(bounds=True)
    k = np.asarray(model["rayleigh_molar_scattering"])
    assert np.array_equal(xb[-ng:], np.where(k > 0, np.log(np.where(k > 0, k, 1.0)), MIN_X)) and xb[b.nx - ng + 4] == MIN_X
    # An optimised coefficient reaches the kernels as exp(ln k), the Rayleigh ones of a handle with the flag like the gases' of
    # every handle, and exp(ln k) is k only to a unit or so in the last place.  The handle without the flag, which reads its
    # Rayleigh coefficients as they are, is therefore given the ones the handle with the flag uses at its first guess:
    # rayleigh_coefficients(x) returns what the device formed from x for the forward kernels.
    k_dev = b.rayleigh_coefficients(xb)
    assert np.allclose(k_dev, k, rtol=1e-14, atol=0.0) and k_dev[4] == 0.0
    a = _opt(ctx, dict(model, rayleigh_molar_scattering=k_dev), scenes, cfg, "plain", active=False)
    assert b.nx == a.nx + ng and not a.rayleigh_plan()["active"] and b.rayleigh_plan()["active"]
    xa = a.initial_state()
    assert np.array_equal(xb[:a.nx], xa)
    assert np.all(lo[a.nx:] == -np.inf) and np.all(hi[a.nx:] == np.inf) and np.all(np.isfinite(hi[:a.nx][xa > MIN_X]))
    assert np.array_equal(a.rayleigh_coefficients(), k_dev) and np.array_equal(a.rayleigh_coefficients(xa), k_dev)
    assert np.array_equal(a.forward(xa)[0], b.forward(xb)[0])
    # a plain handle launches the same forward kernels with and without the flag
    assert a.forward_plan() == b.forward_plan()
    (Ja, ga), (Jb, gb) = a.cost_grad(xa), b.cost_grad(xb)
    assert Ja == Jb and np.array_equal(ga, gb[:a.nx]) and gb[a.nx + 4] == 0.0 and np.all(gb[a.nx:][k > 0] != 0.0)
    # the scattering handle: same layout, five more slots per level in its workspace and one more double per thread in LDS
    c, d = _opt(ctx, dict(model, rayleigh_molar_scattering=k_dev), scenes, cfg, "scattering", active=False), _opt(ctx, model, scenes, cfg, "scattering")
    assert d.nx == c.nx + ng and np.array_equal(d.initial_state(), xb)
    pc, pd = c.forward_plan(), d.forward_plan()
    assert pd["kernel"] == "rayleigh" and pd["threads"] == pc["threads"] and pd["lds_bytes"] == (pc["lds_bytes"] + 7) // 8 * 8 + 8 * pd["threads"]
    # (two instances of one kernel template: the same arithmetic, not necessarily the same contraction into FMAs)
    (Jc, gc), (Jd, gd) = c.cost_grad(xa), d.cost_grad(xb)
    assert Jc == pytest.approx(Jd, rel=1e-12) and np.allclose(gc, gd[:c.nx], rtol=1e-9, atol=1e-12 * np.abs(gc).max())
    for o in (a, b, c, d):
        o.close()


# ---- 2. shapes ----
@pytest.mark.parametrize("handle,threads", [("plain", None), ("scattering", None), ("scattering", 192)])
@pytest.mark.parametrize("nband", [1, 3])
@pytest.mark.parametrize("ng", [5, 64, 70])
@pytest.mark.parametrize("nlay", [1, 2, 17])
def test_shapes(ctx, oracle, nlay, ng, nband, handle, threads, monkeypatch):
    if threads:
        monkeypatch.setenv("ECCKD_K8A_THREADS", str(threads))
    model, scenes, cfg, orc, _ = _problem(oracle, handle, seed=3, ng=ng, nband=nband, nlay=nlay, nscene=1, ncol=2, ray_sigma=2.0)
    opt = _opt(ctx, model, scenes, cfg, handle, ray_sigma=2.0)
    plan = opt.rayleigh_plan()
    nrows = 8 if handle == "scattering" else 8 * nlay
    assert plan["active"] and plan["nrows"] == nrows and plan["npart"] == -(-nrows // plan["chunk_rows"])
    x, free, rs = _state(opt, orc, 1)          # (a seed that keeps every shape off the branch edges)
    _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs, handle)
    opt.close()


@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_rows_at_the_first_level_chunk(ctx, oracle, handle, offset):
    """Row counts of the reduction one below, at and one above its first-level chunk (the cells of a plain handle, the columns
    of a scattering one); the constant comes from the library."""
    from ecckd_amd import api
    model, scenes, cfg, orc, _ = _problem(oracle, handle, seed=3, ng=5, nband=1, nlay=1, nscene=1, ncol=2)
    probe = _opt(ctx, model, scenes, cfg, handle)
    chunk = probe.rayleigh_plan()["chunk_rows"]
    probe.close()
    assert chunk > 4
    # columns = profiles x solar zenith angles; one layer, so rows = columns for either handle
    nrows = chunk + offset
    mu0 = tuple(np.linspace(1.0, 0.15, nrows)) if nrows % 2 else tuple(np.linspace(1.0, 0.15, nrows // 2))
    ncol = 1 if nrows % 2 else 2
    model, scenes, cfg, orc, _ = _problem(oracle, handle, seed=3, ng=5, nband=1, nlay=1, nscene=1, ncol=ncol, mu0=mu0, ray_sigma=1.5)
    opt = _opt(ctx, model, scenes, cfg, handle, ray_sigma=1.5)
    plan = opt.rayleigh_plan()
    assert plan["nrows"] == nrows and plan["npart"] == (1 if offset <= 0 else 2)
    x, free, rs = _state(opt, orc, 6)
    _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs, handle)
    opt.close()


# ---- 3. branches ----
VARIANTS = ["base", "spectral_only", "mixed_albedo", "albedo_zero", "boundary", "negative_od", "resonance", "one_g_without_rayleigh"]


def _variant_kw(variant):
    return {"base": {}, "spectral_only": dict(broadband_weight=0.0), "mixed_albedo": dict(albedo=(0.2, 0.0, 0.1)),
            "albedo_zero": dict(albedo=(0.0, 0.0, 0.0)), "boundary": dict(boundary=True), "negative_od": dict(ch4_low=True),
            "resonance": dict(rayleigh=lambda r: 1.0e-3 * r, absorb=30.0, mu0=(0.5, 0.5, 1.0, 0.25)),
            "one_g_without_rayleigh": dict(rayleigh=lambda r: np.where(np.arange(r.size) == 4, 0.0, r))}[variant]


@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_cost_and_gradient(ctx, oracle, variant, handle):
    model, scenes, cfg, orc, _ = _problem(oracle, handle, seed=3, ray_sigma=3.0, **_variant_kw(variant))
    opt = _opt(ctx, model, scenes, cfg, handle, ray_sigma=3.0)
    x, free, rs = _state(opt, orc, 1, negative_od=variant == "negative_od")
    nx, ng = x.size, orc.ng
    if variant == "negative_od":
        od = np.concatenate([ckd_synth.Oracle.optical_depth(orc, x, s).ravel() for s in scenes])
        if handle == "plain":                                    # Rayleigh is added BEFORE the clamp there
            od = np.concatenate([orc.optical_depth(x, s).ravel() for s in scenes])
        assert (od < 0).sum() > 10 and (od >= 0).sum() > 10      # clamped cells next to unclamped ones
    if variant == "resonance" and handle == "scattering":
        terms = [orc.layer_terms(x, s) for s in scenes]
        inside = sum(int((t["scat"] & (np.abs(1.0 - t["km"]) < rayleigh_ref.RESONANCE_H)).sum()) for t in terms)
        assert inside >= 10, inside
    # In a cell whose gases were clamped w is exactly 1: where the rounding guard on Tdd is active in about a tenth of the
    # cells (test_cells_at_an_active_clamp of tests/test_optimize_rayleigh_gpu.py), which cells it catches being a matter of the
    # last bit.  The branch-edge assertion is therefore made on the other cells of the scattering handle's negative_od variant
    # (it is NOT waived for them); the difference bounds are asserted in full, tail included.
    J, g = _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs, handle,
                                    but_conservative=variant == "negative_od" and handle == "scattering")
    if variant == "one_g_without_rayleigh":
        # that g point's tail element is pinned: gradient exactly 0, and it stays at MIN_X through minimize
        assert x[nx - ng + 4] == MIN_X and not free[nx - ng + 4] and g[nx - ng + 4] == 0.0 and np.all(g[nx - ng:][free[nx - ng:]] != 0.0)
        res = opt.minimize(max_iterations=5, convergence_criterion=0.0, bounded=True)
        assert res["x"][nx - ng + 4] == MIN_X and opt.rayleigh_coefficients(res["x"])[4] == 0.0
        assert np.any(res["x"][nx - ng:] != opt.initial_state()[nx - ng:])
    opt.close()


@pytest.mark.parametrize("handle", HANDLES)
def test_relative_to_fluxes(ctx, oracle, handle):
    """relative-to fluxes come from a handle made WITHOUT the flag, as the tool makes it"""
    Ref = _ref(handle)
    model, scenes, cfg, orc, _ = _problem(oracle, handle, seed=9, boundary=True)
    base, pert = scenes[0], scenes[1]
    pert = dict(pert, pressure_hl=base["pressure_hl"], temperature_hl=base["temperature_hl"])   # same profiles, other gases
    ref_opt = _opt(ctx, model, [dict(base)], cfg, handle, active=False)
    _, fl = ref_opt.forward(ref_opt.initial_state(), unclamped=handle == "plain")
    ref_opt.close()
    truth = Ref(oracle, model, [pert], cfg)
    nband = model["nband"]
    xt = truth.x0 + 0.1
    f_p, f_b = truth.fluxes(xt, pert), truth.fluxes(xt, base)
    bf = _band_fluxes(model, f_p, nband) - _band_fluxes(model, f_b, nband)
    train = dict(pert, flux_dn=np.ascontiguousarray(bf[:, 0]), flux_up=np.ascontiguousarray(bf[:, 1]),
                 relative_flux_dn=np.ascontiguousarray(fl[:, 0]), relative_flux_up=np.ascontiguousarray(fl[:, 1]),
                 spectral_flux_dn_surf=np.ascontiguousarray(f_p[:, 0, -1] - f_b[:, 0, -1]))
    o2 = Ref(oracle, model, [train], cfg, ray_sigma=2.0)
    opt = _opt(ctx, model, [train], cfg, handle, ray_sigma=2.0)
    x, free, rs = _state(opt, o2, 2)
    J, g = _check_cost_and_gradient(opt, o2, cfg, [train], x, free, rs, handle)
    plain = dict(train, relative_flux_dn=None, relative_flux_up=None)
    assert abs(Ref(oracle, model, [plain], cfg).cost_rt(x) - o2.cost_rt(x)) > 1e-6 * abs(J)
    opt.close()


# ---- 4. many rows ----
def _columns(scene, sl):
    out = dict(scene)
    for k in ("pressure_hl", "temperature_hl", "vmr_fl", "mu0", "flux_dn", "flux_up"):
        out[k] = np.ascontiguousarray(scene[k][sl])
    return out


@pytest.mark.parametrize("handle,nlay,K", [("plain", 9, 256), ("scattering", 2, 4096), ("scattering", 2, 256)])
def test_many_rows(ctx, oracle, handle, nlay, K):
    """One small scene's four columns repeated K times, so that every finishing wave of the reduction takes more than one round
    of its loads (9 216 cells of the plain handle, 16 384 columns of the scattering one: its rows are columns; the third case,
    1 024 columns, has one partial per finishing wave).  At the first guess (the prior and its gradient are exactly 0 there) the
    tail gradient and the cost are K times the small scene's, element by element, to the rounding of the longer sum; the terms
    are the small scene's per-column contributions (each from a handle of that one column).  K is a power of two: K times a
    value is exact.  No finite differences at this size.
    Tail gradient: the reduction adds in double-double, its result is rounded once: K eps sum |terms|, one unit in the last
    place of a sum of terms of one sign.
    Cost: it is summed by k_opt_sum_cost, the kernel every handle has always used, in plain double: thread t adds the columns
    t, t + 256, ... in turn, n = ceil(columns / 256) of them, six shuffle steps add the lanes of a wave and three additions the
    four waves.  A column's value passes through at most D = n + 9 additions of relative error eps / 2 each, so the sum is off
    by at most D (eps / 2) sum |J_column| to first order, and K times the small scene's sum (D = 1 + 9 there) by no more:
    |J_K - K J_1| <= (n + 9) eps K sum |J_c|.  That bound is asserted in every case.  Where a thread adds at most four equal
    columns the sum is exact (2 x and 4 x a value are, and 3 x rounded plus the value rounds to 4 x), so there - up to 1 024
    columns - the one-unit bound K eps sum |J_c| is asserted as well."""
    model, scenes, cfg, orc, _ = _problem(oracle, handle, seed=3, ng=5, nband=1, nlay=nlay, nscene=1, ncol=1)
    small = scenes[0]
    ncol = small["pressure_hl"].shape[0]
    opt = _opt(ctx, model, [small], cfg, handle)
    x = opt.initial_state()
    J1, g1 = opt.cost_grad(x)
    opt.close()
    per_col = []
    for c in range(ncol):
        o = _opt(ctx, model, [_columns(small, slice(c, c + 1))], cfg, handle)
        per_col.append(o.cost_grad(x))
        o.close()
    big = dict(small)
    for k in ("pressure_hl", "temperature_hl", "vmr_fl", "mu0", "flux_dn", "flux_up"):
        big[k] = np.ascontiguousarray(np.concatenate([small[k]] * K, axis=0))
    opt = _opt(ctx, model, [big], cfg, handle)
    plan = opt.rayleigh_plan()
    assert plan["nrows"] == K * (ncol * nlay if handle == "plain" else ncol)
    if K * ncol > 1024:
        assert plan["npart"] > plan["finish_waves"] * plan["batch"]               # more than one round per finishing wave
    else:
        assert plan["npart"] >= plan["finish_waves"]
    JK, gK = opt.cost_grad(x)
    JK2, gK2 = opt.cost_grad(x)
    assert JK == JK2 and np.array_equal(gK, gK2)
    opt.close()
    eps = np.finfo(np.float64).eps
    ng = model["ng"]
    tol_g = K * eps * np.sum([np.abs(g[-ng:]) for _, g in per_col], axis=0)
    tol_J = K * eps * np.sum([abs(J) for J, _ in per_col])
    print(f"tail: {gK[-ng:]} against K x {g1[-ng:]}: difference {np.abs(gK[-ng:] - K * g1[-ng:])} bound {tol_g}")
    print(f"cost: {JK:.17g} against K x {J1:.17g}: difference {abs(JK - K * J1):.3g} bound {tol_J:.3g}")
    assert np.all(g1[-ng:] != 0.0)
    assert np.all(np.abs(gK[-ng:] - K * g1[-ng:]) <= tol_g)
    nthread = -(-K * ncol // 256)                                                 # columns per thread of k_opt_sum_cost
    tol_sum = (nthread + 9) * tol_J
    print(f"cost: {nthread} columns per thread, bound of the kernel's summation order {tol_sum:.3g}")
    assert abs(JK - K * J1) <= tol_sum
    if nthread <= 4:
        assert abs(JK - K * J1) <= tol_J


# ---- 5. Rayleigh alone ----
@pytest.mark.parametrize("handle", HANDLES)
def test_rayleigh_alone(ctx, oracle, handle):
    """All gases inactive: the state is the ng Rayleigh elements; the truth is the same model with k_ray exp(0.3 N(0, 1))"""
    model, scenes, cfg, orc, truth = _problem(oracle, handle, seed=7, gases_active=False, truth_ray=0.3, ray_sigma=0.0)
    opt = _opt(ctx, model, scenes, cfg, handle)
    ng = model["ng"]
    assert opt.nx == ng
    x, free, rs = _state(opt, orc, 4)
    _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs, handle)
    x0 = opt.initial_state()
    J0, g0 = opt.cost_grad(x0)
    res = opt.minimize(max_iterations=150, convergence_criterion=1e-3 * np.linalg.norm(g0), bounded=True)
    assert res["status"] in (0, 2)
    assert res["cost"] < 0.5 * J0
    assert _cost(orc, cfg, res["x"]) == pytest.approx(res["cost"], rel=1e-9)
    lnk_truth = np.log(truth["rayleigh_molar_scattering"])
    before, after = np.mean(np.abs(x0 - lnk_truth)), np.mean(np.abs(res["x"] - lnk_truth))
    print(f"cost {J0:.6g} -> {res['cost']:.6g} in {res['iterations']} iterations; mean |ln k - ln k_truth| {before:.4g} -> {after:.4g}")
    assert after < before
    assert np.allclose(opt.rayleigh_coefficients(res["x"]), np.exp(res["x"]), rtol=1e-15, atol=0.0)
    opt.close()


# ---- 6. prior ----
@pytest.mark.parametrize("handle", HANDLES)
def test_prior(ctx, oracle, handle):
    model, scenes, cfg, orc, _ = _problem(oracle, handle, seed=2, nscene=1, ray_sigma=0.5)
    opt = _opt(ctx, model, scenes, cfg, handle, ray_sigma=0.5)
    x, free, rs = _state(opt, orc, 8)
    ng = orc.ng
    x[-ng:] += 0.3 * rs.normal(size=ng)                           # a perturbed tail
    J, g = _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs, handle)
    share = 0.5 * np.sum((x[-ng:] - orc.x0[-ng:]) ** 2) / 0.25
    assert share > 1e-6 * J
    # sigma <= 0: no prior term on these elements
    for sigma in (0.0, -1.0):
        opt.set_rayleigh_prior(sigma)
        orc.ray_sigma = sigma
        J0, g0 = _check_cost_and_gradient(opt, orc, cfg, scenes, x, free, rs, handle, ncoord=2)
        assert J - J0 == pytest.approx(share, rel=1e-9)
        assert np.allclose(g[-ng:] - g0[-ng:], (x[-ng:] - orc.x0[-ng:]) / 0.25, rtol=1e-9, atol=1e-12 * np.abs(g[-ng:]).max())
        assert np.array_equal(g[:-ng], g0[:-ng])
    opt.close()


# ---- 7. reproducibility ----
@pytest.mark.parametrize("handle", HANDLES)
def test_reproducible(ctx, oracle, handle):
    model, scenes, cfg, orc, _ = _problem(oracle, handle, seed=5, ng=70, ray_sigma=1.0)
    a, b = _opt(ctx, model, scenes, cfg, handle, ray_sigma=1.0), _opt(ctx, model, scenes, cfg, handle, ray_sigma=1.0)
    x, _, _ = _state(a, orc, 3)
    (J1, g1), (J2, g2), (J3, g3) = a.cost_grad(x), a.cost_grad(x), b.cost_grad(x)
    assert J1 == J2 == J3 and np.array_equal(g1, g2) and np.array_equal(g1, g3)
    a.close(); b.close()


# ---- 8. refusals ----
@pytest.mark.parametrize("case", ["longwave_model", "no_rayleigh_coefficient", "prior_without_flag", "no_active_gas_without_flag"])
def test_refusals(ctx, oracle, case):
    from ecckd_amd import EcckdError
    model, scenes, cfg, orc, _ = _problem(oracle, "plain", seed=1)
    with pytest.raises(EcckdError) as e:
        if case == "longwave_model":
            lw = ckd_synth.make_model(seed=1)
            sc = ckd_synth.make_scenes(lw)
            t = ckd_synth.Oracle(oracle, lw, sc, cfg)
            for s in sc:
                bf = t.band_fluxes(t.x0, s)
                s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
            _opt(ctx, lw, sc, cfg, "plain")
        if case == "no_rayleigh_coefficient":
            _opt(ctx, dict(model, rayleigh_molar_scattering=None), scenes, cfg, "plain")
        if case == "prior_without_flag":
            o = _opt(ctx, model, scenes, cfg, "plain", active=False)
            try:
                o.set_rayleigh_prior(1.0)
            finally:
                o.close()
        if case == "no_active_gas_without_flag":
            m = dict(model, gases=[dict(g, active=False) for g in model["gases"]])
            _opt(ctx, m, scenes, cfg, "plain", active=False)
    assert e.value.code == 147                                             # ECCKD_PARAMETER_ERROR
    # the context is as usable as before
    opt = _opt(ctx, model, scenes, cfg, "plain")
    assert np.isfinite(opt.cost_grad(opt.initial_state(), False))
    opt.close()
