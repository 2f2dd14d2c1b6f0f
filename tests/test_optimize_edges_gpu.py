"""The optimiser kernels of csrc/optimize.hip at every dispatch, batch, run and block edge.

tests/test_optimize_gpu.py runs them at one shape (ng = 12, nlay = 18, five gases); here the shapes are chosen one edge at a
time (tests/opt_shapes.py) and every case first ASSERTS the kernel it got (Optimizer.forward_plan): a shape that drifts to
another instance of k_opt_forward_adjoint_cells<NC, SW, NB> fails instead of passing for the wrong reason.  References: the
CPU oracle's optical depths and fluxes, cost_rt + cost_prior, its reverse-mode gradient plus the dense-inverse prior - with the
comparisons and tolerances of test_more_than_64_g_points / test_forward_optical_depth_and_fluxes - and, where the cell-parallel
kernel runs, the general kernel with the tolerances of test_cell_parallel_kernel_matches_the_general_one."""
import numpy as np
import pytest

import ckd_synth
import lbfgs_ref
import opt_shapes

pytestmark = pytest.mark.gpu


def _opt(ctx, model, scenes, cfg):
    from ecckd_amd import api
    return api.Optimizer(ctx, model, scenes, **cfg)


def _assert_plan(opt, want):
    plan = opt.forward_plan()
    got = {k: plan[k] for k in want}
    assert got == want, (got, want, plan)
    return plan


def _run(opt, x):
    J, g = opt.cost_grad(x)
    od, fl = opt.forward(x)
    return J, g, od, fl


def _check(ctx, oracle, monkeypatch, prob, want_plan, sw=False, negative=False, seed=3, prior=True):
    """The plan, then forward, cost and gradient at a perturbed state against the oracle, then (where the cell-parallel kernel
    ran) against the general kernel.  -> (opt, x, J, g) with the handle still open.

    (The flux bound of 1e-10 leans on exp rounding alike on both sides.  The thick-layer weight of radiative_transfer_lw,
    fac = 1 - eps / (D tau) for eps > 1e-5, turns a last-bit difference of exp(-D tau) into 1e-16 / eps of fac, and a top layer
    emits B0 eps + (B1 - B0) fac: with the 2 x 2 table of inside_problem, ng = 65 and 5 x 13 cells one cell of eps = 9e-5 gave a
    flux 2.2e-9 off the oracle - from BOTH kernels, which agreed to 8e-16.  No shape of this file is there.)"""
    model, scenes, cfg, orc = prob
    if not prior:
        cfg = dict(cfg, prior_error=1.0e30)
    monkeypatch.delenv("ECCKD_K8A_GENERIC", raising=False)
    opt = _opt(ctx, model, scenes, cfg)
    plan = _assert_plan(opt, want_plan)
    assert np.allclose(opt.initial_state(), orc.x0, rtol=1e-15, atol=0)
    x, free = opt_shapes.perturbed_state(orc, model, seed, negative)
    od_ref = np.concatenate([orc.optical_depth(x, s) for s in scenes])
    fl_ref = np.concatenate([orc.fluxes(x, s) for s in scenes])
    if negative:
        assert (od_ref < 0).sum() > 10 and (od_ref > 0).sum() > 10
    J, g, od, fl = _run(opt, x)
    assert np.allclose(od, np.maximum(od_ref, 0.0), rtol=1e-12, atol=1e-300)
    assert np.allclose(fl, fl_ref, rtol=1e-10, atol=1e-300)
    J_rt, g_rt = orc.cost_grad_rt(x)
    J_b, g_b = orc.cost_prior(x, cfg["prior_error"]) if prior else (0.0, 0.0)
    assert J == pytest.approx(J_rt + J_b, rel=1e-10)
    g_ref = np.where(free, g_rt + g_b, 0.0)
    assert np.allclose(g, g_ref, rtol=1e-8, atol=1e-11 * np.abs(g_ref).max())
    assert np.all(g[~free] == 0.0)
    if prior:                           # (prior_error = 1e30 still adds its ~1e-58 where the radiative-transfer part is 0)
        assert np.array_equal(g == 0.0, g_ref == 0.0)
    if plan["cells"]:
        monkeypatch.setenv("ECCKD_K8A_GENERIC", "1")
        _assert_plan(opt, dict(cells=False, nc_template=0, nb=0))
        J2, g2, od2, fl2 = _run(opt, x)
        monkeypatch.delenv("ECCKD_K8A_GENERIC")
        if negative:
            assert (od2 == 0).sum() > 10
        assert np.allclose(od2, od, rtol=1e-13, atol=1e-300) and np.allclose(fl2, fl, rtol=1e-13, atol=1e-300)
        assert J == pytest.approx(J2, rel=1e-13)
        assert np.allclose(g2, g, rtol=1e-9, atol=1e-12 * np.abs(g2).max())
        assert np.array_equal(g2 == 0.0, g == 0.0)
    return opt, x, J, g


# ---- (a) cells per thread and layer groups ------------------------------------------------------------------------------
# threads: 1024 longwave, 512 shortwave; lgroups = threads // ngpad; nc = ceil(nlay / lgroups); <4> up to 4 cells, <8> up to 8,
# beyond that the general kernel.  The five gases of ckd_synth: 24 entries longwave (nb 3), 25 shortwave (nb 4).

NC_CASES = [
    # ng = 70 (ngpad 128): 8 layer groups longwave, 4 shortwave
    (False, 70, 32, dict(cells=True, nc_template=4, nb=3, threads=1024, ngpad=128, lgroups=8)),     # nc = 4: <4> at its limit
    (False, 70, 33, dict(cells=True, nc_template=8, nb=3, threads=1024, ngpad=128, lgroups=8)),     # nc = 5
    (False, 70, 64, dict(cells=True, nc_template=8, nb=3, threads=1024, ngpad=128, lgroups=8)),     # nc = 8: <8> at its limit
    (False, 70, 65, dict(cells=False, nc_template=0, nb=0, threads=1024, ngpad=128, lgroups=8)),    # nc = 9: the general kernel
    (True, 70, 32, dict(cells=True, nc_template=8, nb=4, threads=512, ngpad=128, lgroups=4)),       # nc = 8
    (True, 70, 33, dict(cells=False, nc_template=0, nb=0, threads=1024, ngpad=128, lgroups=8)),     # nc = 9
    (True, 70, 64, dict(cells=False, nc_template=0, nb=0, threads=1024, ngpad=128, lgroups=8)),     # nc = 16
    (True, 70, 16, dict(cells=True, nc_template=4, nb=4, threads=512, ngpad=128, lgroups=4)),       # nc = 4: shortwave <4> limit
    (True, 70, 17, dict(cells=True, nc_template=8, nb=4, threads=512, ngpad=128, lgroups=4)),       # nc = 5
]


@pytest.mark.parametrize("sw,ng,nlay,plan", NC_CASES, ids=[f"{'sw' if c[0] else 'lw'}-ng{c[1]}-nlay{c[2]}" for c in NC_CASES])
def test_cells_per_thread_and_layer_groups(ctx, oracle, monkeypatch, sw, ng, nlay, plan):
    prob = opt_shapes.problem(oracle, ng=ng, nband=5, nlay=nlay, ncol=2, sw=sw, negative=True, seed=6)
    _check(ctx, oracle, monkeypatch, prob, plan, sw=sw, negative=True)[0].close()


# the chunks of K8A_CH = 8 layers of the sequential recurrences (one wave): no chunk, a chunk less one, one chunk, one and a
# tail, two chunks, two and a tail; nlay = 1 is a single cell, at nlay = 17 longwave 15 of the 16 layer groups hold one cell
CHUNK_NLAY = [1, 7, 8, 9, 16, 17]


@pytest.mark.parametrize("sw", [False, True], ids=["lw", "sw"])
@pytest.mark.parametrize("nlay", CHUNK_NLAY)
def test_recurrence_chunk_edges(ctx, oracle, monkeypatch, nlay, sw):
    lgroups = 8 if sw else 16
    nc = -(-nlay // lgroups)
    assert nc == {(False, 17): 2, (True, 9): 2, (True, 16): 2, (True, 17): 3}.get((sw, nlay), 1)
    plan = dict(cells=True, nc_template=4, nb=4 if sw else 3, threads=512 if sw else 1024, ngpad=64, lgroups=lgroups)
    prob = opt_shapes.problem(oracle, ng=12, nlay=nlay, ncol=3, sw=sw, seed=nlay)
    _check(ctx, oracle, monkeypatch, prob, plan, sw=sw)[0].close()


# ng at the 64-wide padding: threads = ngpad * lgroups, 960 longwave / 384 shortwave at ng = 129; nlay = 9
NGPAD_CASES = [
    (False, 64, dict(cells=True, nc_template=4, nb=3, threads=1024, ngpad=64, lgroups=16)),
    (False, 65, dict(cells=True, nc_template=4, nb=3, threads=1024, ngpad=128, lgroups=8)),
    (False, 128, dict(cells=True, nc_template=4, nb=3, threads=1024, ngpad=128, lgroups=8)),
    (False, 129, dict(cells=True, nc_template=4, nb=3, threads=960, ngpad=192, lgroups=5)),
    (True, 64, dict(cells=True, nc_template=4, nb=4, threads=512, ngpad=64, lgroups=8)),
    (True, 65, dict(cells=True, nc_template=4, nb=4, threads=512, ngpad=128, lgroups=4)),
    (True, 128, dict(cells=True, nc_template=4, nb=4, threads=512, ngpad=128, lgroups=4)),
    (True, 129, dict(cells=True, nc_template=8, nb=4, threads=384, ngpad=192, lgroups=2)),          # nc = 5
]


@pytest.mark.parametrize("sw,ng,plan", NGPAD_CASES, ids=[f"{'sw' if c[0] else 'lw'}-ng{c[1]}" for c in NGPAD_CASES])
def test_g_point_padding_edges(ctx, oracle, monkeypatch, sw, ng, plan):
    prob = opt_shapes.problem(oracle, ng=ng, nband=5, nlay=9, ncol=2, sw=sw, seed=ng)
    _check(ctx, oracle, monkeypatch, prob, plan, sw=sw)[0].close()


@pytest.mark.parametrize("sw", [False, True], ids=["lw", "sw"])
def test_threads_knob_is_read_at_every_call(ctx, oracle, monkeypatch, sw):
    """ECCKD_K8A_THREADS = 192 set in the middle of the process: 3 layer groups, 6 of the 18 layers per thread, <8, ., .>; and
    back to the default block when it is unset again."""
    prob = opt_shapes.problem(oracle, ng=12, nlay=18, ncol=2, sw=sw, negative=True, seed=4)
    monkeypatch.setenv("ECCKD_K8A_THREADS", "192")
    opt, x, J, g = _check(ctx, oracle, monkeypatch, prob, dict(cells=True, nc_template=8, nb=4 if sw else 3, threads=192, ngpad=64, lgroups=3),
                          sw=sw, negative=True)
    monkeypatch.delenv("ECCKD_K8A_THREADS")
    _assert_plan(opt, dict(cells=True, nc_template=4, threads=512 if sw else 1024, lgroups=8 if sw else 16))
    J2, g2 = opt.cost_grad(x)
    assert J2 == pytest.approx(J, rel=1e-13) and np.allclose(g2, g, rtol=1e-9, atol=1e-12 * np.abs(g).max())
    for bad in ("63", "1025", "junk"):                          # outside 64 ... 1024: ignored
        monkeypatch.setenv("ECCKD_K8A_THREADS", bad)
        _assert_plan(opt, dict(cells=True, threads=512 if sw else 1024))
    opt.close()


# ---- (b) the 8-entry batches of a cell's table and the rounds of 64 entries -------------------------------------------------
# nb = ceil(min(nent, 64) / 8): 1 ... 4 in straight-line code, above 32 entries the loop with two batches in flight (nb = 0) -
# 5, 6 and 8 batches at 36, 48 and 64 entries; beyond 64 entries a second round (of one entry: 65 shortwave, the Rayleigh entry
# alone; of one batch: 68, 72; a full one: 128) and a third (129, 132).

def _nb(nent):
    return {1: 1, 2: 2, 3: 3, 4: 4}.get(-(-min(nent, 64) // 8), 0)


NB_CASES = ([(False, n, n in (36, 68)) for n in (4, 8, 12, 16, 20, 32, 36, 40, 48, 64, 68, 72, 128, 132)] +
            [(True, n, n == 65) for n in (5, 9, 17, 25, 33, 65, 129)])
NB_WANT = {4: 1, 5: 1, 8: 1, 9: 2, 12: 2, 16: 2, 17: 3, 20: 3, 25: 4, 32: 4, 33: 0, 36: 0, 40: 0, 48: 0, 64: 0, 65: 0, 68: 0,
           72: 0, 128: 0, 129: 0, 132: 0}


@pytest.mark.parametrize("sw,nent,negative", NB_CASES, ids=[f"{'sw' if c[0] else 'lw'}-nent{c[1]}" for c in NB_CASES])
def test_entry_batches_and_rounds(ctx, oracle, monkeypatch, sw, nent, negative):
    gases = opt_shapes.gas_list(nent, sw=sw, relative=negative)
    assert opt_shapes.nent_of(gases, sw) == nent and _nb(nent) == NB_WANT[nent]
    plan = dict(cells=True, nc_template=4, nb=NB_WANT[nent], threads=512 if sw else 1024, ngpad=64, lgroups=8 if sw else 16)
    prob = opt_shapes.problem(oracle, gases=gases, ng=12, nlay=6, ncol=2, sw=sw, negative=negative, seed=nent)
    _check(ctx, oracle, monkeypatch, prob, plan, sw=sw, negative=negative)[0].close()


# the same batch counts in the <8, ., .> instances: more than 4 cells per thread (longwave 72 layers on 16 groups, shortwave 40
# on 8: nc = 5)
NB8_CASES = [(False, n) for n in (4, 12, 20, 32, 36)] + [(True, n) for n in (5, 9, 17, 25, 33)]


@pytest.mark.parametrize("sw,nent", NB8_CASES, ids=[f"{'sw' if c[0] else 'lw'}-nent{c[1]}" for c in NB8_CASES])
def test_entry_batches_with_eight_cells_per_thread(ctx, oracle, monkeypatch, sw, nent):
    gases = opt_shapes.gas_list(nent, sw=sw)
    plan = dict(cells=True, nc_template=8, nb=NB_WANT[nent], threads=512 if sw else 1024, ngpad=64, lgroups=8 if sw else 16)
    prob = opt_shapes.problem(oracle, gases=gases, ng=12, nlay=40 if sw else 72, ncol=2, sw=sw, seed=nent)
    _check(ctx, oracle, monkeypatch, prob, plan, sw=sw)[0].close()


@pytest.mark.parametrize("nent", [33, 65])
def test_run_ckd_shortwave_entry_rounds(ctx, oracle, nent):
    """ecckd_run_ckd hands the Rayleigh entry (the last one: 32, the end of the loop's first four batches; 64, alone in a second
    round) to the same kernel, which adds it AFTER the clamp: gas optical depth, Rayleigh optical depth and the direct beam."""
    from ecckd_amd import api
    gases = opt_shapes.gas_list(nent, sw=True)
    model, scenes, cfg, orc = opt_shapes.problem(oracle, gases=gases, ng=12, nlay=6, ncol=2, sw=True, seed=nent)
    sc = scenes[0]
    out = api.run_ckd(ctx, model, sc, per_gas=False)
    od_gas = np.maximum(ckd_synth.Oracle.optical_depth(orc, orc.x0, sc), 0.0)
    ray = orc.optical_depth(orc.x0, sc) - ckd_synth.Oracle.optical_depth(orc, orc.x0, sc)
    assert np.allclose(out["optical_depth"], od_gas, rtol=1e-12, atol=1e-300)
    p = sc["pressure_hl"]
    ray_ref = ((p[:, 1:] - p[:, :-1]) / (9.80665 * 0.001 * 28.970))[:, :, None] * model["rayleigh_molar_scattering"][None, None, :]
    assert np.allclose(ray, ray_ref, rtol=1e-12, atol=0) and np.allclose(out["rayleigh_optical_depth"], ray_ref, rtol=1e-12, atol=1e-300)
    direct = np.stack([oracle.radiative_transfer_direct_sw(sc["mu0"][c], orc.ssi(sc), od_gas[c] + ray_ref[c]) for c in range(p.shape[0])])
    assert np.allclose(out["spectral_flux_dn_direct_sw"], direct, rtol=1e-10, atol=1e-300)


# ---- (c) more than one (half level, band) slot per thread in the cost phase -------------------------------------------------

def test_more_level_band_slots_than_threads(ctx, oracle, monkeypatch):
    """shortwave, 8 bands, 64 layers: 65 * 8 = 520 slots on 512 threads (K8A_MAXR rounds), 8 cells per thread"""
    prob = opt_shapes.problem(oracle, ng=12, nband=8, nlay=64, ncol=2, sw=True, negative=True, seed=8)
    plan = dict(cells=True, nc_template=8, nb=4, threads=512, ngpad=64, lgroups=8)
    _check(ctx, oracle, monkeypatch, prob, plan, sw=True, negative=True)[0].close()


@pytest.mark.parametrize("sw", [False, True], ids=["lw", "sw"])
def test_second_round_of_the_staged_seed_store(ctx, oracle, monkeypatch, sw):
    """ECCKD_K8A_THREADS = 64, 9 bands, 8 layers: 9 * 9 = 81 (half level, band) slots on one wave - 17 threads hold a second
    slot in registers across the barrier before the seeds overwrite the band fluxes; one layer group, 8 cells per thread"""
    monkeypatch.setenv("ECCKD_K8A_THREADS", "64")
    prob = opt_shapes.problem(oracle, ng=12, nband=9, nlay=8, ncol=2, sw=sw, negative=True, seed=5)
    plan = dict(cells=True, nc_template=8, nb=4 if sw else 3, threads=64, ngpad=64, lgroups=1)
    _check(ctx, oracle, monkeypatch, prob, plan, sw=sw, negative=True)[0].close()


# ---- (d) a profile too large for either kernel ------------------------------------------------------------------------------

def test_profile_too_large_is_refused_and_the_context_lives_on(ctx, oracle, monkeypatch):
    from ecckd_amd import EcckdError
    monkeypatch.delenv("ECCKD_K8A_GENERIC", raising=False)
    model = opt_shapes.make_model(ng=128, nband=3)
    scenes = opt_shapes.make_scenes(model, nlay=64, ncol=1)
    for s in scenes:
        s["flux_dn"] = np.zeros((1, 65, 3))
        s["flux_up"] = np.zeros((1, 65, 3))
    opt = _opt(ctx, model, scenes, opt_shapes.CFG)
    plan = _assert_plan(opt, dict(cells=False, nc_template=0, nb=0))
    assert plan["lds_bytes"] > 160 * 1024
    x = opt.initial_state()
    with pytest.raises(EcckdError, match="too large for the per-profile LDS tile"):
        opt.cost_grad(x)
    with pytest.raises(EcckdError, match="too large for the per-profile LDS tile"):
        opt.forward(x)
    opt.close()
    prob = opt_shapes.problem(oracle, ng=12, nlay=6, ncol=2, seed=1)
    _check(ctx, oracle, monkeypatch, prob, dict(cells=True, nc_template=4, nb=3))[0].close()


# ---- (e) run lengths of the gradient's gather ---------------------------------------------------------------------------------
# k_opt_gradient_gather adds runs of at most 64 references, eight at a time, two batches in flight; k_opt_gradient_finish adds a
# node's runs eight at a time.  On a 2 x 2 table with every layer inside it each node has exactly ncol * nlay references.

RUN_SHAPES = {n: (1, n) for n in (1, 7, 8, 9, 16, 17, 56, 57, 63, 64, 65, 128)}
RUN_SHAPES.update({129: (3, 43), 513: (9, 57)})                      # 513: 9 runs, past the 8-at-a-time loop of the finish


@pytest.mark.parametrize("ncell,ng", [(n, 12) for n in sorted(RUN_SHAPES)] + [(65, 65)])
def test_gather_run_lengths(ctx, oracle, monkeypatch, ncell, ng):
    ncol, nlay = RUN_SHAPES[ncell]
    prob = opt_shapes.inside_problem(oracle, ncol, nlay, ng=ng, seed=ncell)
    model, scenes = prob[0], prob[1]
    refs = opt_shapes.references_per_node(model, scenes[0])
    assert refs.shape == (1, 2, 2) and np.all(refs == ncell)
    if ng <= 64:
        plan = dict(cells=True, nc_template=4 if nlay <= 64 else 8, nb=1, ngpad=64, lgroups=16)
    else:                               # two 64-g chunks per node and run; 65 layers on 8 groups: the general forward kernel
        plan = dict(cells=False, nc_template=0, nb=0, ngpad=128, lgroups=8)
    _check(ctx, oracle, monkeypatch, prob, plan, seed=ncell)[0].close()


def test_nodes_without_a_reference(ctx, oracle, monkeypatch):
    """A look-up-table gas whose concentration axis reaches far beyond the profiles: its unreferenced nodes get no gather run
    at all, and their radiative-transfer gradient is exactly 0."""
    prob = opt_shapes.inside_problem(oracle, 3, 43, extra_lut=True, seed=2)
    model, scenes, cfg, orc = prob
    refs = opt_shapes.references_per_node(model, scenes[0], gas=1)
    assert (refs == 0).sum() > 0 and (refs > 0).sum() > 0 and refs.sum() == 8 * 129
    opt, x, J, g = _check(ctx, oracle, monkeypatch, prob, dict(cells=True, nc_template=4, nb=2), prior=False)
    # with the look-up-table gas at its prior state the prior's stencil adds exactly nothing there (it stays inside a gas)
    x2 = np.concatenate([x[:orc.sizes[0]], orc.x0[orc.sizes[0]:]])
    J2, g2 = opt.cost_grad(x2)
    g_ref2 = orc.cost_grad_rt(x2)[1]
    g_lut, g_lut_ref = (a[orc.sizes[0]:].reshape(refs.shape + (-1,)) for a in (g2, g_ref2))
    assert np.all(g_lut[refs == 0] == 0.0) and np.all(g_lut[refs > 0] != 0.0)
    assert np.allclose(g_lut, g_lut_ref, rtol=1e-8, atol=1e-11 * np.abs(g_ref2).max())
    opt.close()


# ---- (f) more node tasks than resident waves: the grid-stride loops of the two gradient kernels ---------------------------

def _big_lut_problem(oracle, **over):
    """one active look-up-table gas of 8 x 8 x 130 nodes at 4 g points: 8 320 node tasks (8 192 waves are resident on 256 CUs)"""
    return opt_shapes.problem(oracle, gases=(("lut", True),), ng=4, nband=2, nt=8, np_=130, nconc=8, nlay=6, ncol=2, seed=13, **over)


def test_gradient_grid_stride_and_task_order(ctx, oracle, monkeypatch):
    prob = _big_lut_problem(oracle)
    assert prob[3].x0.size == 8320 * 4
    opt, x, J, g = _check(ctx, oracle, monkeypatch, prob, dict(cells=True, nc_template=4, nb=1), prior=False)
    opt.close()
    # ECCKD_K8B_PLAIN_ORDER is read when the handle is created.  The order tables choose who computes what, never what is
    # computed: bit for bit the same gradient.
    monkeypatch.setenv("ECCKD_K8B_PLAIN_ORDER", "1")
    opt2 = _opt(ctx, prob[0], prob[1], dict(prob[2], prior_error=1.0e30))
    monkeypatch.delenv("ECCKD_K8B_PLAIN_ORDER")
    J2, g2 = opt2.cost_grad(x)
    assert J2 == J and np.array_equal(g2, g)
    opt2.close()


# ---- (g) the prior's stencil at the edges of its three axes -------------------------------------------------------------------

CORRS = [dict(pressure_corr=0.95, temperature_corr=0.95, conc_corr=0.95),
         dict(pressure_corr=0.8, temperature_corr=0.5, conc_corr=1e-3)]          # drops entries below 1e-6


@pytest.mark.parametrize("dims", [(1, 2, 2), (2, 2, 2), (3, 5, 6)], ids=str)
def test_prior_stencil_edges(ctx, oracle, dims):
    """the comparison of test_prior_matches_dense_inverse on the smallest tables the model constructor takes"""
    nconc, nt, np_ = dims
    gases = (("none", True), ("lut", True)) if nconc > 1 else (("none", True), ("linear", True))
    for corr in CORRS:
        model, scenes, cfg, orc = opt_shapes.problem(oracle, gases=gases, nconc=max(nconc, 2), nt=nt, np_=np_, seed=4, flux_weight=0.0, **corr)
        opt = _opt(ctx, model, scenes, cfg)
        x, free = opt_shapes.perturbed_state(orc, model, 2)
        x = orc.x0 + 1.5 * (x - orc.x0)                                            # 0.3 N(0,1)
        J, g = opt.cost_grad(x)
        opt_rt = _opt(ctx, model, scenes, dict(cfg, prior_error=1.0e30))
        J_rt, g_rt = opt_rt.cost_grad(x)
        Jb_ref, gb_ref = orc.cost_prior(x, cfg["prior_error"])
        assert J - J_rt == pytest.approx(Jb_ref, rel=1e-9)
        gb = g - g_rt
        assert np.allclose(gb[free], gb_ref[free], rtol=1e-8, atol=1e-9 * np.abs(gb_ref).max())
        opt.close(); opt_rt.close()


@pytest.mark.parametrize("dims", [(1, 1, 2), (2, 1, 2), (1, 2, 1)], ids=str)
def test_table_axis_of_one_node_is_refused(ctx, oracle, dims):
    """a temperature or pressure axis of a single node cannot be interpolated: ecckd_opt_create refuses it"""
    from ecckd_amd import EcckdError
    nconc, nt, np_ = dims
    gases = (("none", True), ("lut", True)) if nconc > 1 else (("none", True), ("linear", True))
    model = opt_shapes.make_model(gases, nt=2, np_=2)
    # (ckd_model itself needs two nodes per axis to build its grids: cut the axes afterwards)
    model["temperature"] = np.ascontiguousarray(model["temperature"][:nt, :np_])
    model["log_pressure"] = np.ascontiguousarray(model["log_pressure"][:np_])
    for g in model["gases"]:
        for k in ("molar_abs", "min_molar_abs", "max_molar_abs"):
            g[k] = np.ascontiguousarray(g[k][..., :nt, :np_, :])
    scenes = opt_shapes.make_scenes(opt_shapes.make_model(gases), nlay=2, ncol=1)
    for s in scenes:
        s["flux_dn"] = np.zeros((1, 3, 3))
        s["flux_up"] = np.zeros((1, 3, 3))
    with pytest.raises(EcckdError, match="bad model dimensions"):
        _opt(ctx, model, scenes, opt_shapes.CFG)


# ---- (h) the sum of the cost: thread t takes elements t, t + 256, ... eight at a time ---------------------------------------

@pytest.mark.parametrize("ncol", [1, 255, 256, 257, 2048, 2049])
def test_cost_sum_over_profiles(ctx, oracle, ncol):
    model, scenes, cfg, orc = opt_shapes.problem(oracle, gases=(("none", True),), ng=4, nband=2, nlay=2, ncol=ncol, seed=ncol)
    opt = _opt(ctx, model, scenes, cfg)
    x, free = opt_shapes.perturbed_state(orc, model, 5)
    J = opt.cost_grad(x, False)
    assert J == pytest.approx(orc.cost_rt(x) + orc.cost_prior(x, cfg["prior_error"])[0], rel=1e-10)
    assert opt.cost_grad(x, False) == J
    opt.close()


def _kron_prior(orc, model, cfg, x):
    """The prior's cost of a model with ONE active gas through the Kronecker structure of its covariance (B = Bc x Bt x Bp, so
    B^-1 = Bc^-1 x Bt^-1 x Bp^-1): the dense inverse of Oracle.cost_prior without an n x n matrix.  Equal to it where no entry
    of the dense inverse falls below the 1e-6 it zeroes (checked at a small shape by the caller)."""
    g = model["gases"][orc.active[0]]
    nt, np_ = model["temperature"].shape
    nconc = g["molar_abs"].shape[0] if g["conc"] == "lut" else 1
    inv = lambda n, rho: np.linalg.inv(rho ** np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]))
    dx = (x - orc.x0).reshape(nconc, nt, np_, -1)
    y = np.einsum("ai,bj,ck,ijkg->abcg", inv(nconc, cfg["conc_corr"]) if nconc > 1 else np.ones((1, 1)),
                  inv(nt, cfg["temperature_corr"]), inv(np_, cfg["pressure_corr"]), dx, optimize=True)
    return 0.5 * np.sum(dx * y) / cfg["prior_error"] ** 2


def test_cost_sum_over_nodes(ctx, oracle):
    """8 320 node terms of the prior's cost: more than 8 x 256, so every thread's chain of eight is full and wraps round"""
    small = opt_shapes.problem(oracle, gases=(("lut", True),), nconc=3, nt=5, np_=6, seed=3)
    xs, _ = opt_shapes.perturbed_state(small[3], small[0], 5)
    assert _kron_prior(small[3], small[0], small[2], xs) == pytest.approx(small[3].cost_prior(xs, small[2]["prior_error"])[0], rel=1e-11)
    model, scenes, cfg, orc = _big_lut_problem(oracle)
    opt = _opt(ctx, model, scenes, cfg)
    x, free = opt_shapes.perturbed_state(orc, model, 5)
    J = opt.cost_grad(x, False)
    Jb = _kron_prior(orc, model, cfg, x)
    J_rt = orc.cost_rt(x)
    assert Jb > 1e-3 * J_rt                                       # the node sum is a visible part of J
    assert J == pytest.approx(J_rt + Jb, rel=1e-10)
    assert opt.cost_grad(x, False) == J
    opt.close()


# ---- the minimiser's vector kernels against an independent L-BFGS --------------------------------------------------------

@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
@pytest.mark.parametrize("nx", sorted(opt_shapes.MINIMISER_SHAPES))
def test_minimiser_follows_the_two_loop_reference(ctx, nx, bounded):
    """ecckd_opt_minimize (compact L-BFGS, k_lb_update / k_lb_direction / k_lb_step / k_lb_finish, 1 024 threads per block,
    at most one block per CU) over a numpy cost function, against tests/lbfgs_ref.py (two-loop form) from the same state and
    bounds: (iteration, J, |q|) of every iteration and the final x.  nx = 1 023 / 1 024 / 1 025: a block with a partial last
    wave, a full block, a second block of one element; 327 680: more elements than 1 024 x the CUs of any CDNA part - a second
    grid-stride trip, partial in every block.  12 iterations: the ring of 6 pairs wraps.

    Tolerance: 1 000 x the largest relative spread between three runs of the reference - float64, float64 with every sum in a
    shuffled order, np.longdouble - which tests/test_lbfgs_ref.py measures on the CPU and holds against lbfgs_ref.SPREAD:
    3.0e-15 ... 1.6e-14 measured at nx <= 1 025 and 1.7e-13 at nx = 327 680, recorded (rounded up) as 1e-14 / 1e-14 / 3e-14 and
    3e-13, hence an allowance of 1e-11 ... 3e-10 here.  The device sums in yet another order and with fused multiply-adds: three decades of margin over pure
    reordering, and never more than 1e-9."""
    model, scenes, x0_np, lo_np, hi_np, tight = opt_shapes.minimiser_problem(nx)
    opt = _opt(ctx, model, scenes, opt_shapes.CFG)
    assert opt.nx == nx
    x0, lo, hi = opt.initial_state(bounds=True)
    free = x0 > -1.0e20
    assert np.array_equal(x0, x0_np) or np.allclose(x0, x0_np, rtol=1e-15, atol=0)
    assert np.allclose(lo[free], lo_np[free], rtol=1e-14, atol=1e-14) and np.allclose(hi[free], hi_np[free], rtol=1e-14, atol=1e-14)
    assert (~free).sum() > 0 and np.all((hi - x0)[tight] < 1e-9) and np.all((hi - x0)[tight] > 0)
    make = lbfgs_ref.cosh_problem(x0, seed=nx, tight=tight)
    ref = lbfgs_ref.minimize(make(), x0, lo if bounded else None, hi if bounded else None, max_iterations=12)
    assert ref["status"] == 2 and ref["kept"] >= 7 and ref["first_trial"] >= 1
    if bounded:                                                    # (unbounded no step of this problem overshoots: lbfgs_ref.py)
        assert ref["halvings"] >= 1 and ref["kept"] < 12
    allowance = 1000.0 * lbfgs_ref.SPREAD[nx]
    assert allowance <= 1.0e-9
    hist = []
    opt.set_evaluator(make())
    opt.set_progress(lambda it, cost, gnorm: hist.append((it, cost, gnorm)))
    res = opt.minimize(max_iterations=12, convergence_criterion=0.0, bounded=bounded)
    opt.set_evaluator(None)
    assert res["status"] == 2 and res["iterations"] == 12 and len(hist) == len(ref["history"]) == 13
    for (i1, J1, q1), (i2, J2, q2) in zip(hist, ref["history"]):
        print(nx, bounded, i1, abs(J1 - J2) / abs(J2), abs(q1 - q2) / abs(q2))
        assert i1 == i2 and J1 == pytest.approx(J2, rel=allowance) and q1 == pytest.approx(q2, rel=allowance)
    assert np.array_equal(res["x"][~free], x0[~free])
    err = np.abs(res["x"][free] - ref["x"][free]).max() / np.abs(ref["x"][free]).max()
    print(nx, bounded, "x", err, "allowance", allowance)
    assert err <= allowance
    if bounded:
        assert np.all(res["x"][free] >= lo[free]) and np.all(res["x"][free] <= hi[free])
        assert np.array_equal(res["x"][free] == hi[free], ref["x"][free] == hi[free]) and (res["x"][free] == hi[free]).sum() > 16
    opt.close()
