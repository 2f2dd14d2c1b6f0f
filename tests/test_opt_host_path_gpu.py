"""The optimiser's host side (csrc/optimize.hip below the kernels, csrc/opt_tables.cpp): what ecckd_opt_create refuses and that a
refusal leaves nothing behind, that a diagnostic forward pass leaves the handle's evaluation mode as it found it, and that a
handle gives back the device memory it took.  Truth fluxes are fixed-seed arrays: nothing here needs the oracle."""
import numpy as np
import pytest

import ckd_synth

pytestmark = pytest.mark.gpu

PARAMETER_ERROR = 147
CFG = dict(flux_weight=0.2, flux_profile_weight=0.05, broadband_weight=0.4, spectral_boundary_weight=0.0,
           negative_od_penalty=1.0e4, pressure_weight_power=0.5, prior_error=4.0, pressure_corr=0.95,
           temperature_corr=0.95, conc_corr=0.9, cap_relative_linear=0.0)


def _with_fluxes(model, scenes, seed=3):
    rs = np.random.RandomState(seed)
    for s in scenes:
        ncol, nhl = s["pressure_hl"].shape
        s["flux_dn"] = rs.uniform(50.0, 150.0, (ncol, nhl, model["nband"]))
        s["flux_up"] = rs.uniform(50.0, 150.0, (ncol, nhl, model["nband"]))
    return scenes


def _problem(sw=False, **kw):
    if sw:
        model = ckd_synth.make_model_sw(seed=0)
        return model, _with_fluxes(model, ckd_synth.make_scenes_sw(model, (0.15, 0.3, 0.06), **kw))
    model = ckd_synth.make_model(seed=0)
    return model, _with_fluxes(model, ckd_synth.make_scenes(model, **kw))


def _opt(ctx, model, scenes, **over):
    from ecckd_amd import api
    return api.Optimizer(ctx, model, scenes, **dict(CFG, **over))


def _initial_cost(ctx, model, scenes):
    opt = _opt(ctx, model, scenes)
    J = opt.cost_grad(opt.initial_state(), want_grad=False)
    opt.close()
    return J


def _bad_dimensions(model, scenes):
    model["temperature"] = model["temperature"][:1]


def _no_planck(model, scenes):
    model["temperature_planck"], model["planck_function"] = model["temperature_planck"][:1], model["planck_function"][:1]


def _logarithmic(model, scenes):
    model["logarithmic_interpolation"] = True


def _ill_defined_gas(model, scenes):
    g = model["gases"][1]                                    # a look-up-table gas with one mole fraction
    for k in ("molar_abs", "min_molar_abs", "max_molar_abs"):
        g[k] = g[k][:1]
    g["vmr"] = g["vmr"][:1]


def _nlay(nlay):
    def spoil(model, scenes):
        scenes[:] = _with_fluxes(model, ckd_synth.make_scenes(model, nlay=nlay))
    return spoil


def _inconsistent_scene(model, scenes):
    scenes[1] = _with_fluxes(model, ckd_synth.make_scenes(model, nscene=1, nlay=7))[0]


def _other_nband(model, scenes):
    scenes[1]["flux_dn"] = scenes[1]["flux_dn"][:, :, :2]
    scenes[1]["flux_up"] = scenes[1]["flux_up"][:, :, :2]


def _no_active_gas(model, scenes):
    for g in model["gases"]:
        g["active"] = False


REFUSALS = [
    (_bad_dimensions, "ecckd_opt_create: bad model dimensions (ng=12 nt=1 np=16 ngas=5)"),
    (_no_planck, "ecckd_opt_create: Planck look-up table missing"),
    (_logarithmic, "ecckd_opt_create: logarithmic LUT interpolation is not supported (ckd_model.h:359 default is linear)"),
    (_ill_defined_gas, "ecckd_opt_create: gas 1 is ill-defined"),
    (_nlay(0), "ecckd_opt_create: nlay = 0 outside the supported range 1..128"),
    (_nlay(129), "ecckd_opt_create: nlay = 129 outside the supported range 1..128"),
    (_inconsistent_scene, "ecckd_opt_create: scene 1 is inconsistent (nlay/nband/arrays)"),
    (_other_nband, "ecckd_opt_create: scene 1 is inconsistent (nlay/nband/arrays)"),
    (_no_active_gas, "ecckd_opt_create: no active gas to optimise"),
]


@pytest.fixture(scope="module")
def fresh_context_cost():
    """cost at the initial state of the valid problem, from a handle on a context of its own"""
    from ecckd_amd import api
    with api.Context(0) as fresh:
        return _initial_cost(fresh, *_problem())


@pytest.mark.parametrize("spoil,message", REFUSALS, ids=["bad_dimensions", "no_planck", "logarithmic", "ill_defined_gas", "nlay_0",
                                                        "nlay_129", "other_nlay", "other_nband", "no_active_gas"])
def test_create_refuses_and_leaves_the_context_usable(ctx, fresh_context_cost, spoil, message):
    from ecckd_amd._lib import EcckdError
    model, scenes = _problem()
    spoil(model, scenes)
    with pytest.raises(EcckdError) as err:
        _opt(ctx, model, scenes)
    assert err.value.code == PARAMETER_ERROR and err.value.message == message
    assert _initial_cost(ctx, *_problem()) == fresh_context_cost


@pytest.mark.parametrize("unclamped", [False, True])
def test_evaluator_is_still_called_after_a_forward_pass(ctx, unclamped):
    model, scenes = _problem()
    opt = _opt(ctx, model, scenes)
    x0 = opt.initial_state()
    calls = []

    def bowl(x):
        calls.append(1)
        d = np.where(x0 > -1.0e20, x - (x0 + 0.1), 0.0)
        return 0.5 * float(d @ d), d

    opt.set_evaluator(bowl)
    opt.forward(x0, unclamped=unclamped)
    assert not calls                                         # the diagnostic pass is the device's own
    res = opt.minimize(max_iterations=2, convergence_criterion=0.0)
    assert len(calls) >= 3 and res["cost"] < bowl(x0)[0]
    opt.close()


@pytest.mark.parametrize("sw", [False, True])
def test_unclamped_forward_does_not_change_the_cost(ctx, sw):
    model, scenes = _problem(sw, ch4_low=True)
    plain = _opt(ctx, model, scenes)
    x = plain.initial_state()
    sizes = np.cumsum([0] + [g["molar_abs"].size for g in model["gases"] if g["active"]])
    x[sizes[3]:sizes[4]] += 9.0                               # negative optical depths: the clamp matters
    J_plain, g_plain = plain.cost_grad(x)
    plain.close()
    opt = _opt(ctx, model, scenes)
    od, _ = opt.forward(x)
    od_u, _ = opt.forward(x, unclamped=True)
    assert (od == 0.0).sum() > 10 and (od_u[od == 0.0] < 0.0).all()
    J, g = opt.cost_grad(x)
    assert J == J_plain and np.array_equal(g, g_plain)
    opt.close()


def test_a_handle_gives_back_its_device_memory(ctx):
    import torch
    model, scenes = _problem()
    free = lambda: torch.cuda.mem_get_info(ctx.device)[0]

    def cycle(alive=None):
        opt = _opt(ctx, model, scenes)
        x0 = opt.initial_state()
        opt.cost_grad(x0)
        opt.forward(x0)
        opt.minimize(max_iterations=3)
        if alive is not None:
            alive.append(free())
        opt.close()

    cycle()                                                  # warm-up: what the runtime keeps for itself is taken now
    noted = free()
    alive = []
    for _ in range(10):
        cycle(alive)
    footprint = noted - alive[0]                             # one handle with its minimizer workspace
    after = free()
    print(f"free before {noted} B, with a handle alive {alive[0]} B (footprint {footprint} B), after ten cycles {after} B")
    # (at these shapes the footprint read 2 MiB in a process of its own and 0 after the tests before it in the suite)
    assert after >= noted - footprint                        # a handle leaked per cycle would cost nine of them
