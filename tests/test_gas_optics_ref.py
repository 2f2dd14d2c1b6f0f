"""The numpy restatement of the gas-optics formula (gas_optics_ref.py) pinned to the CPU oracle's orc_ckd_optical_depth and
orc_ckd_planck, through ckd_synth.Oracle, with the bounds of test_run_ckd_gpu.py: optical depth 1e-12, applied termwise
(atol = 1e-12 * sum_i |od_i| over the gases' unclamped contributions, rtol = 0: the relative-linear gas contributes with
both signs), Planck rtol 1e-14."""
import numpy as np
import pytest

import ckd_synth
import gas_optics_cases as cases
import gas_optics_ref as ref


def oracle_parts(oracle, model, cols):
    """The oracle's optical depth of each gas alone (the other tables zeroed) -> [ngas, ncol, nlay, ng]"""
    scene = dict(cols, gas_present=None)
    out = []
    for i in range(len(model["gases"])):
        alone = dict(model, gases=[g if j == i else dict(g, molar_abs=np.zeros_like(g["molar_abs"]))
                                   for j, g in enumerate(model["gases"])])
        if alone.get("planck_function") is None:                # Oracle reads ng off the Planck table
            alone["planck_function"] = np.zeros((2, len(model["iband_per_g"])))
        o = ckd_synth.Oracle(oracle, alone, [scene], {})
        k = [g["molar_abs"] for g in alone["gases"]]
        o.coeffs = lambda x, k=k: k                             # the tables as they are, not exp(log k)
        out.append(o.optical_depth(o.x0, scene))
    return np.stack(out)


@pytest.mark.parametrize("ng,nt,np_,nconc,nlay", cases.SHAPES)
@pytest.mark.parametrize("edge", [False, True])
def test_optical_depth_matches_the_oracle(oracle, ng, nt, np_, nconc, nlay, edge):
    model = cases.model_lw(ng=ng, nt=nt, np_=np_, nconc=nconc)
    cols = cases.edge_columns(model, nlay=nlay) if edge else cases.columns(model, ncol=3, nlay=nlay)
    want = oracle_parts(oracle, model, cols)
    got = ref.gas_optical_depths(model, cols["pressure_hl"], cols["temperature_hl"], cols["vmr_fl"])
    assert np.isfinite(got).all()
    atol = cases.od_atol(want)
    err = np.abs(got - want)
    print("max termwise error / bound:", (err / np.where(atol > 0, atol, 1.0)).max())
    assert (err <= atol).all()
    assert (np.abs(got.sum(0) - want.sum(0)) <= atol).all()
    if not edge and ng > 1:
        assert (got[3] < 0).any() and (got[1] > 0).any()        # both signs among the contributions


def test_negative_tables_and_temperature_fl(oracle):
    model = cases.negative_model(cases.model_lw(ng=16))
    cols = cases.columns(model, ncol=3, nlay=9)
    want = oracle_parts(oracle, model, cols)
    got = ref.gas_optical_depths(model, cols["pressure_hl"], cols["temperature_hl"], cols["vmr_fl"])
    assert (np.abs(got - want) <= cases.od_atol(want)).all()
    assert (got.sum(0) < 0).any() and (got.sum(0) > 0).any()    # the clamp of the total has something to do
    # a full-level temperature of the caller's replaces the pressure-weighted mean
    p, T = cols["pressure_hl"], cols["temperature_hl"]
    t_fl = (T[:, :-1] * p[:, :-1] + T[:, 1:] * p[:, 1:]) / (p[:, :-1] + p[:, 1:])
    assert np.array_equal(ref.gas_optical_depths(model, p, T, cols["vmr_fl"], temperature_fl=t_fl), got)
    assert not np.array_equal(ref.gas_optical_depths(model, p, T, cols["vmr_fl"], temperature_fl=t_fl + 1.0), got)


def test_present_and_scaling():
    model = cases.model_lw(ng=16)
    cols = cases.columns(model, ncol=2, nlay=7)
    p, T, v = cols["pressure_hl"], cols["temperature_hl"], cols["vmr_fl"]
    full = ref.gas_optical_depths(model, p, T, v)
    part = ref.gas_optical_depths(model, p, T, v, present=[0, 1, 1, 0, 0], scaling=[1, 1, 4.0, 1, 1])
    assert not part[0].any() and not part[3].any() and not part[4].any()      # absent: nothing, the "none" gas included
    assert np.array_equal(part[1], full[1])
    v4 = v.copy()
    v4[:, 2] *= 4.0
    assert np.array_equal(part[2], ref.gas_optical_depths(model, p, T, v4)[2])


def test_planck_matches_the_oracle(oracle):
    model = cases.model_lw(ng=33)
    tpl = model["temperature_planck"]
    t = np.array([tpl[0] - 60.0, tpl[0] - 0.5, tpl[0], tpl[7], tpl[7] + 0.25, tpl[-2] + 0.75, tpl[-1], tpl[-1] + 60.0])
    o = ckd_synth.Oracle(oracle, model, [], {})
    want = o.planck(t)
    got = ref.planck(model, t)
    assert got.shape == (t.size, 33)
    assert np.allclose(got, want, rtol=cases.PLANCK_RTOL, atol=0.0)
    assert np.array_equal(got[3], model["planck_function"][7])                # on a node
    assert (got[-1] > got[-2]).all()                                          # extrapolated above the table
