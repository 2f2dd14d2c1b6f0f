"""Models and columns shared by the gas-optics tests (test_gas_optics_ref.py on the CPU, test_gas_optics_gpu.py on the device):
the synthetic five-gas model at the shapes where the interpolation can go wrong, columns held inside the table at both ends of
every axis, and tables with negative coefficients."""
import numpy as np

import ckd_synth

# (ng, nt, np_, nconc, nlay): every ng of the issue, both ends of nconc / np_ / nt, nlay 1 / 7 / 9
SHAPES = [(1, 5, 16, 4, 7), (16, 2, 2, 2, 1), (33, 5, 16, 2, 9), (64, 2, 16, 4, 7), (65, 5, 2, 4, 9)]

OD_BOUND = 1e-12        # termwise: atol = OD_BOUND * sum_i |od_i| over the gases' unclamped contributions, rtol = 0
PLANCK_RTOL = 1e-14


def model_lw(ng=12, nt=5, np_=16, nconc=4, seed=5):
    return ckd_synth.make_model(ng=ng, nt=nt, np_=np_, nconc=nconc, seed=seed, nband=min(3, ng))


def model_sw(ng=12, nt=5, np_=16, nconc=4, seed=5):
    return ckd_synth.make_model_sw(ng=ng, nt=nt, np_=np_, nconc=nconc, seed=seed, nband=min(3, ng))


def negative_model(model):
    """The co2 table negated at the first half of the g points: its optical depth is negative there, and so is the total
    where co2 outweighs the rest (the upper layers)."""
    gases = [dict(g) for g in model["gases"]]
    k = np.array(gases[2]["molar_abs"], copy=True)
    k[..., : max(1, k.shape[-1] // 2)] *= -1.0
    gases[2]["molar_abs"] = k
    return dict(model, gases=gases)


def columns(model, ncol=4, nlay=7, seed=3):
    """ch4 below its reference (contributions of both signs), all gases present."""
    s = ckd_synth.make_scenes(model, nscene=1, ncol=ncol, nlay=nlay, seed=seed, ch4_low=True)[0]
    return dict(pressure_hl=s["pressure_hl"], temperature_hl=s["temperature_hl"], vmr_fl=s["vmr_fl"])


def edge_columns(model, nlay=7, seed=3):
    """Four columns outside the table: 0 above its top, 60 K colder than the coldest node, h2o below its axis; 1 below its
    bottom, 60 K hotter than the hottest node, h2o above its axis; 2 with a layer between the last pressure node and the
    n - 1.0001 limit, and mole fractions of exactly 0 for the look-up-table gas and a linear gas; 3 as make_scenes gives it."""
    s = columns(model, ncol=4, nlay=nlay, seed=seed)
    lp, temp = np.asarray(model["log_pressure"]), np.asarray(model["temperature"])
    p, T, v = s["pressure_hl"], s["temperature_hl"], s["vmr_fl"]
    p[0] = np.exp(lp[0]) * np.linspace(0.01, 0.9, nlay + 1)
    T[0] = temp.min() - 60.0
    v[0, 1] = 1e-8
    p[1] = np.exp(lp[-1]) * np.linspace(1.05, 3.0, nlay + 1)
    T[1] = temp.max() + 60.0
    v[1, 1] = 0.5
    pm = np.exp(lp[-1] - 0.00005 * (lp[1] - lp[0]))
    p[2, -2:] = [0.99 * pm, 1.01 * pm]
    v[2, 1, 0] = 0.0
    v[2, 2, min(1, nlay - 1)] = 0.0
    assert (np.diff(p, axis=1) > 0).all()
    return s


def many_columns(model, ncol, nlay, seed=3):
    """ncol columns, all different: the four of columns() repeated, each repeat 0.1 K warmer and 1 % moister"""
    base = columns(model, ncol=4, nlay=nlay, seed=seed)
    c = np.arange(ncol)
    rep = (c // 4).astype(np.float64)
    vmr = base["vmr_fl"][c % 4].copy()
    vmr[:, 1] *= (1.0 + 0.01 * rep)[:, None]
    return dict(pressure_hl=base["pressure_hl"][c % 4].copy(), temperature_hl=base["temperature_hl"][c % 4] + 0.1 * rep[:, None],
                vmr_fl=vmr)


def od_atol(parts):
    """parts [ngas, ncol, nlay, ng] -> the termwise bound on any sum of them, clamped or not"""
    return OD_BOUND * np.abs(parts).sum(axis=0)
