"""float64 numpy restatement of what the gas-optics handle computes (ecckd_gas_optics_dev, ecckd_gas_optics_planck_dev):
CkdModel::calc_optical_depth as the optimiser's build_entries flattens it (opt_tables.cpp; ckd_model.cpp:925-1102), with
run_ckd's rule for absent gases, and CkdModel::calc_planck_function (:1107-1145).  Test infrastructure only."""
import numpy as np

MOLES_PER_PA = 1.0 / (9.80665 * 0.001 * 28.970)


def axis_pos(index0, n):
    """Lower node and the two weights on an evenly spaced axis of n nodes, held inside it (the n - 1.0001 rule)."""
    index0 = np.fmax(0.0, np.fmin(index0, n - 1.0001))
    i0 = index0.astype(np.int64)
    w1 = index0 - i0
    return i0, 1.0 - w1, w1


def gas_optical_depths(model, pressure_hl, temperature_hl, vmr_fl=None, temperature_fl=None, present=None, scaling=None):
    """Unclamped optical depth of every gas -> [ngas, ncol, nlay, ng]; zeros for a gas with present[i] == 0."""
    p, T = np.asarray(pressure_hl, dtype=np.float64), np.asarray(temperature_hl, dtype=np.float64)
    log_p, temp = np.asarray(model["log_pressure"]), np.asarray(model["temperature"])
    nt, np_ = temp.shape
    ncol, nlay = p.shape[0], p.shape[1] - 1
    p0, p1 = p[:, :-1], p[:, 1:]
    t_fl = np.asarray(temperature_fl) if temperature_fl is not None else (T[:, :-1] * p0 + T[:, 1:] * p1) / (p0 + p1)
    ip0, pw0, pw1 = axis_pos((np.log(0.5 * (p1 + p0)) - log_p[0]) / (log_p[1] - log_p[0]), np_)
    t_0 = pw0 * temp[0][ip0] + pw1 * temp[0][ip0 + 1]
    it0, tw0, tw1 = axis_pos((t_fl - t_0) / (temp[1, 0] - temp[0, 0]), nt)
    simple_weight = MOLES_PER_PA * (p1 - p0)
    out = []
    for i, g in enumerate(model["gases"]):
        k = np.asarray(g["molar_abs"], dtype=np.float64)
        ng = k.shape[-1]
        od = np.zeros((ncol, nlay, ng))
        if present is not None and not present[i]:
            out.append(od)
            continue
        if g["conc"] == "none":
            weight, vm = simple_weight, None
        else:
            vm = np.asarray(vmr_fl)[:, i, :] * (1.0 if scaling is None else scaling[i])
            weight = simple_weight * (vm - g.get("reference_vmr", 0.0)) if g["conc"] == "relative-linear" else simple_weight * vm
        if g["conc"] == "lut":
            v = np.asarray(g["vmr"], dtype=np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                ic0, cw0, cw1 = axis_pos((np.log(vm) - np.log(v[0])) / np.log(v[1] / v[0]), v.size)
            k4 = k
        else:
            ic0, cw0, cw1 = np.zeros_like(ip0), np.ones_like(pw0), np.ones_like(pw0)
            k4 = k[None]
        for dc in range(2 if g["conc"] == "lut" else 1):
            for dt in range(2):
                for dp in range(2):
                    coef = weight * (cw1 if dc else cw0) * (tw1 if dt else tw0) * (pw1 if dp else pw0)
                    od = od + coef[:, :, None] * k4[ic0 + dc, it0 + dt, ip0 + dp]
        out.append(od)
    return np.stack(out)


def rayleigh_optical_depth(model, pressure_hl):
    p = np.asarray(pressure_hl, dtype=np.float64)
    ray = model.get("rayleigh_molar_scattering")
    moles = (p[:, 1:] - p[:, :-1]) * MOLES_PER_PA
    ng = len(model["iband_per_g"])
    return moles[:, :, None] * (np.asarray(ray)[None, None, :] if ray is not None else np.zeros(ng))


def planck(model, temperature):
    """-> temperature.shape + (ng,)"""
    t = np.asarray(temperature, dtype=np.float64)
    tpl, pf = np.asarray(model["temperature_planck"], dtype=np.float64), np.asarray(model["planck_function"], dtype=np.float64)
    tindex0 = (t - tpl[0]) / (tpl[1] - tpl[0])
    it0 = np.minimum(np.maximum(tindex0, 0.0).astype(np.int64), tpl.size - 2)
    w1 = tindex0 - it0
    inside = (1.0 - w1)[..., None] * pf[it0] + w1[..., None] * pf[it0 + 1]
    below = (t / tpl[0])[..., None] * pf[0]
    return np.where((tindex0 >= 0)[..., None], inside, below)


def incoming(model, tsi):
    ssi = np.asarray(model["solar_irradiance"], dtype=np.float64)
    return tsi / np.cumsum(ssi)[-1] * ssi          # (the sum in g order, as the library adds it)
