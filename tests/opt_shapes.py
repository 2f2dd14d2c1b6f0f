"""Optimiser problems of a chosen shape for the edge tests of csrc/optimize.hip: a synthetic CKD model with ANY list of gases
on top of ecckd_amd.synthetic.ckd_model (whose axes, Planck table and band map it keeps, and whose defaults it does not touch:
bench.py and the tools use them), one or more training scenes, and the CPU oracle of both.

A gas list is a sequence of (conc, active), conc in "none" | "linear" | "lut" | "relative-linear".  The forward kernel's table
has nent = sum(8 if lut else 4) + (1 if shortwave: the Rayleigh entry) entries per cell (opt_tables.cpp, build_entries).
The features of the five-gas model of ckd_synth are kept as far as the list has room for them:
  * the first active gas has a g point where it does not absorb (k = 0: x pinned at -1e20),
  * the last active gas has a g point with k_min == 0 (the other bound rule),
  * inactive gases are where the list says so,
  * with three or more gases, the last one that has a concentration dependence and is not the relative-linear gas is absent
    from the (last) scene.
At most one relative-linear gas: the summed optical depth stays free of cancellation, unless `negative` asks for it - then
that gas sits at half its reference concentration in every third layer, and a state that raises its coefficients drives those
cells negative."""
import numpy as np

import ckd_synth
from ecckd_amd.synthetic import ckd_model

CFG = dict(flux_weight=0.2, flux_profile_weight=0.05, broadband_weight=0.4, spectral_boundary_weight=0.0,
           negative_od_penalty=1.0e4, pressure_weight_power=0.5, prior_error=4.0, pressure_corr=0.95,
           temperature_corr=0.95, conc_corr=0.9, cap_relative_linear=0.0)

# (conc, active): the five gases of ckd_synth.make_model
FIVE = (("none", True), ("lut", True), ("linear", True), ("relative-linear", True), ("linear", False))
SCALE = {"none": 2e-4, "lut": 3.0, "linear": 30.0, "relative-linear": 50.0}
REFERENCE_VMR = 1.8e-6


def nent_of(gases, sw):
    return sum(8 if conc == "lut" else 4 for conc, _ in gases) + (1 if sw else 0)


def gas_list(nent, sw=False, relative=False):
    """A gas list with exactly `nent` table entries per cell: one "none" gas first, [the relative-linear gas,] then look-up
    table gases, linear gases to fill, the last linear gas inactive when there are at least four gases."""
    n = nent - (1 if sw else 0)
    assert n >= 4 and n % 4 == 0, nent
    gases = [("none", True)]
    n -= 4
    if relative and n >= 4:
        gases.append(("relative-linear", True))
        n -= 4
    while n >= 12 or n == 8:
        gases.append(("lut", True))
        n -= 8
    while n > 0:
        gases.append(("linear", True))
        n -= 4
    if len(gases) >= 4 and gases[-1][0] == "linear":
        gases[-1] = ("linear", False)
    assert nent_of(gases, sw) == nent
    return tuple(gases)


def make_model(gases=FIVE, ng=12, nband=3, nt=3, np_=6, nconc=2, sw=False, seed=0, lut_vmr=(1e-6, 4e-2)):
    assert sum(conc == "relative-linear" for conc, _ in gases) <= 1
    m = ckd_model(ng=ng, nt=nt, np_=np_, nband=nband, seed=seed, nconc=nconc)
    rs = np.random.RandomState(seed + 31)
    g_strength = 10.0 ** np.linspace(-3.0, 1.5, ng)
    pfac = 0.2 + np.exp(0.4 * (m["log_pressure"] - m["log_pressure"][-1]))[:, None]
    count = {c: max(1, sum(conc == c for conc, _ in gases)) for c in SCALE}
    out = []
    for i, (conc, active) in enumerate(gases):
        shape = (nconc, nt, np_, ng) if conc == "lut" else (nt, np_, ng)
        k = SCALE[conc] / count[conc] * (0.002 if sw else 1.0) * g_strength * (1.0 + 0.3 * rs.uniform(size=shape)) * pfac
        g = dict(name=f"gas{i}", conc=conc, active=bool(active), molar_abs=k)
        if conc == "lut":
            g["vmr"] = np.exp(np.linspace(np.log(lut_vmr[0]), np.log(lut_vmr[1]), nconc))
        if conc == "relative-linear":
            g["reference_vmr"] = REFERENCE_VMR
        out.append(g)
    act = [g for g in out if g["active"]]
    act[0]["molar_abs"][..., 0] = 0.0
    for g in out:
        g["min_molar_abs"] = g["molar_abs"] * 0.5
        g["max_molar_abs"] = g["molar_abs"] * 2.0
    act[-1]["min_molar_abs"][..., min(3, ng - 1)] = 0.0
    m["gases"] = out
    if sw:
        ssi = rs.uniform(0.5, 1.5, ng)
        m["solar_irradiance"] = 1340.0 * ssi / ssi.sum()
        m["rayleigh_molar_scattering"] = 10.0 ** rs.uniform(-7.0, -5.5, ng)
        m["planck_function"] = None
        m["temperature_planck"] = None
        m["ng"] = ng
    return m


def absent_gas(gases):
    if len(gases) < 3:
        return None
    cand = [i for i, (conc, _) in enumerate(gases) if conc in ("linear", "lut")]
    return cand[-1] if cand else None


def make_scenes(model, nlay=6, ncol=2, nscene=1, sw=False, negative=False, seed=1, mu0=(1.0, 0.25), albedo=None):
    rs = np.random.RandomState(seed)
    gases = [(g["conc"], g["active"]) for g in model["gases"]]
    ngas = len(gases)
    scenes = []
    for s in range(nscene):
        p = np.empty((ncol, nlay + 1))
        T = np.empty((ncol, nlay + 1))
        vmr = np.empty((ncol, ngas, nlay))
        for c in range(ncol):
            p[c] = np.concatenate([[1.0], np.exp(np.linspace(np.log(5.0), np.log(101325.0 - 2000 * (c % 8)), nlay))])
            T[c] = 210.0 + 80.0 * (p[c] / p[c, -1]) ** 0.25 + rs.uniform(-3, 3, nlay + 1) + 4.0 * s
            pf = 0.5 * (p[c, 1:] + p[c, :-1]) / p[c, -1]
            for i, (conc, _) in enumerate(gases):
                if conc == "none":
                    vmr[c, i] = 1.0
                elif conc == "lut":
                    vmr[c, i] = np.clip(2e-2 * pf ** 3 * (1 + 0.5 * s) * rs.uniform(0.5, 1.5), 2e-6, 5e-2)
                elif conc == "linear":
                    vmr[c, i] = 4e-4 * (1.0 + s) * (1.0 + 0.1 * i)
                else:
                    # negative: every third layer below the reference (a thread of the forward kernel owns layers 8 or 16
                    # apart: its cells are a mix of clamped and unclamped ones)
                    vmr[c, i] = (np.where((np.arange(nlay) + c) % 3 == 0, 0.5, 1.5) if negative else 1.0 + 0.5 * (s + 1)) * REFERENCE_VMR
        present = np.ones(ngas, dtype=np.int32)
        ab = absent_gas(gases)
        if ab is not None and s == nscene - 1:
            present[ab] = 0
        sc = dict(pressure_hl=p, temperature_hl=T, vmr_fl=vmr, gas_present=present)
        if sw:
            sc["mu0"] = np.resize(np.asarray(mu0, dtype=np.float64), ncol)
            sc["tsi"] = 1361.0
            sc["albedo"] = (np.linspace(0.06, 0.3, model["nband"]) if albedo is None else np.asarray(albedo, dtype=np.float64))
        scenes.append(sc)
    return scenes


def add_truth(oracle, model, scenes, cfg, sw, seed):
    """The "line-by-line" band fluxes of the scenes: those of a perturbed model, through the oracle."""
    truth = dict(model, gases=[dict(g) for g in model["gases"]])
    rs = np.random.RandomState(seed + 5)
    for g in truth["gases"]:
        g["molar_abs"] = g["molar_abs"] * np.exp(0.25 * rs.normal(size=g["molar_abs"].shape))
    Orc = ckd_synth.OracleSW if sw else ckd_synth.Oracle
    t = Orc(oracle, truth, scenes, cfg)
    for s in scenes:
        bf = t.band_fluxes(t.x0, s)
        s["flux_dn"], s["flux_up"] = np.ascontiguousarray(bf[:, 0]), np.ascontiguousarray(bf[:, 1])
    return Orc(oracle, model, scenes, cfg)


def problem(oracle, gases=FIVE, ng=12, nband=3, nt=3, np_=6, nconc=2, nlay=6, ncol=2, nscene=1, sw=False, negative=False,
            seed=0, lut_vmr=(1e-6, 4e-2), **over):
    """-> model, scenes, cfg, oracle of (model, scenes)"""
    cfg = dict(CFG, **over)
    model = make_model(gases, ng=ng, nband=nband, nt=nt, np_=np_, nconc=nconc, sw=sw, seed=seed, lut_vmr=lut_vmr)
    scenes = make_scenes(model, nlay=nlay, ncol=ncol, nscene=nscene, sw=sw, negative=negative, seed=seed + 1)
    return model, scenes, cfg, add_truth(oracle, model, scenes, cfg, sw, seed)


def perturbed_state(orc, model, seed, negative=False):
    """x0 + 0.2 N(0,1) on the free elements; negative: the relative-linear gas raised by 9 (with the scene's concentration
    below the reference its optical depth is negative and large: clamp, penalty and the clamp mask of the kernels are live)."""
    rs = np.random.RandomState(seed)
    x0 = orc.x0
    free = x0 > -1.0e20
    x = x0 + np.where(free, 0.2 * rs.normal(size=x0.size), 0.0)
    if negative:
        off = np.cumsum([0] + orc.sizes)
        pos = [orc.active.index(i) for i, g in enumerate(model["gases"]) if g["conc"] == "relative-linear" and g["active"]]
        assert len(pos) == 1
        x[off[pos[0]]:off[pos[0] + 1]] += np.where(free[off[pos[0]]:off[pos[0] + 1]], 9.0, 0.0)
    return x, free


# ---- a 2 x 2 table with every layer strictly inside it: each node is referenced by every cell --------------------------

def inside_problem(oracle, ncol, nlay, ng=12, extra_lut=False, seed=0, **over):
    """One "none" gas on a table of nt = np_ = 2 nodes and profiles whose layers all lie strictly inside it in pressure and in
    temperature: each of the 4 nodes has exactly ncol * nlay references (transpose_entries of opt_tables.cpp keeps the entries
    with a non-zero coefficient).  extra_lut adds an active look-up-table gas whose concentration axis (8 nodes, 1e-6 ... 1e2)
    reaches far beyond the profiles' mole fractions: most of its nodes have no reference at all."""
    cfg = dict(CFG, **over)
    gases = (("none", True), ("lut", True)) if extra_lut else (("none", True),)
    model = make_model(gases, ng=ng, nband=3, nt=2, np_=2, nconc=8, seed=seed, lut_vmr=(1e-6, 1e2))
    logp = model["log_pressure"]
    rs = np.random.RandomState(seed + 3)
    p = np.empty((ncol, nlay + 1))
    T = np.empty((ncol, nlay + 1))
    for c in range(ncol):
        # half levels between 10 % and 90 % of the table's log-pressure range: every mid-layer pressure is inside as well
        lp = np.linspace(logp[0] + (0.10 + 0.01 * (c % 5)) * (logp[1] - logp[0]), logp[0] + 0.90 * (logp[1] - logp[0]), nlay + 1)
        p[c] = np.exp(lp)
        w = (lp - logp[0]) / (logp[1] - logp[0])
        t_lo = (1 - w) * model["temperature"][0, 0] + w * model["temperature"][0, 1]
        t_hi = (1 - w) * model["temperature"][1, 0] + w * model["temperature"][1, 1]
        T[c] = t_lo + (0.3 + 0.4 * rs.uniform(size=nlay + 1)) * (t_hi - t_lo)
    vmr = np.ones((ncol, len(gases), nlay))
    if extra_lut:
        vmr[:, 1, :] = 10.0 ** rs.uniform(-5.5, -3.5, size=(ncol, nlay))
    scenes = [dict(pressure_hl=p, temperature_hl=T, vmr_fl=vmr, gas_present=np.ones(len(gases), dtype=np.int32))]
    return model, scenes, cfg, add_truth(oracle, model, scenes, cfg, False, seed)


def references_per_node(model, scene, gas=0):
    """References of each (concentration,) temperature, pressure node of gas `gas`, from the axes alone: the cells whose
    interpolation weight at the node is non-zero (the positions are held inside the axes as axis_pos of opt_tables.cpp does)."""
    m = model
    g = m["gases"][gas]
    p, T = scene["pressure_hl"], scene["temperature_hl"]
    nt, np_ = m["temperature"].shape
    logp = m["log_pressure"]
    nconc = g["molar_abs"].shape[0] if g["conc"] == "lut" else 1
    count = np.zeros((nconc, nt, np_), dtype=np.int64)

    def pos(index0, n):
        index0 = max(0.0, min(index0, n - 1.0001))
        i0 = int(index0)
        return i0, 1.0 - (index0 - i0), index0 - i0

    for c in range(p.shape[0]):
        for l in range(p.shape[1] - 1):
            t_fl = (T[c, l] * p[c, l] + T[c, l + 1] * p[c, l + 1]) / (p[c, l] + p[c, l + 1])
            ip, wp0, wp1 = pos((np.log(0.5 * (p[c, l] + p[c, l + 1])) - logp[0]) / (logp[1] - logp[0]), np_)
            t0 = wp0 * m["temperature"][0, ip] + wp1 * m["temperature"][0, ip + 1]
            it, wt0, wt1 = pos((t_fl - t0) / (m["temperature"][1, 0] - m["temperature"][0, 0]), nt)
            ic, wc = 0, (1.0,)
            if g["conc"] == "lut":
                v = scene["vmr_fl"][c, gas, l]
                ic, wc0, wc1 = pos((np.log(v) - np.log(g["vmr"][0])) / np.log(g["vmr"][1] / g["vmr"][0]), nconc)
                wc = (wc0, wc1)
            for dc, a in enumerate(wc):
                for dt, b in enumerate((wt0, wt1)):
                    for dp, e in enumerate((wp0, wp1)):
                        if a * b * e != 0.0:
                            count[ic + dc, it + dt, ip + dp] += 1
    return count


# ---- shapes by the length of the state, for the minimiser's vector kernels (one active gas, nlay = 2, ncol = 1) ----------

MINIMISER_SHAPES = {1023: dict(conc="none", nt=3, np_=11, ng=31), 1024: dict(conc="none", nt=4, np_=16, ng=16),
                    1025: dict(conc="none", nt=5, np_=5, ng=41), 327680: dict(conc="lut", nconc=4, nt=8, np_=80, ng=128)}


def minimiser_problem(nx):
    """-> model, scenes (zero "truth" fluxes: the tests of the minimiser install their own cost function), the initial state
    with its log-space bounds as ecckd_opt_initial_state defines them (solve_adept.cpp:335-353), in numpy, and the indices of
    16 free elements, the last one among them, whose upper bound lies only 5e-10 above the initial state."""
    sh = MINIMISER_SHAPES[nx]
    model = make_model(((sh["conc"], True),), ng=sh["ng"], nband=3, nt=sh["nt"], np_=sh["np_"], nconc=sh.get("nconc", 2), seed=nx % 97)
    scenes = make_scenes(model, nlay=2, ncol=1)
    for s in scenes:
        s["flux_dn"] = np.zeros((1, 3, 3))
        s["flux_up"] = np.zeros((1, 3, 3))
    g = model["gases"][0]
    k, kmin, kmax = (g[n].ravel() for n in ("molar_abs", "min_molar_abs", "max_molar_abs"))   # (views: the model changes too)
    assert k.size == nx
    free = k > 0
    tight = np.unique(np.concatenate([np.nonzero(free)[0][::max(1, int(free.sum()) // 15)][:15], [nx - 1]]))
    assert free[tight].all()
    kmax[tight] = k[tight] * np.exp(5.0e-10)
    with np.errstate(divide="ignore"):
        x0 = np.where(free, np.log(np.where(free, k, 1.0)), -1.0e20)
        hi = np.where(free, np.log(np.where(free, kmax, 1.0)), -1.0e20)
        lo = np.where(kmin > 0, np.log(np.where(kmin > 0, kmin, 1.0)), np.minimum(3 * x0 - 2 * hi, hi - 1.0))
    lo = np.where(free, lo, -1.0e20)
    return model, scenes, x0, lo, hi, tight
