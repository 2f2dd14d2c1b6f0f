"""SHA-256 of everything the line-by-line flux entry points return, at the smallest shapes where each piece of their kernels can
go wrong (csrc/lbl_fluxes.hip, lbl_gpoint_fluxes.hip, lbl_gpoint_fluxes_sw.hip, lbl_scenarios.hip, lbl_fluxes_sw_rayleigh.hip, lbl_gpoint_fluxes_sw_rayleigh.hip, lbl_scenarios_sw_rayleigh.hip), and of every band entry with every band empty: a change that is meant to
leave their arithmetic alone is run once on the build before it and once on the build after it, on the same GPU, and every
digest has to be equal.  profiles/lbl_digests.json holds the output of the build it was committed with; a ROCm math-library
update may change digests legitimately, which is why this is a tool and not a test.
Inputs from ecckd_amd.synthetic with fixed seeds; g-point maps as tests/test_lbl_gpoint_fluxes*_gpu.py build them (7 % of the
points at no g point, a run of them at the start of the first tile, one g point that owns nothing when ng > 1).  Device
spectra are copied back before they are hashed.  Prints one JSON object.
usage: python tools/lbl_digest.py"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecckd_amd import api, synthetic as syn  # noqa: E402

BIG = 2 ** 20 + 4321          # 4113 tiles of 256: more than the 2048 blocks of a g-point launch, so several tiles per block
# (nlay, nwav, ng, dtype): one column through all 32 segments with a ragged last tile; 16 columns; more columns than the 48 an
# accumulator holds (several launches, only the first bins the points of no g point); 7 flux rows (only the tail batch)
GPOINT_LW = [(20, 20011, 1, "float64"), (54, 20011, 16, "float32"), (54, 20011, 200, "float32"), (3, BIG, 16, "float32")]
# (nlay, nwav, ng, nsza, dtype): ... five angles in launches of 2 + 2 + 1; the column split
GPOINT_SW = [(20, 20011, 1, 1, "float64"), (54, 20011, 32, 5, "float32"), (54, 20011, 200, 5, "float32"), (3, BIG, 16, 3, "float32")]
ANGLES = {1: (0.5,), 3: (0.1, 0.5, 0.9), 5: (0.1, 0.3, 0.5, 0.7, 0.9)}
BAND_CASES = [(54, 20011, "float32"), (17, 777, "float64")]
EMPTY_G = 3
out = {}


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if isinstance(a, torch.Tensor):
            a = a.cpu().numpy()
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def column(nlay, nwav, dtype, seed, lo=0.0, hi=3260.0, column_scale=30.0):
    p = syn.pressure_grid(nlay)
    wn, dwn = syn.wavenumber_grid(nwav, lo, hi)
    od = syn.optical_depth(np, p, wn, syn.SEED_BASE + seed, nlines=48 if nwav < 100000 else 6, dtype=dtype,
                           column_scale=column_scale, lo=lo, hi=hi)
    return p, wn, dwn, od


def g_points(nlay, nwav, ng):
    rng = np.random.default_rng(4321 + ng + nlay)
    g = rng.integers(0, ng, size=nwav).astype(np.int32)
    if ng > 1:
        g[g == EMPTY_G] = (EMPTY_G + 1) % ng
    g[rng.random(nwav) < 0.07] = -1
    g[:3] = -1
    return g


def bands13(nwav):
    """13 bands over the spectrum, none a multiple of 256 wide, one of them empty (begin 0, end -1)."""
    edges = np.linspace(0, nwav, 14).astype(np.int64)
    begin, end = edges[:-1].copy(), edges[1:] - 1
    begin[5], end[5] = 0, -1
    assert all((e - b + 1) % 256 for b, e in zip(begin, end) if e >= b)
    return begin, end


def scales(nscen, ngas, nlay, seed):
    rs = np.random.RandomState(seed)
    sc = rs.uniform(0.25, 4.0, (nscen, ngas, 1)) * np.ones((1, 1, nlay))
    sc[0] = 1.0
    if nscen > 2:
        sc[1, 0] = 0.0
        sc[2] = rs.uniform(0.5, 2.0, (ngas, nlay))
    return sc


with api.Context(0) as ctx:
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)

    for nlay, nwav, ng, dtype in GPOINT_LW:
        p, wn, dwn, od = column(nlay, nwav, dtype, seed=11)
        t_hl, d_wn, d_dwn, d_od = syn.temperature_profile(p), dev(wn), dev(dwn), dev(od)
        gm = api.GPointMap(ctx, dev(g_points(nlay, nwav, ng)), ng, d_wn, d_dwn)
        out[f"gpoint_lw {nlay} {nwav} {ng} {dtype}"] = digest(*gm.lbl_fluxes_lw(t_hl, d_od))
        gm.close()
        out[f"spectral_lw {nlay} {nwav} {dtype}"] = digest(*api.lbl_spectral_fluxes_lw(ctx, t_hl, d_wn, d_dwn, d_od))

    for nlay, nwav, ng, nsza, dtype in GPOINT_SW:
        p, wn, dwn, od = column(nlay, nwav, dtype, seed=11, lo=250.0, hi=50000.0, column_scale=3.0)
        d_wn, d_dwn, d_od = dev(wn), dev(dwn), dev(od)
        ssi, albedo = dev(syn.solar_spectral_irradiance(wn, dwn)), dev(np.where(wn < 12000.0, 0.2, 0.05))
        gm = api.GPointMap(ctx, dev(g_points(nlay, nwav, ng)), ng, d_wn, d_dwn)
        for alb in (None, albedo):
            tag = f"{nlay} {nwav} {ng} nsza={nsza} {dtype} albedo={alb is not None}"
            out["gpoint_sw " + tag] = digest(*gm.lbl_fluxes_sw(ANGLES[nsza], ssi, d_od, alb))
            out["spectral_sw " + tag] = digest(*api.lbl_spectral_fluxes_sw(ctx, ANGLES[nsza], ssi, d_od, alb))
        # Rayleigh scattering per g point and per wavenumber: a float32 Rayleigh spectrum beside the absorber as it is
        d_ray = dev(syn.optical_depth(np, p, wn, syn.SEED_BASE + 7, nlines=6, column_scale=0.3, lo=250.0, hi=50000.0).astype("float32"))
        tag = f"{nlay} {nwav} {ng} nsza={nsza} {dtype}"
        out["gpoint_sw_rayleigh " + tag] = digest(*gm.lbl_fluxes_sw_rayleigh(ANGLES[nsza], ssi, d_od, d_ray, albedo))
        out["spectral_sw_rayleigh " + tag] = digest(*api.lbl_spectral_fluxes_sw_rayleigh(ctx, ANGLES[nsza], ssi, d_od, d_ray, albedo))
        gm.close()

    for nlay, nwav, dtype in BAND_CASES:
        begin, end = bands13(nwav)
        p, wn, dwn, od = column(nlay, nwav, dtype, seed=5)
        for nangle in (0, 4):
            out[f"band_lw {nlay} {nwav} {dtype} nangle={nangle}"] = digest(*api.lbl_band_fluxes_lw(
                ctx, syn.temperature_profile(p), dev(wn), dev(dwn), dev(od), begin, end, boundary=True, nangle=nangle))
        p, wn, dwn, od = column(nlay, nwav, dtype, seed=5, lo=250.0, hi=50000.0, column_scale=3.0)
        ssi, albedo = dev(syn.solar_spectral_irradiance(wn, dwn)), dev(np.where(wn < 12000.0, 0.2, 0.05))
        for alb in (None, albedo):
            out[f"band_sw {nlay} {nwav} {dtype} albedo={alb is not None}"] = digest(*api.lbl_band_fluxes_sw(
                ctx, 0.5, ssi, dev(od), begin, end, albedo=alb, boundary=True))

        # Rayleigh scattering: 1 and 5 angles; the Rayleigh spectrum float32 beside a float64 absorber, then the reverse
        ray = syn.optical_depth(np, p, wn, syn.SEED_BASE + 7, nlines=6, column_scale=0.3, lo=250.0, hi=50000.0)
        for nsza in (1, 5):
            for abs_dt, ray_dt in (("float64", "float32"), ("float32", "float64")):
                out[f"band_sw_rayleigh {nlay} {nwav} nsza={nsza} abs={abs_dt} ray={ray_dt}"] = digest(*api.lbl_band_fluxes_sw_rayleigh(
                    ctx, ANGLES[nsza], ssi, dev(od.astype(abs_dt)), dev(ray.astype(ray_dt)), begin, end, albedo=albedo, boundary=True))

    # Rayleigh scattering per g point, host arrays: ncol 2, nlay 16, ng 7
    rs = np.random.RandomState(5)
    odg, rayg, inc = rs.uniform(0.0, 0.4, (2, 16, 7)), rs.uniform(0.0, 0.05, (2, 16, 7)), rs.uniform(10.0, 300.0, (2, 7))
    rayg[:, 1, 2] = 0.0
    out["rt_sw_gpoints_rayleigh 2 16 7"] = digest(*api.rt_sw_gpoints_rayleigh(ctx, 0.5, 0.15, inc, odg, rayg))

    # every band empty (begin 0, end -1): each band entry returns zeros, on the host and in the boundary spectra
    nlay, nwav = 3, 300
    begin, end = np.zeros(2, dtype=np.int64), -np.ones(2, dtype=np.int64)
    p, wn, dwn, od = column(nlay, nwav, "float64", seed=5, lo=250.0, hi=50000.0, column_scale=3.0)
    t_hl, d_wn, d_dwn, d_od, one = syn.temperature_profile(p), dev(wn), dev(dwn), dev(od), np.ones((2, 1, nlay))
    ssi = dev(syn.solar_spectral_irradiance(wn, dwn))
    out["empty band_lw"] = digest(*api.lbl_band_fluxes_lw(ctx, t_hl, d_wn, d_dwn, d_od, begin, end, boundary=True))
    out["empty band_sw"] = digest(*api.lbl_band_fluxes_sw(ctx, 0.5, ssi, d_od, begin, end, boundary=True))
    out["empty band_sw_rayleigh"] = digest(*api.lbl_band_fluxes_sw_rayleigh(ctx, ANGLES[3], ssi, d_od, d_od, begin, end, boundary=True))
    out["empty scenarios_lw"] = digest(*api.lbl_band_fluxes_lw_scenarios(ctx, t_hl, d_wn, d_dwn, [d_od], one, begin, end, boundary=True))
    out["empty scenarios_sw"] = digest(*api.lbl_band_fluxes_sw_scenarios(ctx, ANGLES[3], ssi, [d_od], one, begin, end, boundary=True))
    out["empty scenarios_sw_rayleigh"] = digest(*api.lbl_band_fluxes_sw_rayleigh_scenarios(ctx, ANGLES[3], ssi, [d_od], d_od, one, begin, end,
                                                                                          boundary=True))

    # scenarios: a FLOAT and a DOUBLE gas; longwave 11 scenarios (two launches at 8 slots); shortwave 7 scenarios with 1 and 5
    # angles (3 scenarios per launch); 130 layers: 5 longwave scenarios per launch, and the 8 angles of one shortwave scenario
    # over two launches of 4
    nwav = 3000
    begin, end = bands13(nwav)
    for nlay in (3, 54, 130):
        p = syn.pressure_grid(nlay)
        wn, dwn = syn.wavenumber_grid(nwav)
        ods = [dev(syn.optical_depth(np, p, wn, syn.SEED_BASE + 21 + g, nlines=48, dtype=dt)) for g, dt in enumerate(("float32", "float64"))]
        nscen = 6 if nlay == 130 else 11
        for nangle in (0,) if nlay == 130 else (0, 4):
            out[f"scenarios_lw {nlay} nscen={nscen} nangle={nangle}"] = digest(*api.lbl_band_fluxes_lw_scenarios(
                ctx, syn.temperature_profile(p), dev(wn), dev(dwn), ods, scales(nscen, 2, nlay, 3), begin, end, boundary=True, nangle=nangle))
        wn, dwn = syn.wavenumber_grid(nwav, 250.0, 50000.0)
        ods = [dev(syn.optical_depth(np, p, wn, syn.SEED_BASE + 31 + g, nlines=48, dtype=dt, column_scale=3.0, lo=250.0, hi=50000.0))
               for g, dt in enumerate(("float32", "float64"))]
        ssi, albedo = dev(syn.solar_spectral_irradiance(wn, dwn)), dev(np.where(wn < 12000.0, 0.2, 0.05))
        nscen = 2 if nlay == 130 else 7
        for mu in (np.linspace(0.15, 0.85, 8),) if nlay == 130 else (ANGLES[1], ANGLES[5]):
            for alb in (albedo,) if nlay == 130 else (None, albedo):
                out[f"scenarios_sw {nlay} nscen={nscen} nsza={len(mu)} albedo={alb is not None}"] = digest(*api.lbl_band_fluxes_sw_scenarios(
                    ctx, mu, ssi, ods, scales(nscen, 2, nlay, 5), begin, end, albedo=alb, boundary=True))
        # with Rayleigh scattering: the same absorbers and scalings, a float32 row that scatters; 1 and 5 angles, with albedo
        if nlay != 130:
            d_ray = dev(syn.optical_depth(np, p, wn, syn.SEED_BASE + 7, nlines=6, column_scale=0.3, lo=250.0, hi=50000.0).astype("float32"))
            for mu in (ANGLES[1], ANGLES[5]):
                out[f"scenarios_sw_rayleigh {nlay} nscen={nscen} nsza={len(mu)}"] = digest(*api.lbl_band_fluxes_sw_rayleigh_scenarios(
                    ctx, mu, ssi, ods, d_ray, scales(nscen, 2, nlay, 5), begin, end, albedo=albedo, boundary=True))

print(json.dumps(out, indent=1))
