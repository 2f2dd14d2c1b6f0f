"""Wall time of api.Optimizer(...) - ecckd_opt_create: the host tables, their upload, the work buffers - at the shapes of
bench.py --config 4 (ng = 64, 6 x 53 (T, p) grid, 12 mole fractions, 8 scenarios x 50 columns x 54 layers; shortwave: three zenith
angles per column), longwave and shortwave.  Truth fluxes are zeros: the tables do not depend on their values.  Prints one JSON
line with each region's times in ms and their median.
usage: python tools/opt_create_probe.py [repeats]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecckd_amd import api, synthetic as syn  # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out = {}
with api.Context(0) as ctx:
    for region in ("longwave", "shortwave"):
        model = syn.ckd_model(ng=64, nt=6, np_=53, nband=13, seed=11, nconc=12)
        scenes = syn.ckd_scenes(model, nscene=8, ncol=50, nlay=54, seed=13)
        if region == "shortwave":
            rs = np.random.RandomState(110)
            ssi = rs.uniform(0.5, 1.5, 64)
            model.update(solar_irradiance=1340.0 * ssi / ssi.sum(), rayleigh_molar_scattering=10.0 ** rs.uniform(-7.0, -5.5, 64),
                         planck_function=None, temperature_planck=None)
            mu0 = (1.0, 0.5, 0.1)
            rep = lambda a: np.ascontiguousarray(np.repeat(a, len(mu0), axis=0))
            scenes = [dict(pressure_hl=rep(s["pressure_hl"]), temperature_hl=rep(s["temperature_hl"]), vmr_fl=rep(s["vmr_fl"]),
                           gas_present=s["gas_present"], mu0=np.tile(np.asarray(mu0), s["pressure_hl"].shape[0]), tsi=1361.0,
                           albedo=np.full(13, 0.15)) for s in scenes]
        for s in scenes:
            ncol, nhl = s["pressure_hl"].shape
            s["flux_dn"] = s["flux_up"] = np.zeros((ncol, nhl, 13))
        cfg = dict(flux_weight=0.2, flux_profile_weight=0.0, broadband_weight=0.5, prior_error=4.0, pressure_corr=0.95,
                   temperature_corr=0.95, conc_corr=0.95)
        api.Optimizer(ctx, model, scenes, **cfg).close()          # warm-up
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            opt = api.Optimizer(ctx, model, scenes, **cfg)
            ms.append((time.perf_counter() - t0) * 1e3)
            opt.close()
        out[region] = {"create_ms": [round(v, 3) for v in ms], "median_ms": round(float(np.median(ms)), 3), "nx": opt.nx}
print(json.dumps(out))
