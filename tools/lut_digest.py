"""SHA-256 of everything the entry points of the g-point map return (csrc/create_lut.hip, K6/K7), on the EDGE, STRIDE and NONE_ONLY
layouts of tests/create_lut_cases.py - the chunk, lane-stride and no-chunk edges of its segmented reductions: a change that is
meant to leave their arithmetic alone is run once on the build before it and once on the build after it, on the same GPU, and
every digest has to be equal.  profiles/lut_digests.json holds the output of the build it was committed with; a ROCm
math-library update may change digests legitimately, which is why this is a tool and not a test.
Hashed: the counts; the averages (fit, min, max) under all eight methods, FLOAT and DOUBLE, Planck and solar weights, as plain
optical depth and as molar absorption, at 3, 43 and 54 layers (and the designed optical depths of EDGE at 54); the Planck table
with 1, 4 and 231 rows; the fractions for width_intervals; the erythemal weights; the row sums of FLOAT and DOUBLE rows; the map
in natural order, through lbl_fluxes_lw on EDGE.  The inputs are those of this tree's tests/create_lut_cases.py whichever build
runs.  Prints one JSON object.
usage: python tools/lut_digest.py [tree to import ecckd_amd from; default: this one]"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE
sys.path.insert(0, TREE)
from ecckd_amd import api, synthetic as syn  # noqa: E402  (before conftest, which puts its own tree in front)
assert os.path.dirname(os.path.dirname(os.path.abspath(api.__file__))) == TREE
sys.path.insert(0, os.path.join(HERE, "tests"))
import create_lut_cases as K  # noqa: E402

VMR = 4.0e-4
LAYERS = (3, 43, 54)
out = {}


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


with api.Context(0) as ctx:
    dev = lambda a: torch.as_tensor(np.array(a, order="C"), device=ctx.device)      # (a packed copy: the cached inputs are read-only)

    for name in ("EDGE", "STRIDE", "NONE_ONLY"):
        g, ng = K.layout_g(name), K.layout_ng(name)
        wn, dwn = K.grid(g.size)
        gm = api.GPointMap(ctx, dev(g), ng, dev(wn), dev(dwn))
        out[f"counts {name}"] = digest(gm.counts())
        ssi = dev(K.ssi_weights(g.size))
        for nlay in LAYERS:
            p = K.pressure_grid(nlay)
            t_fl = K.temperature_fl(p)
            for variant in ("smooth", "designed") if (name, nlay) == ("EDGE", 54) else ("smooth",):
                od64 = K.optical_depth(name, nlay, variant, "float64")
                for dtype in ("float32", "float64"):
                    od = dev(od64.astype(dtype))
                    for weights, kw in (("planck", dict(temperature_fl=t_fl)), ("solar", dict(ssi=ssi))):
                        for vmr in (-1.0, VMR):
                            for method in K.METHODS:
                                out[f"average {name} {nlay} {variant} {dtype} {weights} vmr={vmr} {method}"] = digest(
                                    *gm.average_optical_depth(p, od, method, vmr, **kw))
                    if nlay == 3:
                        out[f"sum_rows {name} {dtype}"] = digest(gm.sum_rows(od))
                    if (name, nlay, dtype) == ("EDGE", 43, "float32"):
                        out[f"natural order lbl_fluxes_lw {name} {nlay} {dtype}"] = digest(*gm.lbl_fluxes_lw(syn.temperature_profile(p), od))
        for nlut in (1, 4, 231):
            t = np.arange(120.0, 351.0)[:nlut] if nlut > 1 else np.array([287.5])
            out[f"planck_lut {name} {nlut}"] = digest(gm.planck_lut(t))
        if name == "NONE_ONLY":
            w1, w2 = np.array([599.0, 601.0]), np.array([601.0, 700.0])
        else:
            w1, w2, _ = K.width_intervals(g, wn, K.G_SMOOTH if name == "EDGE" else 0)
        out[f"gpoint_fraction {name} {len(w1)}"] = digest(gm.gpoint_fraction(w1, w2))
        gm.close()
        ewn, edwn = K.erythemal_grid(g.size)
        gm = api.GPointMap(ctx, dev(g), ng, dev(ewn), dev(edwn))
        out[f"erythemal {name}"] = digest(gm.erythemal_spectrum())
        gm.close()

print(json.dumps(out, indent=1))
