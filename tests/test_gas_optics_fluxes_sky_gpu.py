"""The resident fluxes under clouds and over a real surface (api.GasOptics.fluxes_lw / fluxes_sw with the cloud and surface
arguments, ecckd_gas_optics_fluxes_{lw,sw}_sky_dev).  Every comparison runs over every (column, g, level).

nothing given      the sky entries with sky NULL or all-NULL are the clear calls bit for bit (the clear kernel runs)
neutral values     zero clouds, emissivity 1, skin = temperature_hl[nlay] through the sky kernel: per g within 1e-12 x the largest
                   clear flux of the (column, g), the project's termwise bound (cases.OD_BOUND); seen on the device: 0 (bit equal)
longwave cloud     against api.rt_lw_gpoints(planck, optical_depth + cloud_od[..., iband]) on the device's own optical depths and
                   Planck values, 1e-12 x the largest composed flux; sums and heating rates by the bounds of the clear test
longwave surface   against allsky_ref.lw_fluxes on the same inputs; the bound is the larger of 1e-12 and 10 x the discrepancy,
                   measured here and printed, between that restatement at emissivity 1 and api.rt_lw_gpoints, times the largest
                   flux of the (column, g)
shortwave          against allsky_ref.two_stream_closed fed GasOptics.optical_depth and incoming: 1e-9 * mu0 * incoming[g], the
                   bound of the Rayleigh device tests
independence       bit for bit: alone / in a batch / moved, default / forced grid, a second handle, float32 = rounded float64,
                   broadband with and without the other outputs, another column's cloud
refusals           each by its message, the context usable afterwards"""
import ctypes as C

import numpy as np
import pytest

import allsky_ref as ar
import gas_optics_cases as cases
import test_gas_optics_fluxes_gpu as clear

pytestmark = pytest.mark.gpu

EPS = clear.EPS
TSI = clear.TSI
SW_BOUND = 1e-9                      # per unit mu0 * incoming[g]
SHAPES = cases.SHAPES + [(257, 2, 2, 2, 7)]


@pytest.fixture(scope="module")
def api():
    from ecckd_amd import api
    return api


def dev(ctx, a):
    return None if a is None else clear.dev(ctx, a)


def banded(model, nband):
    """the model with nband 1, or with 3 bands whose iband_per_g is not monotone (1, 0, 2, 1, 0, 2, ...)"""
    ng = len(model["iband_per_g"])
    ib = np.zeros(ng, dtype=np.int32) if nband == 1 or ng < 3 else ((np.arange(ng) * 2 + 1) % 3).astype(np.int32)
    return dict(model, iband_per_g=ib, nband=int(ib.max()) + 1)


def make_model(kind, nband=3, **kw):
    return banded(clear.make_model(kind, **kw), nband)


def nbands(model):
    return int(np.max(model["iband_per_g"])) + 1


def clouds(model, ncol, nlay, seed=1, lo=1e-2, hi=20.0, layout=None):
    """cloud_od [ncol, nlay, nband]: log-uniform in lo..hi in half the (cell, band) pairs, exactly 0 in the rest.  layout: per
    column c % 4 -> clouds in every layer, in none, in the top layer only, in the bottom layer only."""
    rng = np.random.default_rng(seed)
    shape = (ncol, nlay, nbands(model))
    od = np.exp(rng.uniform(np.log(lo), np.log(hi), shape))
    if layout is None:
        return np.where(rng.random(shape) < 0.5, od, 0.0)
    for c in range(ncol):
        if c % 4 == 1:
            od[c] = 0.0
        elif c % 4 == 2:
            od[c, 1:] = 0.0
        elif c % 4 == 3:
            od[c, :-1] = 0.0
    return od


def scatterers(model, ncol, nlay, seed=2, amax=0.9):
    """cloud_ssa of {0.5, 0.9, 0.999, 0.999999, 1}, cloud_asymmetry in 0..amax, [ncol, nlay, nband]"""
    rng = np.random.default_rng(seed)
    shape = (ncol, nlay, nbands(model))
    return rng.choice([0.5, 0.9, 0.999, 0.999999, 1.0], shape), rng.uniform(0.0, amax, shape)


def fused(ctx, go, kind, cols, mu0=None, albedo=None, everything=True, **kw):
    """clear.fused with the sky arguments (numpy) as device tensors"""
    sky = {k: dev(ctx, kw.pop(k)) for k in ("cloud_od", "cloud_ssa", "cloud_asymmetry", "surface_emissivity", "skin_temperature") if k in kw}
    if everything:
        kw = dict(dict(bands=True, spectral=True), **kw)
    return clear.fused(ctx, go, kind, cols, mu0, albedo, **sky, **kw)


def device_optics(ctx, go, cols):
    p, T, v = (dev(ctx, cols[k]) for k in ("pressure_hl", "temperature_hl", "vmr_fl"))
    o = go.optical_depth(p, T, v)
    return {k: t.cpu().numpy() for k, t in o.items()}


def angles(api, nangle):
    if nangle == 0:
        return [1.66], [1.0]
    mu, w = api.gauss_legendre_01(nangle)
    return list(1.0 / mu), list(2.0 * w * mu)


def check_sums(model, cols, got, keys):
    """broadband and band outputs against the call's own per-g fluxes (ascending g; (ng - 1) half-ulps of the absolute sum for
    another order), heating rates by the clear test's check"""
    ib = np.asarray(model["iband_per_g"])
    for k in keys:
        s = got["spectral_" + k]
        ng = s.shape[-1]
        clear.assert_within(got[k], s.sum(-1), (ng - 1) * EPS * np.abs(s).sum(-1), "broadband " + k)
        for b in range(int(ib.max()) + 1):
            sel = ib == b
            clear.assert_within(got["band_" + k][..., b], s[..., sel].sum(-1), (ng - 1) * EPS * np.abs(s[..., sel]).sum(-1), f"band {b} " + k)
    clear.check_heating(cols, got)


# ------------------------------------------------------------------------------------------------------- 1 nothing given
def raw_call(ctx, go, kind, cols, mu0, albedo, sky, entry="sky"):
    """the C entries themselves with every output asked for -> dict of numpy arrays; sky: None (NULL) or a _lib.FluxSky"""
    import torch
    from ecckd_amd import _lib, api
    p, T, v = (dev(ctx, cols[k]) for k in ("pressure_hl", "temperature_hl", "vmr_fl"))
    ncol, nhl = cols["pressure_hl"].shape
    nlay, lw = nhl - 1, kind.startswith("lw")
    shapes = dict(flux_dn=(ncol, nhl), flux_up=(ncol, nhl), band_flux_dn=(ncol, nhl, go.nband), band_flux_up=(ncol, nhl, go.nband),
                  spectral_flux_dn=(ncol, nhl, go.ng), spectral_flux_up=(ncol, nhl, go.ng), heating_rate=(ncol, nlay))
    if not lw:
        shapes.update(flux_dn_direct=(ncol, nhl), band_flux_dn_direct=(ncol, nhl, go.nband), spectral_flux_dn_direct=(ncol, nhl, go.ng))
    out, o = {}, _lib.FluxOutputs()
    for k, s in shapes.items():
        out[k] = torch.full(s, np.nan, dtype=torch.float64, device=ctx.device)
        setattr(o, k, out[k].data_ptr())
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    skyp = None if sky is None else C.addressof(sky)
    ctx.fence_from_torch()
    if lw:
        head = (go.handle, int(kind[2:]), ncol, nlay, ptr(p), ptr(T), None, ptr(v), None, None, _lib.F64, C.byref(o))
        rc = ctx.lib.ecckd_gas_optics_fluxes_lw_sky_dev(*head, skyp) if entry == "sky" else ctx.lib.ecckd_gas_optics_fluxes_lw_dev(*head)
    else:
        m, a = dev(ctx, mu0), dev(ctx, albedo)
        tail = (ncol, nlay, ptr(p), ptr(T), None, ptr(v), None, None, ptr(m), ptr(a), TSI, _lib.F64, C.byref(o))
        rc = ctx.lib.ecckd_gas_optics_fluxes_sw_sky_dev(go.handle, *tail, skyp) if entry == "sky" else \
            ctx.lib.ecckd_gas_optics_fluxes_sw_dev(go.handle, 1, *tail)
    api.check(rc)
    ctx.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.parametrize("kind", ["lw0", "lw4", "sw_twostream"])
def test_nothing_given_is_the_clear_call(ctx, api, kind):
    from ecckd_amd import _lib
    model = make_model(kind, ng=33)
    go = api.GasOptics(ctx, model)
    try:
        cpb = go.fluxes_geometry(7, mode=0 if kind.startswith("lw") else 2)["columns_per_block"]
        ncol = cpb + 1
        cols = cases.many_columns(model, ncol, 7)
        mu0, albedo = clear.sun(ncol)
        want = raw_call(ctx, go, kind, cols, mu0, albedo, None, entry="clear")
        assert all(np.isfinite(v).all() and v.any() for v in want.values())
        empty = _lib.FluxSky()
        scaled = _lib.FluxSky()
        scaled.delta_eddington = 0 if kind.startswith("lw") else 1
        for sky in (None, empty, scaled):
            got = raw_call(ctx, go, kind, cols, mu0, albedo, sky)
            for k in want:
                assert np.array_equal(got[k], want[k]), k
        # and the methods without the new arguments, or with all of them None, are the clear methods
        a = fused(ctx, go, kind, cols, mu0, albedo)
        none = dict(cloud_od=None, surface_emissivity=None, skin_temperature=None) if kind.startswith("lw") else \
            dict(cloud_od=None, cloud_ssa=None, cloud_asymmetry=None)
        b = fused(ctx, go, kind, cols, mu0, albedo, **none)
        names = {"dn": "flux_dn", "up": "flux_up", "hr": "heating_rate", "direct": "flux_dn_direct"}
        for k in a:
            pre = "band_" if k.startswith("band_") else ("spectral_" if k.startswith("spectral_") else "")
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], want[pre + names[k[len(pre):]]]), k
    finally:
        go.close()


# ----------------------------------------------------------------------------------------------------- 2 neutral values
@pytest.mark.parametrize("kind", ["lw0", "lw4", "sw_twostream"])
@pytest.mark.parametrize("ng,nband", [(33, 3), (16, 1), (257, 3)])
def test_neutral_values_are_the_clear_call(ctx, api, kind, ng, nband):
    model = make_model(kind, nband=nband, ng=ng, nt=2, np_=2, nconc=2) if ng == 257 else make_model(kind, nband=nband, ng=ng)
    go = api.GasOptics(ctx, model)
    try:
        lw = kind.startswith("lw")
        nlay = 9
        ncol = go.fluxes_geometry(nlay, mode=0 if lw else 2)["columns_per_block"] + 1
        cols = cases.many_columns(model, ncol, nlay)
        mu0, albedo = clear.sun(ncol)
        want = fused(ctx, go, kind, cols, mu0, albedo)
        zeros = np.zeros((ncol, nlay, nbands(model)))
        if lw:
            sky = dict(cloud_od=zeros, surface_emissivity=np.ones((ncol, nbands(model))), skin_temperature=cols["temperature_hl"][:, -1].copy())
        else:
            sky = dict(cloud_od=zeros, cloud_ssa=np.full_like(zeros, 0.9), cloud_asymmetry=np.full_like(zeros, 0.8))
        got = fused(ctx, go, kind, cols, mu0, albedo, **sky)
        keys = ["dn", "up"] + ([] if lw else ["direct"])
        scale = np.max([np.abs(want["spectral_" + k]).max(axis=1, keepdims=True) for k in keys], axis=0)
        worst = max(float((np.abs(got["spectral_" + k] - want["spectral_" + k]) / scale).max()) for k in keys)
        print(f"{kind} ng={ng}: neutral sky against clear, worst per-g error / largest flux = {worst:.3e};",
              "bit equal" if all(np.array_equal(got[k], want[k]) for k in want) else "not bit equal")
        for k in keys:
            clear.assert_within(got["spectral_" + k], want["spectral_" + k], cases.OD_BOUND * scale * np.ones_like(want["spectral_" + k]), "per-g " + k)
        check_sums(model, cols, got, keys)
    finally:
        go.close()


# ---------------------------------------------------------------------------------------------------- 3 longwave, cloud
def lw_cloud_case(ctx, api, go, model, nangle, cols, seed=1):
    ncol, nlay = cols["pressure_hl"].shape[0], cols["pressure_hl"].shape[1] - 1
    cloud = clouds(model, ncol, nlay, seed=seed)
    cloud[0, 0] = -1.0                                               # not > 0: adds nothing
    got = fused(ctx, go, f"lw{nangle}", cols, cloud_od=cloud)
    od = device_optics(ctx, go, cols)["optical_depth"]
    added = np.where(cloud > 0.0, cloud, 0.0)[..., np.asarray(model["iband_per_g"])]
    planck = go.planck(dev(ctx, cols["temperature_hl"])).cpu().numpy()
    dn, up = api.rt_lw_gpoints(ctx, planck, od + added, nangle=nangle)
    clear.check(model, cols, got, dict(dn=dn, up=up))
    return got


@pytest.mark.parametrize("nangle", [0, 1, 4])
@pytest.mark.parametrize("ng,nt,np_,nconc,nlay", SHAPES)
def test_longwave_cloud_against_the_composed_calls(ctx, api, ng, nt, np_, nconc, nlay, nangle):
    model = make_model("lw", nband=1 if ng in (16, 65) else 3, ng=ng, nt=nt, np_=np_, nconc=nconc)
    go = api.GasOptics(ctx, model)
    try:
        got = lw_cloud_case(ctx, api, go, model, nangle, cases.edge_columns(model, nlay=nlay))
        plain = fused(ctx, go, f"lw{nangle}", cases.edge_columns(model, nlay=nlay))
        assert not np.array_equal(got["spectral_dn"], plain["spectral_dn"])
    finally:
        go.close()


@pytest.fixture(scope="module")
def lw33(ctx, api):
    model = make_model("lw", ng=33)
    go = api.GasOptics(ctx, model)
    yield model, go
    go.close()


@pytest.fixture(scope="module")
def sw33(ctx, api):
    model = make_model("sw", ng=33)
    go = api.GasOptics(ctx, model)
    yield model, go
    go.close()


@pytest.mark.parametrize("columns", [-1, 0, 1])
def test_longwave_cloud_at_the_group_edges(ctx, api, lw33, columns):
    model, go = lw33
    cpb = go.fluxes_geometry(9)["columns_per_block"]
    assert cpb == 7
    lw_cloud_case(ctx, api, go, model, 1, cases.many_columns(model, cpb + columns, 9), seed=4)


# -------------------------------------------------------------------------------------------------- 4 longwave, surface
@pytest.mark.parametrize("nangle", [0, 1, 4])
@pytest.mark.parametrize("ng,nband", [(33, 3), (16, 1)])
def test_longwave_emissivity_and_skin_temperature(ctx, api, ng, nband, nangle):
    model = make_model("lw", nband=nband, ng=ng)
    go = api.GasOptics(ctx, model)
    try:
        nlay = 9
        ncol = go.fluxes_geometry(nlay)["columns_per_block"] + 1
        cols = cases.many_columns(model, ncol, nlay)
        ib = np.asarray(model["iband_per_g"])
        rng = np.random.default_rng(7)
        cloud = clouds(model, ncol, nlay, seed=5)
        emis = rng.uniform(0.5, 1.0, (ncol, nbands(model)))
        skin = cols["temperature_hl"][:, -1] + rng.uniform(-8.0, 8.0, ncol)
        od = device_optics(ctx, go, cols)["optical_depth"] + cloud[..., ib]
        planck = go.planck(dev(ctx, cols["temperature_hl"])).cpu().numpy()
        planck_skin = go.planck(dev(ctx, skin)).cpu().numpy()                                   # [ncol, ng]
        sec, wgt = angles(api, nangle)

        def restated(emissivity, b_skin):
            dn, up = np.empty_like(planck), np.empty_like(planck)
            for c in range(ncol):
                dn[c], up[c] = ar.lw_fluxes(planck[c], od[c], sec, wgt, emissivity[c][ib] if emissivity is not None else 1.0,
                                            None if b_skin is None else b_skin[c])
            return dn, up

        # the restatement's own distance from the device's transfer, at emissivity 1 on these very inputs
        rt = api.rt_lw_gpoints(ctx, planck, od, nangle=nangle)
        black = restated(None, None)
        scale = np.max([np.abs(a).max(axis=1, keepdims=True) for a in rt], axis=0)
        measured = max(float((np.abs(a - b) / scale).max()) for a, b in zip(black, rt))
        rel = max(cases.OD_BOUND, 10.0 * measured)
        print(f"nangle={nangle} ng={ng}: numpy restatement against rt_lw_gpoints at emissivity 1, worst / largest flux = {measured:.3e};"
              f" bound {rel:.3e}")
        got = fused(ctx, go, f"lw{nangle}", cols, cloud_od=cloud, surface_emissivity=emis, skin_temperature=skin)
        want = restated(emis, planck_skin)
        scale = np.max([np.abs(a).max(axis=1, keepdims=True) for a in want], axis=0)
        for k, w in zip(("dn", "up"), want):
            clear.assert_within(got["spectral_" + k], w, rel * scale * np.ones_like(w), "per-g " + k)
        check_sums(model, cols, got, ["dn", "up"])
        # the atmosphere above does not see the surface: the down fluxes are those of the cloud-only call
        only = fused(ctx, go, f"lw{nangle}", cols, cloud_od=cloud)
        for k in ("dn", "band_dn", "spectral_dn"):
            assert np.array_equal(got[k], only[k]), k
        # a warmer skin raises the upwelling flux at the surface and leaves the downwelling one alone, bit for bit
        warm = fused(ctx, go, f"lw{nangle}", cols, cloud_od=cloud, surface_emissivity=emis, skin_temperature=skin + 5.0)
        assert (warm["spectral_up"][:, nlay] > got["spectral_up"][:, nlay]).all() and (warm["up"][:, nlay] > got["up"][:, nlay]).all()
        for k in ("dn", "band_dn", "spectral_dn"):
            assert np.array_equal(warm[k], got[k]), k
        # each input alone: the skin temperature with emissivity 1, the emissivity with the air's temperature
        for sky, w in ((dict(skin_temperature=skin), restated(None, planck_skin)), (dict(surface_emissivity=emis), restated(emis, None))):
            one = fused(ctx, go, f"lw{nangle}", cols, cloud_od=cloud, **sky)
            for k, wk in zip(("dn", "up"), w):
                clear.assert_within(one["spectral_" + k], wk, rel * scale * np.ones_like(wk), "per-g " + k + " " + next(iter(sky)))
        if nangle == 0:
            mirror = fused(ctx, go, "lw0", cols, cloud_od=cloud, surface_emissivity=np.zeros_like(emis), skin_temperature=skin)
            assert np.array_equal(mirror["spectral_up"][:, nlay], mirror["spectral_dn"][:, nlay])
            assert mirror["spectral_dn"][:, nlay].all()
    finally:
        go.close()


# ---------------------------------------------------------------------------------------------------------- 5 shortwave
def sw_reference(ctx, go, cols, mu0, albedo, cloud, ssa, asym, scale, ib):
    """allsky_ref.two_stream_closed per column on the device's own optical depths -> dict(direct, dn, up) [ncol, nlay+1, ng]"""
    o = device_optics(ctx, go, cols)
    od, ray, inc = o["optical_depth"], o["rayleigh_optical_depth"], go.incoming(TSI)
    ncol = od.shape[0]
    albedo = np.zeros(ncol) if albedo is None else albedo
    res = {k: np.zeros((ncol, od.shape[1] + 1, od.shape[2])) for k in ("direct", "dn", "up")}
    for c in range(ncol):
        if mu0[c] > 0.0:
            d, dn, up = ar.two_stream_closed(od[c], ray[c], cloud[c][:, ib], ssa[c][:, ib], asym[c][:, ib], mu0[c], albedo[c], inc, scale=scale)
            res["direct"][c], res["dn"][c], res["up"][c] = d, d + dn, up
    return res, inc


def check_sw(model, cols, got, want, mu0, inc):
    bound = SW_BOUND * np.maximum(mu0, 0.0)[:, None, None] * inc[None, None, :] * np.ones_like(want["dn"])
    for k in ("direct", "dn", "up"):
        clear.assert_within(got["spectral_" + k], want[k], bound, "per-g " + k)
    check_sums(model, cols, got, ["dn", "up", "direct"])


def sw_case(ctx, go, model, cols, scale, seed=1, dark=(), layout=True):
    ncol, nlay = cols["pressure_hl"].shape[0], cols["pressure_hl"].shape[1] - 1
    mu0, albedo = clear.sun(ncol)
    mu0 = mu0.copy()
    mu0[list(dark)] = [0.0, -0.2][:len(dark)]
    cloud = clouds(model, ncol, nlay, seed=seed, lo=1e-3, hi=50.0, layout=True if layout else None)
    ssa, asym = scatterers(model, ncol, nlay, seed=seed + 1, amax=0.9 if scale else 0.45)
    got = fused(ctx, go, "sw_twostream", cols, mu0, albedo, cloud_od=cloud, cloud_ssa=ssa, cloud_asymmetry=asym, delta_eddington=scale)
    want, inc = sw_reference(ctx, go, cols, mu0, albedo, cloud, ssa, asym, scale, np.asarray(model["iband_per_g"]))
    check_sw(model, cols, got, want, mu0, inc)
    return got, (mu0, albedo, cloud, ssa, asym)


@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("ng,nt,np_,nconc,nlay", SHAPES)
def test_shortwave_clouds_against_the_closed_form(ctx, api, ng, nt, np_, nconc, nlay, scale):
    """per column c % 4: clouds in every layer, in none, in the top layer only, in the bottom layer only"""
    model = make_model("sw", nband=1 if ng in (16, 65) else 3, ng=ng, nt=nt, np_=np_, nconc=nconc)
    go = api.GasOptics(ctx, model)
    try:
        cols = cases.edge_columns(model, nlay=nlay)
        got, (mu0, albedo, *_) = sw_case(ctx, go, model, cols, scale)
        plain = fused(ctx, go, "sw_twostream", cols, mu0, albedo)
        for k in ("spectral_dn", "spectral_up", "spectral_direct"):     # the column without a cloud is the clear column, the others are not
            scale = np.max([np.abs(plain["spectral_" + q][1]).max(axis=0) for q in ("dn", "up")], axis=0)
            clear.assert_within(got[k][1], plain[k][1], cases.OD_BOUND * scale * np.ones_like(plain[k][1]), "cloudless column " + k)
        assert not np.array_equal(got["spectral_up"][0], plain["spectral_up"][0])
    finally:
        go.close()


@pytest.mark.parametrize("columns", [-1, 0, 1])
def test_shortwave_clouds_at_the_group_edges_and_without_sun(ctx, sw33, columns):
    model, go = sw33
    cpb = go.fluxes_geometry(9, mode=2)["columns_per_block"]
    assert cpb == 7
    ncol = cpb + columns
    cols = cases.many_columns(model, ncol, 9)
    lit, (mu0, albedo, cloud, ssa, asym) = sw_case(ctx, go, model, cols, True, seed=3, layout=False)
    dark, (dark_mu0, *_) = sw_case(ctx, go, model, cols, True, seed=3, dark=(2, 5), layout=False)
    keep = [c for c in range(ncol) if c not in (2, 5)]
    for k in lit:
        assert not dark[k][[2, 5]].any() and lit[k][[2, 5]].any(), k
        assert np.array_equal(dark[k][keep], lit[k][keep]), k


def test_shortwave_layers_inside_the_resonance_window(ctx, api):
    """ng = 1, one layer, one column per (ssa, gg): mu0 = (1 + 3e-5) / k of the column's own mixture"""
    model = make_model("sw", nband=1, ng=1)
    go = api.GasOptics(ctx, model)
    try:
        pairs = [(0.3, 0.2), (0.5, 0.45), (0.6, 0.0), (0.55, 0.3), (0.1, 0.4)]
        ncol = len(pairs)
        cols = cases.many_columns(model, ncol, 1)
        o = device_optics(ctx, go, cols)
        cloud = 3.0 + 20.0 * o["rayleigh_optical_depth"]              # the particulate dominates the scattering: k stays above 1
        ssa = np.array([p[0] for p in pairs]).reshape(ncol, 1, 1)
        asym = np.array([p[1] for p in pairs]).reshape(ncol, 1, 1)
        _, m_ssa, m_gg = ar.mix(o["optical_depth"], o["rayleigh_optical_depth"], cloud, ssa, asym)
        g1, g2 = 2.0 - m_ssa * (1.25 + 0.75 * m_gg), m_ssa * (0.75 - 0.75 * m_gg)
        k = np.sqrt((g1 - g2) * (g1 + g2))[:, 0, 0]
        mu0 = (1.0 + 3e-5) / k
        assert (mu0 <= 1.0).all() and (np.abs(1.0 - k * mu0) < 0.5 * ar.RESONANCE_H).all()
        albedo = np.full(ncol, 0.15)
        got = fused(ctx, go, "sw_twostream", cols, mu0, albedo, cloud_od=cloud, cloud_ssa=ssa, cloud_asymmetry=asym, delta_eddington=False)
        want, inc = sw_reference(ctx, go, cols, mu0, albedo, cloud, ssa, asym, False, np.zeros(1, dtype=int))
        check_sw(model, cols, got, want, mu0, inc)
        assert (got["spectral_dn"][:, 1] > got["spectral_direct"][:, 1]).all()
    finally:
        go.close()


def test_a_thick_bright_cloud_over_a_black_surface(ctx, sw33):
    """od 50, ssa 0.999999, asymmetry 0.85 in one layer, albedo 0"""
    model, go = sw33
    ncol, nlay = 8, 9
    cols = cases.many_columns(model, ncol, nlay)
    mu0, _ = clear.sun(ncol)
    cloud = np.zeros((ncol, nlay, 3))
    cloud[:, 4] = 50.0
    ssa, asym = np.full_like(cloud, 0.999999), np.full_like(cloud, 0.85)
    for scale in (True, False):
        got = fused(ctx, go, "sw_twostream", cols, mu0, None, cloud_od=cloud, cloud_ssa=ssa, cloud_asymmetry=asym, delta_eddington=scale)
        plain = fused(ctx, go, "sw_twostream", cols, mu0, None)
        assert all(np.isfinite(v).all() for v in got.values())
        for pre in ("", "band_", "spectral_"):
            assert (got[pre + "dn"] >= got[pre + "direct"]).all() and (got[pre + "direct"] >= 0.0).all(), pre
        assert (got["up"][:, 0] > plain["up"][:, 0]).all()
        if scale:
            want, inc = sw_reference(ctx, go, cols, mu0, None, cloud, ssa, asym, True, np.asarray(model["iband_per_g"]))
            check_sw(model, cols, got, want, mu0, inc)


# ------------------------------------------------------------------------------------------------------- 6 independence
def sky_inputs(model, kind, ncol, nlay, cols):
    rng = np.random.default_rng(11)
    if kind.startswith("lw"):
        return dict(cloud_od=clouds(model, ncol, nlay, seed=8), surface_emissivity=rng.uniform(0.5, 1.0, (ncol, nbands(model))),
                    skin_temperature=cols["temperature_hl"][:, -1] + rng.uniform(-5.0, 5.0, ncol))
    ssa, asym = scatterers(model, ncol, nlay, seed=9)
    return dict(cloud_od=clouds(model, ncol, nlay, seed=8, lo=1e-3, hi=50.0), cloud_ssa=ssa, cloud_asymmetry=asym)


@pytest.mark.parametrize("kind", ["lw0", "lw4", "sw_twostream"])
def test_bit_identity(ctx, api, lw33, sw33, kind, monkeypatch):
    import torch
    model, go = lw33 if kind.startswith("lw") else sw33
    nlay = 7
    cpb = go.fluxes_geometry(nlay, mode=0 if kind.startswith("lw") else 2)["columns_per_block"]
    ncol = 4 * cpb + 1
    cols = cases.many_columns(model, ncol, nlay)
    mu0, albedo = clear.sun(ncol)
    sky = sky_inputs(model, kind, ncol, nlay, cols)
    pick = lambda idx: (({k: v[idx] for k, v in cols.items()}, mu0[idx], albedo[idx]), {k: v[idx] for k, v in sky.items()})
    c = cpb + 2
    batch = fused(ctx, go, kind, cols, mu0, albedo, **sky)
    (args, s) = pick([c])
    alone = fused(ctx, go, kind, *args, **s)
    (args, s) = pick([0, c, 1])
    moved = fused(ctx, go, kind, *args, **s)
    for k in batch:
        assert np.array_equal(batch[k][c], alone[k][0]), k
        assert np.array_equal(batch[k][c], moved[k][1]), k
    for grid in ("1", "2"):                                       # five groups on one block and on two
        monkeypatch.setenv("ECCKD_GAS_OPTICS_FLUXES_GRID", grid)
        forced = fused(ctx, go, kind, cols, mu0, albedo, **sky)
        monkeypatch.delenv("ECCKD_GAS_OPTICS_FLUXES_GRID")
        for k in batch:
            assert np.array_equal(batch[k], forced[k]), (grid, k)
    fresh = api.GasOptics(ctx, model)
    again = fused(ctx, fresh, kind, cols, mu0, albedo, **sky)
    fresh.close()
    for k in batch:
        assert np.array_equal(batch[k], again[k]), k
    plain = fused(ctx, go, kind, cols, mu0, albedo, everything=False, **sky)
    assert sorted(plain) == sorted(k for k in batch if not k.startswith(("band_", "spectral_")))
    for k in plain:
        assert np.array_equal(plain[k], batch[k]), k
    f32 = fused(ctx, go, kind, cols, mu0, albedo, dtype=torch.float32, **sky)
    for k in batch:
        assert f32[k].dtype == np.float32 and np.array_equal(f32[k], batch[k].astype(np.float32)), k
    # another column's cloud (and surface) is no business of this one
    other = {k: v.copy() for k, v in sky.items()}
    other["cloud_od"][c] = np.where(other["cloud_od"][c] > 0.0, 0.0, 2.5)
    changed = fused(ctx, go, kind, cols, mu0, albedo, **other)
    rest = [i for i in range(ncol) if i != c]
    for k in batch:
        assert np.array_equal(changed[k][rest], batch[k][rest]), k
    assert not np.array_equal(changed["spectral_up"][c], batch["spectral_up"][c])


# ----------------------------------------------------------------------------------------------------------- 7 refusals
def test_refusals(ctx, api):
    """each refusal is code 147 with its own message, nothing is launched, and the handles work afterwards"""
    import torch
    from ecckd_amd import _lib
    lib = ctx.lib
    lw_model, sw_model = make_model("lw", ng=16), make_model("sw", ng=16)
    lw, sw = api.GasOptics(ctx, lw_model), api.GasOptics(ctx, sw_model)
    bare_lw, bare_sw = api.GasOptics(ctx, dict(lw_model, iband_per_g=None)), api.GasOptics(ctx, dict(sw_model, iband_per_g=None))
    no_rayleigh = api.GasOptics(ctx, dict(sw_model, rayleigh_molar_scattering=None))
    cols = cases.columns(lw_model, ncol=2, nlay=7)
    p, T, v = (clear.dev(ctx, cols[k]) for k in ("pressure_hl", "temperature_hl", "vmr_fl"))
    mu0 = clear.dev(ctx, np.array([0.5, 0.7]))
    buf = clear.dev(ctx, np.full((2, 8), np.nan))
    arr = clear.dev(ctx, np.full((2, 7, 3), 0.5))
    flat = clear.dev(ctx, np.full((2, 3), 0.9))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    messages = []

    def sky(delta_eddington=0, **kw):
        s = _lib.FluxSky()
        for k, t in kw.items():
            setattr(s, k, t.data_ptr())
        s.delta_eddington = delta_eddington
        return s

    def raw_lw(s, h=lw, nangle=0, nlay=7, t_=T):
        o = _lib.FluxOutputs()
        o.flux_dn = buf.data_ptr()
        return lambda: lib.ecckd_gas_optics_fluxes_lw_sky_dev(h.handle, nangle, 2, nlay, ptr(p), ptr(t_), None, ptr(v), None, None, 8, C.byref(o),
                                                              None if s is None else C.addressof(s))

    def raw_sw(s, h=sw, mu=mu0, direct=False):
        o = _lib.FluxOutputs()
        o.flux_dn = buf.data_ptr()
        if direct:
            o.flux_dn_direct = buf.data_ptr()
        return lambda: lib.ecckd_gas_optics_fluxes_sw_sky_dev(h.handle, 2, 7, ptr(p), ptr(T), None, ptr(v), None, None, ptr(mu), None, TSI, 8,
                                                              C.byref(o), None if s is None else C.addressof(s))

    def refused(call, *words):
        ctx.synchronize()                                         # (the sound calls before are queued on the context's stream)
        buf.fill_(float("nan"))
        torch.cuda.synchronize()
        with pytest.raises(api.EcckdError) as e:
            api.check(call())
        assert e.value.code == 147, e.value
        for w in words:
            assert w in e.value.message, e.value.message
        messages.append(e.value.message)
        ctx.synchronize()
        assert torch.isnan(buf).all()                             # nothing was launched

    cloud3 = dict(cloud_od=arr, cloud_ssa=arr, cloud_asymmetry=arr)
    try:
        before = lw.fluxes_lw(p, T, v, cloud_od=arr)
        api.check(raw_lw(sky(cloud_od=arr, surface_emissivity=flat, skin_temperature=mu0))())      # the raw calls themselves are sound
        api.check(raw_sw(sky(1, **cloud3), direct=True)())
        api.check(raw_lw(sky(skin_temperature=mu0), h=bare_lw)())                                   # not indexed by band: served
        # a band-indexed input on a model created without iband_per_g
        refused(raw_lw(sky(cloud_od=arr), h=bare_lw), "ecckd_gas_optics_fluxes_lw_sky_dev", "cloud_od", "iband_per_g")
        refused(raw_lw(sky(surface_emissivity=flat), h=bare_lw), "surface_emissivity", "iband_per_g")
        refused(raw_sw(sky(1, **cloud3), h=bare_sw), "ecckd_gas_optics_fluxes_sw_sky_dev", "cloud_od", "iband_per_g")
        # shortwave: the cloud triple is whole or absent
        refused(raw_sw(sky(cloud_od=arr, cloud_asymmetry=arr)), "without sky.cloud_ssa")
        refused(raw_sw(sky(cloud_od=arr, cloud_ssa=arr)), "without sky.cloud_asymmetry")
        refused(raw_sw(sky(cloud_ssa=arr)), "cloud_ssa is given without sky.cloud_od")
        refused(raw_sw(sky(cloud_asymmetry=arr)), "cloud_asymmetry is given without sky.cloud_od")
        # longwave: no scattering
        refused(raw_lw(sky(cloud_od=arr, cloud_ssa=arr)), "cloud_ssa", "shortwave call")
        refused(raw_lw(sky(cloud_od=arr, cloud_asymmetry=arr)), "cloud_asymmetry", "shortwave call")
        refused(raw_lw(sky(1, cloud_od=arr)), "delta_eddington = 1", "shortwave call")
        # shortwave: the surface is the albedo
        refused(raw_sw(sky(1, surface_emissivity=flat, **cloud3)), "surface_emissivity", "longwave call")
        refused(raw_sw(sky(1, skin_temperature=mu0)), "skin_temperature", "longwave call")
        # delta_eddington outside {0, 1}, with and without pointers
        refused(raw_sw(sky(2, **cloud3)), "delta_eddington must be 0 or 1, not 2")
        refused(raw_sw(sky(-1)), "delta_eddington must be 0 or 1, not -1")
        refused(raw_lw(sky(3)), "ecckd_gas_optics_fluxes_lw_sky_dev", "not 3")
        # the wrong kind of handle, and what the clear calls refuse, under the sky entries' names
        refused(raw_lw(sky(cloud_od=arr), h=sw), "ecckd_gas_optics_fluxes_lw_sky_dev", "shortwave model")
        refused(raw_sw(sky(1, **cloud3), h=lw), "ecckd_gas_optics_fluxes_sw_sky_dev", "longwave model")
        refused(raw_sw(sky(1, **cloud3), h=no_rayleigh), "Rayleigh coefficients")
        refused(raw_lw(sky(cloud_od=arr), nangle=17), "nangle = 17")
        refused(raw_lw(sky(cloud_od=arr), nlay=0), "positive")
        refused(raw_lw(None, t_=None), "ecckd_gas_optics_fluxes_lw_sky_dev", "d_temperature_hl")
        refused(raw_sw(sky(1, **cloud3), mu=None), "d_cos_sza")
        assert len(set(messages)) == len(messages)
        # the method: clouds without scattering
        with pytest.raises(api.EcckdError) as e:
            sw.fluxes_sw(p, T, v, mu0, cloud_od=arr, cloud_ssa=arr, cloud_asymmetry=arr)
        assert e.value.code == 147 and "scattering=True" in e.value.message
        with pytest.raises(api.EcckdError) as e:
            sw.fluxes_sw(p, T, v, mu0, scattering=True, cloud_od=arr)
        assert e.value.code == 147 and "cloud_ssa" in e.value.message
        with pytest.raises(api.EcckdError) as e:
            lw.fluxes_lw(p, T, v, cloud_od=flat)
        assert e.value.code == 147 and "cloud_od" in e.value.message and "shape" in e.value.message
        after = lw.fluxes_lw(p, T, v, cloud_od=arr)
        assert all(torch.equal(before[k], after[k]) for k in before)
        assert sw.fluxes_sw(p, T, v, mu0, scattering=True, **cloud3)["flux_up_sw"].isfinite().all()
    finally:
        for h in (lw, sw, bare_lw, bare_sw, no_rayleigh):
            h.close()
