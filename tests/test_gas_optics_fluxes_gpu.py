"""The fused fluxes of the resident gas-optics handle (api.GasOptics.fluxes_lw / fluxes_sw, ecckd_gas_optics_fluxes_*) against
the composition of the calls they fuse, evaluated on the same inputs: GasOptics.optical_depth, planck and incoming, then
api.rt_lw_gpoints / rt_sw_gpoints / rt_sw_gpoints_rayleigh (column by column where cos_sza or albedo differ), then numpy sums.
Per g point |fused - composed| <= 1e-12 * scale, rtol 0, with scale the largest composed flux of that (column, g) over levels
and directions: the optical depths and Planck values that enter the recurrences are bit-identical by construction (one source
text, no contraction), so only contraction inside the recurrences separates the two, and 1e-12 is the project's termwise bound
(cases.OD_BOUND).  Sums over g: that bound summed over the g points plus (ng - 1) * 2^-53 * sum_g |flux_g| for the order of
summation.  Heating rates: the formula in numpy on the call's own float64 broadband fluxes, within
8 * 2^-53 * |conv| * (|dn[l+1]| + |dn[l]| + |up[l+1]| + |up[l]|)."""
import ctypes as C

import numpy as np
import pytest

import gas_optics_cases as cases

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CONV = 9.80665 / 1004.0
KINDS = ["lw0", "lw1", "lw4", "sw_direct", "sw_twostream"]
TSI = 1361.0


@pytest.fixture(scope="module")
def api():
    from ecckd_amd import api
    return api


def dev(ctx, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=ctx.device)


def sun(ncol):
    """per-column cos_sza in (0, 1] and albedo in [0, 0.6], all different"""
    c = np.arange(ncol)
    return 0.15 + 0.85 * ((c * 7) % 11) / 10.0, 0.6 * ((c * 5) % 7) / 6.0


def make_model(kind, **kw):
    return (cases.model_lw if kind.startswith("lw") else cases.model_sw)(**kw)


def fused(ctx, go, kind, cols, mu0=None, albedo=None, **kw):
    """the fused call -> dict(dn, up[, direct], hr, band_*, spectral_*) of numpy arrays"""
    p, T, v = (dev(ctx, cols[k]) for k in ("pressure_hl", "temperature_hl", "vmr_fl"))
    if kind.startswith("lw"):
        out = go.fluxes_lw(p, T, v, nangle=int(kind[2:]), **kw)
        names = {"flux_dn_lw": "dn", "flux_up_lw": "up", "heating_rate_lw": "hr"}
    else:
        two = kind == "sw_twostream"
        out = go.fluxes_sw(p, T, v, dev(ctx, mu0), None if albedo is None else dev(ctx, albedo), tsi=TSI, scattering=two, **kw)
        names = {"flux_dn_sw": "dn", "flux_up_sw": "up", "flux_dn_direct_sw": "direct", "heating_rate_sw": "hr"} if two else \
                {"flux_dn_direct_sw": "dn", "flux_up_sw": "up", "heating_rate_sw": "hr"}
    res = {}
    for k, t in out.items():
        pre = "band_" if k.startswith("band_") else ("spectral_" if k.startswith("spectral_") else "")
        res[pre + names[k[len(pre):]]] = t.cpu().numpy()
    return res


def composed(ctx, api, go, kind, cols, mu0=None, albedo=None):
    """the calls that exist without the fused one -> per-g fluxes dict(dn, up[, direct]), each [ncol, nlay+1, ng]"""
    p, T, v = (dev(ctx, cols[k]) for k in ("pressure_hl", "temperature_hl", "vmr_fl"))
    o = go.optical_depth(p, T, v)
    od = o["optical_depth"].cpu().numpy()
    if kind.startswith("lw"):
        dn, up = api.rt_lw_gpoints(ctx, go.planck(T).cpu().numpy(), od, nangle=int(kind[2:]))
        return dict(dn=dn, up=up)
    ray, inc = o["rayleigh_optical_depth"].cpu().numpy(), go.incoming(TSI)[None]
    ncol = od.shape[0]
    albedo = np.zeros(ncol) if albedo is None else albedo
    res = {k: np.zeros((ncol, od.shape[1] + 1, od.shape[2])) for k in (("dn", "up", "direct") if kind == "sw_twostream" else ("dn", "up"))}
    for c in range(ncol):
        if not mu0[c] > 0.0:
            continue
        if kind == "sw_direct":
            res["dn"][c], res["up"][c] = (a[0] for a in api.rt_sw_gpoints(ctx, mu0[c], albedo[c], inc, (od + ray)[c:c + 1]))
        else:
            res["direct"][c], res["dn"][c], res["up"][c] = (a[0] for a in api.rt_sw_gpoints_rayleigh(ctx, mu0[c], albedo[c], inc, od[c:c + 1],
                                                                                                       ray[c:c + 1]))
    return res


def assert_within(got, want, atol, what):
    err = np.abs(got - want)
    print(what, "max error / bound:", (err / np.where(atol > 0, atol, 1.0)).max())
    assert np.isfinite(got).all(), what
    assert (err <= atol).all(), what


def check(model, cols, got, want):
    """per-g fluxes, broadband and band sums, heating rates of a fused call asked for everything"""
    scale = np.max([np.abs(want[k]).max(axis=1, keepdims=True) for k in want], axis=0)            # [ncol, 1, ng]
    ng = scale.shape[-1]
    for k in want:
        assert_within(got["spectral_" + k], want[k], cases.OD_BOUND * scale * np.ones_like(want[k]), "per-g " + k)
        bound = cases.OD_BOUND * scale.sum(-1) + (ng - 1) * EPS * np.abs(want[k]).sum(-1)
        assert_within(got[k], want[k].sum(-1), bound, "broadband " + k)
        if "band_" + k in got:
            ib = np.asarray(model["iband_per_g"])
            for b in range(int(ib.max()) + 1):
                sel = ib == b
                bound = cases.OD_BOUND * scale[..., sel].sum(-1) + (ng - 1) * EPS * np.abs(want[k][..., sel]).sum(-1)
                assert_within(got["band_" + k][..., b], want[k][..., sel].sum(-1), bound, f"band {b} " + k)
    check_heating(cols, got)


def check_heating(cols, got):
    p, dn, up = cols["pressure_hl"], got["dn"], got["up"]
    conv = -CONV / (p[:, 1:] - p[:, :-1])
    want = conv * (dn[:, 1:] - dn[:, :-1] - up[:, 1:] + up[:, :-1])
    bound = 8 * EPS * np.abs(conv) * (np.abs(dn[:, 1:]) + np.abs(dn[:, :-1]) + np.abs(up[:, 1:]) + np.abs(up[:, :-1]))
    assert_within(got["hr"], want, bound, "heating rate")


def run_and_check(ctx, api, go, model, kind, cols, bands=True):
    ncol = cols["pressure_hl"].shape[0]
    mu0, albedo = sun(ncol) if kind.startswith("sw") else (None, None)
    got = fused(ctx, go, kind, cols, mu0, albedo, bands=bands, spectral=True)
    want = composed(ctx, api, go, kind, cols, mu0, albedo)
    check(model, cols, got, want)
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ng,nt,np_,nconc,nlay", cases.SHAPES)
def test_against_the_composed_calls(ctx, api, ng, nt, np_, nconc, nlay, kind):
    """ng 1 / 16 / 33 / 64 / 65, nlay 1 / 7 / 9, both ends of every table axis"""
    model = make_model(kind, ng=ng, nt=nt, np_=np_, nconc=nconc)
    cols = cases.edge_columns(model, nlay=nlay)
    go = api.GasOptics(ctx, model)
    try:
        got = run_and_check(ctx, api, go, model, kind, cols)
        assert got["dn"].any() and got["up"].any() and got["hr"].any()
    finally:
        go.close()


@pytest.mark.parametrize("kind", ["lw0", "sw_direct", "sw_twostream"])
def test_negative_tables_are_clamped_before_the_transfer(ctx, api, kind):
    model = cases.negative_model(make_model(kind, ng=16))
    cols = cases.columns(model, ncol=3, nlay=9)
    go = api.GasOptics(ctx, model)
    try:
        p, T, v = (dev(ctx, cols[k]) for k in ("pressure_hl", "temperature_hl", "vmr_fl"))
        assert (go.optical_depth(p, T, v, keep_negative=True)["optical_depth"] < 0).any()
        run_and_check(ctx, api, go, model, kind, cols)
    finally:
        go.close()


@pytest.fixture(scope="module")
def lw33(ctx, api):
    model = cases.model_lw(ng=33)
    go = api.GasOptics(ctx, model)
    yield model, go
    go.close()


@pytest.fixture(scope="module")
def sw33(ctx, api):
    model = cases.model_sw(ng=33)
    go = api.GasOptics(ctx, model)
    yield model, go
    go.close()


@pytest.mark.parametrize("kind", ["lw4", "sw_direct", "sw_twostream"])
@pytest.mark.parametrize("columns,layers", [(-1, 0), (0, 0), (1, 0), (None, 0), (1, -1), (1, 1)])
def test_group_and_tile_edges(ctx, api, lw33, sw33, kind, columns, layers):
    """ncol at columns_per_block - 1, at it, one past it and at two groups plus one; nlay at layer_tile - 1, at it and one past"""
    model, go = lw33 if kind.startswith("lw") else sw33
    geo = go.fluxes_geometry(9, mode=KINDS.index(kind) - 2 if kind.startswith("sw") else 0)
    cpb, tile = geo["columns_per_block"], geo["layer_tile"]
    assert (cpb, tile, geo["threads"]) == (7, 9, 256)
    ncol = 2 * cpb + 1 if columns is None else cpb + columns
    cols = cases.many_columns(model, ncol, tile + layers)
    run_and_check(ctx, api, go, model, kind, cols)


@pytest.mark.parametrize("kind", ["lw1", "sw_twostream"])
def test_a_block_loops_over_g(ctx, api, kind):
    """ng = 257: one column per block, two passes over g, the second with one live thread"""
    model = make_model(kind, ng=257, nt=2, np_=2, nconc=2)
    go = api.GasOptics(ctx, model)
    try:
        assert go.fluxes_geometry(7)["columns_per_block"] == 1
        run_and_check(ctx, api, go, model, kind, cases.many_columns(model, 3, 7))
    finally:
        go.close()


@pytest.mark.parametrize("kind", ["lw0", "sw_twostream"])
def test_forced_grids_walk_several_groups(ctx, api, lw33, sw33, kind, monkeypatch):
    """ECCKD_GAS_OPTICS_FLUXES_GRID = 1 and 2 with 4 * columns_per_block + 1 columns: five groups on one and on two blocks"""
    model, go = lw33 if kind.startswith("lw") else sw33
    cpb = go.fluxes_geometry(7)["columns_per_block"]
    cols = cases.many_columns(model, 4 * cpb + 1, 7)
    mu0, albedo = sun(4 * cpb + 1)
    free = fused(ctx, go, kind, cols, mu0, albedo, bands=True, spectral=True)
    for grid in ("1", "2"):
        monkeypatch.setenv("ECCKD_GAS_OPTICS_FLUXES_GRID", grid)
        forced = fused(ctx, go, kind, cols, mu0, albedo, bands=True, spectral=True)
        monkeypatch.delenv("ECCKD_GAS_OPTICS_FLUXES_GRID")
        for k in free:
            assert np.array_equal(free[k], forced[k]), (grid, k)
    check(model, cols, free, composed(ctx, api, go, kind, cols, mu0, albedo))


@pytest.mark.parametrize("kind", ["lw4", "sw_direct", "sw_twostream"])
def test_bit_identity(ctx, api, lw33, sw33, kind):
    import torch
    model, go = lw33 if kind.startswith("lw") else sw33
    cpb = go.fluxes_geometry(7)["columns_per_block"]
    ncol = 3 * cpb + 2
    cols = cases.many_columns(model, ncol, 7)
    mu0, albedo = sun(ncol)
    pick = lambda idx: ({k: v[idx] for k, v in cols.items()}, mu0[idx], albedo[idx])
    c = cpb + 2
    everything = dict(bands=True, spectral=True)
    batch = fused(ctx, go, kind, cols, mu0, albedo, **everything)
    alone = fused(ctx, go, kind, *pick([c]), **everything)
    moved = fused(ctx, go, kind, *pick([0, c, 1]), **everything)
    for k in batch:
        assert np.array_equal(batch[k][c], alone[k][0]), k
        assert np.array_equal(batch[k][c], moved[k][1]), k
    fresh = api.GasOptics(ctx, model)
    again = fused(ctx, fresh, kind, cols, mu0, albedo, **everything)
    fresh.close()
    for k in batch:
        assert np.array_equal(batch[k], again[k]), k
    # the broadband outputs do not depend on what else is asked for
    plain = fused(ctx, go, kind, cols, mu0, albedo)
    assert sorted(plain) == sorted(k for k in batch if not k.startswith(("band_", "spectral_")))
    for k in plain:
        assert np.array_equal(plain[k], batch[k]), k
    no_hr = fused(ctx, go, kind, cols, mu0, albedo, heating_rate=False)
    assert "hr" not in no_hr and all(np.array_equal(no_hr[k], batch[k]) for k in no_hr)
    # float32 is the double result rounded once
    f32 = fused(ctx, go, kind, cols, mu0, albedo, dtype=torch.float32, **everything)
    for k in batch:
        assert f32[k].dtype == np.float32 and np.array_equal(f32[k], batch[k].astype(np.float32)), k


@pytest.mark.parametrize("kind", ["sw_direct", "sw_twostream"])
def test_columns_without_sun_and_the_default_albedo(ctx, api, sw33, kind):
    model, go = sw33
    ncol = 9
    cols = cases.many_columns(model, ncol, 7)
    mu0, albedo = sun(ncol)
    lit = fused(ctx, go, kind, cols, mu0, albedo, bands=True, spectral=True)
    dark_mu0 = mu0.copy()
    dark_mu0[[2, 6]] = [0.0, -0.2]
    dark = fused(ctx, go, kind, cols, dark_mu0, albedo, bands=True, spectral=True)
    for k in lit:
        assert np.isfinite(dark[k]).all() and not dark[k][[2, 6]].any(), k
        assert lit[k][[2, 6]].any(), k
        keep = [c for c in range(ncol) if c not in (2, 6)]
        assert np.array_equal(dark[k][keep], lit[k][keep]), k
    check(model, cols, dark, composed(ctx, api, go, kind, cols, dark_mu0, albedo))
    none = fused(ctx, go, kind, cols, mu0, None, bands=True, spectral=True)
    zeros = fused(ctx, go, kind, cols, mu0, np.zeros(ncol), bands=True, spectral=True)
    for k in none:
        assert np.array_equal(none[k], zeros[k]), k
    assert not np.array_equal(none["up"], lit["up"])


@pytest.mark.parametrize("kind", ["lw0", "sw_direct"])
def test_a_model_without_iband_per_g(ctx, api, kind):
    model = make_model(kind, ng=16)
    cols = cases.columns(model, ncol=3, nlay=7)
    bare = api.GasOptics(ctx, dict(model, iband_per_g=None))
    try:
        with pytest.raises(api.EcckdError) as e:
            fused(ctx, bare, kind, cols, *sun(3), bands=True)
        assert e.value.code == 147 and "iband_per_g" in e.value.message
        run_and_check(ctx, api, bare, model, kind, cols, bands=False)
    finally:
        bare.close()


def test_refusals(ctx, api):
    """each refusal is code 147 with its own message, and the handle works afterwards"""
    from ecckd_amd import _lib
    lib = ctx.lib
    lw_model, sw_model = cases.model_lw(ng=16), cases.model_sw(ng=16)
    lw, sw = api.GasOptics(ctx, lw_model), api.GasOptics(ctx, sw_model)
    bare_sw = api.GasOptics(ctx, dict(sw_model, rayleigh_molar_scattering=None))
    cols = cases.columns(lw_model, ncol=2, nlay=7)
    p, T, v = (dev(ctx, cols[k]) for k in ("pressure_hl", "temperature_hl", "vmr_fl"))
    mu0 = dev(ctx, np.array([0.5, 0.7]))
    buf = dev(ctx, np.zeros((2, 8)))
    before = lw.fluxes_lw(p, T, v)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    messages = []

    def outputs(**kw):
        o = _lib.FluxOutputs()
        for k, t in kw.items():
            setattr(o, k, t.data_ptr())
        return o

    def refused(call, *words):
        with pytest.raises(api.EcckdError) as e:
            api.check(call())
        assert e.value.code == 147, e.value
        for w in words:
            assert w in e.value.message, e.value.message
        messages.append(e.value.message)

    def raw_lw(h=lw, nangle=0, ncol=2, nlay=7, p_=p, t_=T, v_=v, out_type=8, o=None, null_out=False):
        o = outputs(flux_dn=buf) if o is None else o
        return lambda: lib.ecckd_gas_optics_fluxes_lw_dev(h.handle, nangle, ncol, nlay, ptr(p_), ptr(t_), None, ptr(v_), None, None, out_type,
                                                          None if null_out else C.byref(o))

    def raw_sw(h=sw, scattering=0, ncol=2, nlay=7, p_=p, mu=mu0, out_type=8, o=None):
        o = outputs(flux_dn=buf) if o is None else o
        return lambda: lib.ecckd_gas_optics_fluxes_sw_dev(h.handle, scattering, ncol, nlay, ptr(p_), ptr(T), None, ptr(v), None, None, ptr(mu),
                                                          None, TSI, out_type, C.byref(o))

    try:
        api.check(raw_lw()())                                      # the raw calls themselves are sound
        api.check(raw_sw()())
        api.check(raw_sw(scattering=1, o=outputs(flux_dn=buf, flux_dn_direct=buf))())
        refused(raw_lw(h=sw), "ecckd_gas_optics_fluxes_lw_dev", "shortwave")
        refused(raw_sw(h=lw), "ecckd_gas_optics_fluxes_sw_dev", "longwave")
        refused(raw_lw(nangle=17), "nangle")
        refused(raw_lw(nangle=-1), "nangle = -1")
        refused(raw_sw(scattering=2), "scattering must be")
        refused(raw_sw(h=bare_sw, scattering=1), "Rayleigh coefficients")
        refused(raw_sw(o=outputs(flux_dn=buf, flux_dn_direct=buf)), "_direct", "scattering = 0")
        refused(raw_lw(o=outputs(flux_dn=buf, spectral_flux_dn_direct=buf)), "_direct", "longwave")
        refused(raw_lw(o=outputs()), "no output")
        refused(raw_lw(null_out=True), "output structure")
        refused(raw_lw(p_=None), "d_pressure_hl")
        refused(raw_lw(t_=None), "ecckd_gas_optics_fluxes_lw_dev", "d_temperature_hl")
        refused(raw_sw(mu=None), "d_cos_sza")
        refused(raw_lw(v_=None), "d_vmr_fl", "gas 1")
        refused(raw_lw(out_type=2), "out_type")
        refused(raw_sw(out_type=0), "ecckd_gas_optics_fluxes_sw_dev", "out_type")
        refused(raw_lw(nlay=0), "positive")                        # a shape the plan refuses
        refused(raw_sw(ncol=-3), "positive", "ncol=-3")
        assert len(set(messages)) == len(messages)
        import torch
        after = lw.fluxes_lw(p, T, v)
        assert all(torch.equal(before[k], after[k]) for k in before)
    finally:
        for h in (lw, sw, bare_sw):
            h.close()
