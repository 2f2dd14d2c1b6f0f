"""The resident gas-optics handle (api.GasOptics, ecckd_gas_optics_*) on the device against the numpy restatement of its
formula (gas_optics_ref.py, pinned to the oracle by test_gas_optics_ref.py) and against api.run_ckd, with the bounds of
test_run_ckd_gpu.py: optical depth 1e-12 termwise (atol = 1e-12 * sum_i |od_i| over the gases' unclamped contributions,
rtol = 0), Planck rtol 1e-14.  Host and device log may differ by an ulp (1.8e-15 of ln 1e5), which moves an interpolation
weight by under 1e-14 on the grids of synthetic.ckd_model, whose neighbouring nodes differ by well under a factor of 10."""
import ctypes as C

import numpy as np
import pytest

import gas_optics_cases as cases
import gas_optics_ref as ref

pytestmark = pytest.mark.gpu


def dev(ctx, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=ctx.device)


def apply(ctx, go, cols, **kw):
    """optical_depth on device copies of the columns -> dict of numpy arrays"""
    vmr = kw.pop("vmr_fl", cols["vmr_fl"])
    out = go.optical_depth(dev(ctx, cols["pressure_hl"]), dev(ctx, cols["temperature_hl"]), None if vmr is None else dev(ctx, vmr), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def expected(model, cols, present=None, scaling=None):
    return ref.gas_optical_depths(model, cols["pressure_hl"], cols["temperature_hl"], cols["vmr_fl"], present=present, scaling=scaling)


def assert_within(got, want, atol, what):
    err = np.abs(got - want)
    print(what, "max error / bound:", (err / np.where(atol > 0, atol, 1.0)).max())
    assert np.isfinite(got).all(), what
    assert (err <= atol).all(), what


@pytest.fixture(scope="module")
def api():
    from ecckd_amd import api
    return api


@pytest.fixture(scope="module")
def lw16(ctx, api):
    """one longwave model and its handle for the tests that need no particular shape"""
    model = cases.model_lw(ng=16)
    go = api.GasOptics(ctx, model)
    yield model, go
    go.close()


@pytest.mark.parametrize("sw", [False, True])
@pytest.mark.parametrize("ng,nt,np_,nconc,nlay", cases.SHAPES)
def test_against_restatement_and_run_ckd(ctx, api, ng, nt, np_, nconc, nlay, sw):
    """every ng, both ends of nconc / np_ / nt, nlay 1 / 7 / 9, columns held inside the table at both ends of every axis"""
    model = (cases.model_sw if sw else cases.model_lw)(ng=ng, nt=nt, np_=np_, nconc=nconc)
    cols = cases.edge_columns(model, nlay=nlay)
    names = [g["name"] for g in model["gases"]]
    go = api.GasOptics(ctx, model)
    try:
        assert (go.ng, go.ngas, go.is_sw, go.entries_per_cell) == (ng, 5, sw, 24)
        out = apply(ctx, go, cols, per_gas=True)
        parts = expected(model, cols)
        atol = cases.od_atol(parts)
        assert_within(out["optical_depth"], np.maximum(parts.sum(0), 0.0), atol, "total")
        for i, n in enumerate(names):
            assert_within(out[n + "_optical_depth"], np.maximum(parts[i], 0.0), atol, n)
        scene = dict(cols, mu0=np.full(4, 0.5), tsi=1361.0) if sw else cols
        old = api.run_ckd(ctx, model, scene)
        assert_within(out["optical_depth"], old["optical_depth"], atol, "total against run_ckd")
        for n in names:
            assert_within(out[n + "_optical_depth"], old[n + "_optical_depth"], atol, n + " against run_ckd")
        if sw:
            assert np.allclose(out["rayleigh_optical_depth"], ref.rayleigh_optical_depth(model, cols["pressure_hl"]), rtol=1e-15, atol=0.0)
            assert np.array_equal(out["rayleigh_optical_depth"], old["rayleigh_optical_depth"])
            assert np.allclose(go.incoming(1361.0), ref.incoming(model, 1361.0), rtol=1e-15, atol=0.0)
            assert np.array_equal(go.incoming(1361.0), old["incoming_sw"][0])
        else:
            assert "rayleigh_optical_depth" not in out
    finally:
        go.close()


def test_shortwave_model_without_rayleigh_coefficients(ctx, api):
    model = dict(cases.model_sw(ng=16), rayleigh_molar_scattering=None)
    cols = cases.columns(model, ncol=2, nlay=7)
    go = api.GasOptics(ctx, model)
    out = apply(ctx, go, cols)
    go.close()
    assert not out["rayleigh_optical_depth"].any()
    assert_within(out["optical_depth"], np.maximum(expected(model, cols).sum(0), 0.0), cases.od_atol(expected(model, cols)), "total")


@pytest.mark.parametrize("nlay,offset", [(7, -1), (9, -1), (1, 0), (1, 1), (1, None)])
def test_tile_edges(ctx, api, nlay, offset):
    """ncol * nlay at cells_per_block - 1 (as 9 x 7 and 7 x 9), cells_per_block, + 1, and two tiles plus one"""
    model = cases.model_lw(ng=33)
    go = api.GasOptics(ctx, model)
    geo = go.geometry()
    cpb = geo["cells_per_block"]
    assert cpb > 0 and geo["threads"] % 64 == 0
    ncell = 2 * cpb + 1 if offset is None else cpb + offset
    assert ncell % nlay == 0, "the tile no longer divides as this test assumes: choose other nlay"
    cols = cases.many_columns(model, ncell // nlay, nlay)
    out = apply(ctx, go, cols, per_gas=True)
    go.close()
    parts = expected(model, cols)
    atol = cases.od_atol(parts)
    assert_within(out["optical_depth"], np.maximum(parts.sum(0), 0.0), atol, "total")
    for i, g in enumerate(model["gases"]):
        assert_within(out[g["name"] + "_optical_depth"], np.maximum(parts[i], 0.0), atol, g["name"])


def test_bit_identity(ctx, api, lw16):
    import torch
    model, go = lw16
    cpb = go.geometry()["cells_per_block"]
    nlay = 7
    ncol = 3 * cpb // nlay + 3                                     # more than three tiles
    cols = cases.many_columns(model, ncol, nlay)
    c = (cpb + nlay - 1) // nlay                                   # a column near the first tile edge ...
    while not (c * nlay < 2 * cpb <= (c + 1) * nlay - 1 or c * nlay < cpb <= (c + 1) * nlay - 1):
        c += 1                                                     # ... whose layers lie on both sides of one
    pick = lambda idx: {k: v[idx] for k, v in cols.items()}
    batch = apply(ctx, go, cols, per_gas=True)
    alone = apply(ctx, go, pick([c]), per_gas=True)
    last = apply(ctx, go, pick([0, 1, c]), per_gas=True)
    for k in batch:
        assert np.array_equal(batch[k][c], alone[k][0]), k
        assert np.array_equal(batch[k][c], last[k][2]), k
    # a fresh handle against one that has served other shapes
    fresh = api.GasOptics(ctx, model)
    again = apply(ctx, fresh, cols, per_gas=True)
    fresh.close()
    for k in batch:
        assert np.array_equal(batch[k], again[k]), k
    # a per-gas output against the total of a call with that gas alone present
    for i, g in enumerate(model["gases"]):
        only = apply(ctx, go, cols, gases=[i])
        assert np.array_equal(only["optical_depth"], batch[g["name"] + "_optical_depth"]), g["name"]
    # float32 is the double result rounded once
    f32 = apply(ctx, go, cols, per_gas=True, dtype=torch.float32)
    for k in batch:
        assert f32[k].dtype == np.float32 and np.array_equal(f32[k], batch[k].astype(np.float32)), k


def test_negative_tables_and_the_clamp(ctx, api):
    model = cases.negative_model(cases.model_lw(ng=16))
    cols = cases.columns(model, ncol=3, nlay=9)
    go = api.GasOptics(ctx, model)
    kept = apply(ctx, go, cols, per_gas=True, keep_negative=True)
    clamped = apply(ctx, go, cols, per_gas=True, keep_negative=False)
    go.close()
    parts = expected(model, cols)
    atol = cases.od_atol(parts)
    names = [g["name"] + "_optical_depth" for g in model["gases"]]
    assert (kept["optical_depth"] < 0).any() and (kept["optical_depth"] > 0).any()
    assert (kept["co2_optical_depth"] < 0).any() and (kept["ch4_optical_depth"] < 0).any()
    assert_within(kept["optical_depth"], parts.sum(0), atol, "unclamped total")
    for i, n in enumerate(names):
        assert_within(kept[n], parts[i], atol, "unclamped " + n)
    # keep_negative = 0: the SUM is clamped, and each per-gas output on its own
    for k in kept:
        assert np.array_equal(clamped[k], np.maximum(kept[k], 0.0)), k
    # keep_negative = 1: the per-gas outputs add up to the total
    total = sum(kept[n] for n in names)
    bound = 4 * 2.0 ** -52 * sum(np.abs(kept[n]) for n in names)
    assert (np.abs(total - kept["optical_depth"]) <= bound).all()


def test_gas_list_and_scalings_against_run_ckd(ctx, api, lw16):
    model, go = lw16
    cols = cases.columns(model, ncol=3, nlay=9)
    out = apply(ctx, go, cols, gases=["h2o", "co2"], scalings={2: 4.0}, per_gas=True)
    old = api.run_ckd(ctx, model, cols, gases=["h2o", "co2"], scalings={2: 4.0})
    parts = expected(model, cols, present=[0, 1, 1, 0, 0], scaling=[1.0, 1.0, 4.0, 1.0, 1.0])
    atol = cases.od_atol(parts)
    assert sorted(out) == sorted(k for k in old if k.endswith("optical_depth"))
    for k in out:
        assert_within(out[k], old[k], atol, k + " against run_ckd")
    assert_within(out["optical_depth"], np.maximum(parts.sum(0), 0.0), atol, "total")
    # the gas list by index; a gas without concentration dependence needs no mole fractions, and is skipped when absent
    alone = apply(ctx, go, cols, gases=[0], vmr_fl=None)
    assert_within(alone["optical_depth"], np.maximum(expected(model, cols, present=[1, 0, 0, 0, 0])[0], 0.0), atol, "composite alone")
    assert not apply(ctx, go, cols, gases=[])["optical_depth"].any()


def test_device_tensors_in_and_out(ctx, api, lw16):
    import torch
    model, go = lw16
    cols = cases.columns(model, ncol=3, nlay=7)
    p, T, v = (dev(ctx, cols[k]) for k in ("pressure_hl", "temperature_hl", "vmr_fl"))
    out = go.optical_depth(p, T, v, per_gas=True)
    for k, t in out.items():
        assert t.is_cuda and t.device == ctx.device and t.dtype == torch.float64 and t.shape == (3, 7, 16) and t.data_ptr() != 0, k
    # the inputs are used where they lie: a non-owning view into a larger buffer gives the same results
    big = torch.full((p.numel() + 5,), float("nan"), dtype=torch.float64, device=ctx.device)
    big[5:] = p.reshape(-1)
    view = big[5:].view(p.shape)
    assert view.data_ptr() == big.data_ptr() + 40
    again = go.optical_depth(view, T, v, per_gas=True)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    # the caller's own full-level temperature replaces the pressure-weighted mean
    t_fl = (T[:, :-1] * p[:, :-1] + T[:, 1:] * p[:, 1:]) / (p[:, :-1] + p[:, 1:])
    warm = go.optical_depth(p, T, v, temperature_fl=t_fl + 1.0)["optical_depth"].cpu().numpy()
    parts = ref.gas_optical_depths(model, cols["pressure_hl"], cols["temperature_hl"], cols["vmr_fl"], temperature_fl=t_fl.cpu().numpy() + 1.0)
    assert_within(warm, np.maximum(parts.sum(0), 0.0), cases.od_atol(parts), "temperature_fl")
    assert not np.array_equal(warm, out["optical_depth"].cpu().numpy())
    # a tensor that would have to be copied is refused
    with pytest.raises(api.EcckdError):
        go.optical_depth(p.float(), T, v)
    with pytest.raises(api.EcckdError):
        go.optical_depth(p.cpu(), T, v)


def test_planck(ctx, api, lw16):
    import torch
    model, go = lw16
    tpl = model["temperature_planck"]
    # below the table, on a node, between nodes, in the last interval, on and above the last node
    t = np.array([[tpl[0] - 60.0, tpl[0] - 0.5, tpl[0], tpl[7]], [tpl[7] + 0.25, tpl[-2] + 0.75, tpl[-1], tpl[-1] + 60.0]])
    got = go.planck(dev(ctx, t))
    assert got.is_cuda and got.shape == (2, 4, 16)
    want = ref.planck(model, t)
    assert np.allclose(got.cpu().numpy(), want, rtol=cases.PLANCK_RTOL, atol=0.0)
    assert np.array_equal(got[0, 3].cpu().numpy(), model["planck_function"][7])
    assert torch.equal(go.planck(dev(ctx, t), dtype=torch.float32), got.float())
    # against run_ckd's planck_hl
    cols = cases.columns(model, ncol=2, nlay=7)
    old = api.run_ckd(ctx, model, cols, per_gas=False)
    hl = go.planck(dev(ctx, cols["temperature_hl"])).cpu().numpy()
    assert np.allclose(hl, old["planck_hl"], rtol=cases.PLANCK_RTOL, atol=0.0)


def test_refusals(ctx, api, lw16):
    """each refusal is code 147 with its own message, and the handle works afterwards"""
    model, go = lw16
    lib = ctx.lib
    cols = cases.columns(model, ncol=2, nlay=7)
    p, T, v = (dev(ctx, cols[k]) for k in ("pressure_hl", "temperature_hl", "vmr_fl"))
    before = go.optical_depth(p, T, v)["optical_depth"]
    od = before.clone()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    messages = []

    def refused(call, *words):
        with pytest.raises(api.EcckdError) as e:
            call()
        assert e.value.code == 147, e.value
        for w in words:
            assert w in e.value.message, e.value.message
        messages.append(e.value.message)

    def raw(ncol=2, nlay=7, p_=p, t_=T, v_=v, keep=0, out_type=8, od_=od, ray=None, h=None):
        return lambda: api.check(lib.ecckd_gas_optics_dev(h or go.handle, ncol, nlay, ptr(p_) if p_ is not None else None,
                                                          ptr(t_) if t_ is not None else None, None, ptr(v_) if v_ is not None else None,
                                                          None, None, keep, out_type, ptr(od_) if od_ is not None else None, None,
                                                          ptr(ray) if ray is not None else None))

    raw()()                                                        # the raw call itself is sound
    refused(raw(p_=None), "d_pressure_hl")
    refused(raw(ncol=0), "positive")
    refused(raw(nlay=-1), "positive")
    refused(raw(od_=None), "no output")
    refused(raw(ray=od), "d_rayleigh_od", "longwave")
    refused(raw(out_type=2), "out_type")
    refused(raw(keep=2), "keep_negative")
    refused(raw(v_=None), "d_vmr_fl", "gas 1")
    refused(lambda: go.incoming(1361.0), "ecckd_gas_optics_incoming", "longwave")
    refused(lambda: api.GasOptics(ctx, dict(model, logarithmic_interpolation=True)), "ecckd_gas_optics_create", "logarithmic")
    refused(lambda: api.check(lib.ecckd_gas_optics_planck_dev(go.handle, 0, ptr(T), 8, ptr(od))), "ecckd_gas_optics_planck_dev")
    sw = api.GasOptics(ctx, cases.model_sw(ng=16))
    refused(lambda: sw.planck(T), "ecckd_gas_optics_planck_dev", "shortwave")
    assert sw.optical_depth(p, T, v)["optical_depth"].shape == (2, 7, 16)
    sw.close()
    assert len(set(messages)) == len(messages)
    import torch
    assert torch.equal(go.optical_depth(p, T, v)["optical_depth"], before)
