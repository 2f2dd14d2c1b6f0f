"""GPU parity for the band fluxes of many scenarios from one read of the spectra (ecckd_lbl_band_fluxes_lw_scenarios /
_sw_scenarios, csrc/lbl_scenarios.hip).  The reference of every comparison is the single-scenario path, which other tests pin
to the oracle: api.merge_spectrum gas after gas into a DOUBLE matrix (k_merge), then api.lbl_band_fluxes_lw / _sw.  The fused
call is never compared with itself except for the bit-equality properties (identical scenarios, a scenario of a many-scenario
call against the same scenario run alone, an angle of a many-angle call against a one-angle call).

Tolerance.  The merged optical depths are bit-identical by construction; what may differ is the contraction of the recurrence
in a differently shaped kernel: a few roundings per layer, nlay <= 54, on sums of non-negative terms, so a relative difference of
about (3 nlay + 8) 2^-53 = 2e-14.  rtol = 1e-12 leaves a factor of 50; atol = 1e-15 x the largest flux of that scenario.
The tests print whether the match was bitwise (run with -s); DESIGN.md records the result."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NWAV = 1000                                         # not a multiple of 256: the last chunk of a band has dead lanes
# [0, 599] ends in the middle of the chunk 512..767; [600, 639] is narrower than a wave; one band is empty (begin 0, end -1, as
# ecckd_band_ranges reports a band without wavenumbers); the last one runs to the end of the spectrum
BEGIN = np.array([0, 600, 0, 640])
END = np.array([599, 639, -1, NWAV - 1])
GASES = [("float32",), ("float64",), ("float32", "float64", "float32")]
MU5 = np.array([0.1, 0.3, 0.5, 0.7, 0.9])
RTOL = 1e-12


def _spectra(nlay, dtypes, seed):
    """Random positive optical depths with a few strong lines: some levels saturated (tau ~ 1e3), some thin (tau ~ 1e-7)."""
    rs = np.random.RandomState(seed)
    pressure = np.linspace(0.02, 1.0, nlay)[:, None]
    ods = []
    for dt in dtypes:
        od = rs.gamma(0.5, 1.0, (nlay, NWAV)) * 10.0 ** rs.uniform(-7.0, -1.0, NWAV) * pressure
        for centre in rs.randint(0, NWAV, 6):
            od += 10.0 ** rs.uniform(1.0, 3.0) * pressure ** 2 / (1.0 + ((np.arange(NWAV) - centre) / rs.uniform(1.0, 6.0)) ** 2)
        ods.append(od.astype(dt))
    return ods


def _scales(nscen, ngas, nlay, seed):
    """[nscen][ngas][nlay]: 0 as is; 1 the first gas scaled by 0; 2 a profile per layer; 3 the same again; then one factor per gas."""
    rs = np.random.RandomState(seed)
    sc = np.ones((nscen, ngas, nlay))
    for s in range(1, nscen):
        sc[s] = rs.uniform(0.25, 4.0, (ngas, 1))
    if nscen > 3:
        sc[1, 0] = 0.0
        sc[2] = rs.uniform(0.5, 2.0, (ngas, nlay))
        sc[3] = sc[2]
    return sc


def _merged(ctx, d_ods, scale):
    """The parent's merged DOUBLE matrix of one scenario: k_merge gas after gas."""
    from ecckd_amd import api
    m = None
    for g, od in enumerate(d_ods):
        m = api.merge_spectrum(ctx, od, scale[g], merged=m)
    ctx.synchronize()
    return m


def _close(got, want, what):
    """rtol 1e-12, atol 1e-15 x the scenario's largest flux; returns whether the match is bitwise."""
    atol = 1e-15 * float(np.max(np.abs(want))) if want.size else 0.0
    err = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)) if want.size else 0.0
    assert np.allclose(got, want, rtol=RTOL, atol=atol), f"{what}: largest relative difference {err:.3e}"
    return np.array_equal(got, want)


def _lw_inputs(ctx, nlay, dtypes, seed=11):
    from ecckd_amd import synthetic as syn
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)
    p = syn.pressure_grid(nlay)
    wn, dwn = syn.wavenumber_grid(NWAV)
    return syn.temperature_profile(p), dev(wn), dev(dwn), [dev(o) for o in _spectra(nlay, dtypes, seed)]


@pytest.mark.parametrize("nangle", [0, 4])
@pytest.mark.parametrize("dtypes", GASES, ids=lambda d: "+".join(d))
@pytest.mark.parametrize("nlay", [3, 54])
def test_lw_scenarios_against_the_single_scenario_path(ctx, nlay, dtypes, nangle):
    from ecckd_amd import api
    t_hl, wn, dwn, d_ods = _lw_inputs(ctx, nlay, dtypes)
    T = api.lbl_scenarios_slots(False, nlay)
    assert T == min(8, 43008 // (64 * (nlay + 1))) == 8
    nscen = T + 1                                   # one more than a launch carries: two launches (5 + 4 scenarios)
    sc = _scales(nscen, len(dtypes), nlay, seed=3)
    dn, up, sdn, tup = api.lbl_band_fluxes_lw_scenarios(ctx, t_hl, wn, dwn, d_ods, sc, BEGIN, END, boundary=True, nangle=nangle)
    assert dn.shape == up.shape == (nscen, 4, nlay + 1) and tuple(sdn.shape) == tuple(tup.shape) == (nscen, NWAV)
    sdn, tup = sdn.cpu().numpy(), tup.cpu().numpy()
    bitwise = True
    for s in range(nscen):
        m = _merged(ctx, d_ods, sc[s])
        rdn, rup, rsdn, rtup = api.lbl_band_fluxes_lw(ctx, t_hl, wn, dwn, m, BEGIN, END, boundary=True, nangle=nangle)
        bitwise &= _close(dn[s], rdn, f"flux_dn of scenario {s}") & _close(up[s], rup, f"flux_up of scenario {s}")
        bitwise &= _close(sdn[s], rsdn.cpu().numpy(), f"surface spectrum of scenario {s}")
        bitwise &= _close(tup[s], rtup.cpu().numpy(), f"TOA spectrum of scenario {s}")
        # scenario s of the call is the same scenario run alone (nscen = 1), bit for bit: nothing depends on the tile
        adn, aup, asdn, atup = api.lbl_band_fluxes_lw_scenarios(ctx, t_hl, wn, dwn, d_ods, sc[s:s + 1], BEGIN, END, boundary=True,
                                                                nangle=nangle)
        assert np.array_equal(adn[0], dn[s]) and np.array_equal(aup[0], up[s]), s
        assert np.array_equal(asdn.cpu().numpy()[0], sdn[s]) and np.array_equal(atup.cpu().numpy()[0], tup[s]), s
    print(f"\nlw scenarios nlay={nlay} gases={'+'.join(dtypes)} nangle={nangle}: bitwise equal to the single-scenario path: {bitwise}")
    assert np.array_equal(dn[2], dn[3]) and np.array_equal(up[2], up[3])          # the two identical scenarios
    assert np.array_equal(sdn[2], sdn[3]) and np.array_equal(tup[2], tup[3])
    assert np.all(dn[:, 2] == 0) and np.all(up[:, 2] == 0) and np.all(dn[0, 0, 1:] > 0)   # the empty band; a real flux elsewhere
    # the (nscen, ngas) form of the scales is the profile form with one factor per gas
    flat = sc[[0, 4, 5]][:, :, 0]
    dn2, up2 = api.lbl_band_fluxes_lw_scenarios(ctx, t_hl, wn, dwn, d_ods, flat, BEGIN, END, nangle=nangle)
    assert np.array_equal(dn2, dn[[0, 4, 5]]) and np.array_equal(up2, up[[0, 4, 5]])


def _sw_inputs(ctx, nlay, dtypes, seed=17):
    from ecckd_amd import synthetic as syn
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)
    wn, dwn = syn.wavenumber_grid(NWAV, 250.0, 50000.0)
    ssi = syn.solar_spectral_irradiance(wn, dwn)
    albedo = np.where(wn < 12000.0, 0.2, 0.05)
    return dev(ssi), dev(albedo), [dev(o) for o in _spectra(nlay, dtypes, seed)]


@pytest.mark.parametrize("with_albedo", [False, True])
@pytest.mark.parametrize("mu", [np.array([0.6]), MU5], ids=["1angle", "5angles"])
@pytest.mark.parametrize("dtypes", GASES, ids=lambda d: "+".join(d))
@pytest.mark.parametrize("nlay", [3, 54])
def test_sw_scenarios_against_the_single_scenario_path(ctx, nlay, dtypes, mu, with_albedo):
    from ecckd_amd import api
    ssi, albedo, d_ods = _sw_inputs(ctx, nlay, dtypes)
    alb = albedo if with_albedo else None
    T = api.lbl_scenarios_slots(True, nlay)
    assert T == min(16, 59392 // (64 * (nlay + 1))) == 16
    nscen, nsza = T + 1, mu.size                    # 17 slots (2 launches) with one angle, 85 (6 launches of 3 scenarios) with five
    sc = _scales(nscen, len(dtypes), nlay, seed=5)
    dn, up, sdn, tup = api.lbl_band_fluxes_sw_scenarios(ctx, mu, ssi, d_ods, sc, BEGIN, END, albedo=alb, boundary=True)
    assert dn.shape == up.shape == (nscen, nsza, 4, nlay + 1) and tuple(sdn.shape) == tuple(tup.shape) == (nscen, nsza, NWAV)
    sdn, tup = sdn.cpu().numpy(), tup.cpu().numpy()
    bitwise = True
    for s in range(nscen):
        m = _merged(ctx, d_ods, sc[s])
        for a in range(nsza):
            rdn, rup, rsdn, rtup = api.lbl_band_fluxes_sw(ctx, mu[a], ssi, m, BEGIN, END, albedo=alb, boundary=True)
            bitwise &= _close(dn[s, a], rdn, f"flux_dn_direct of scenario {s}, angle {a}") & _close(up[s, a], rup, f"flux_up of scenario {s}, angle {a}")
            bitwise &= _close(sdn[s, a], rsdn.cpu().numpy(), f"surface spectrum of scenario {s}, angle {a}")
            bitwise &= _close(tup[s, a], rtup.cpu().numpy(), f"TOA spectrum of scenario {s}, angle {a}")
        if s < 5 or s == nscen - 1:
            # the scenario alone, and each of its angles alone: the same bits
            adn, aup, asdn, atup = api.lbl_band_fluxes_sw_scenarios(ctx, mu, ssi, d_ods, sc[s:s + 1], BEGIN, END, albedo=alb, boundary=True)
            assert np.array_equal(adn[0], dn[s]) and np.array_equal(aup[0], up[s]), s
            assert np.array_equal(asdn.cpu().numpy()[0], sdn[s]) and np.array_equal(atup.cpu().numpy()[0], tup[s]), s
            for a in range(nsza if nsza > 1 else 0):
                odn, oup = api.lbl_band_fluxes_sw_scenarios(ctx, mu[a], ssi, d_ods, sc[s:s + 1], BEGIN, END, albedo=alb)
                assert np.array_equal(odn[0, 0], dn[s, a]) and np.array_equal(oup[0, 0], up[s, a]), (s, a)
    print(f"\nsw scenarios nlay={nlay} gases={'+'.join(dtypes)} nsza={nsza} albedo={with_albedo}: bitwise equal to the single-scenario path: {bitwise}")
    assert np.array_equal(dn[2], dn[3]) and np.array_equal(up[2], up[3]) and np.array_equal(sdn[2], sdn[3]) and np.array_equal(tup[2], tup[3])
    assert np.all(dn[:, :, 2] == 0) and np.all(up[:, :, 2] == 0) and np.all(dn[0, :, 0] > 0)
    if not with_albedo:
        assert np.all(up == 0.0) and np.all(tup == 0.0)                           # no upwelling sweep: exactly zero


def test_many_layers_split_the_angles_too(ctx):
    """130 layers: a longwave launch holds 5 scenarios, a shortwave one 7 slots - fewer than the 8 angles of one scenario, which
    go over two launches of 4."""
    from ecckd_amd import api
    nlay, dtypes = 130, ("float32", "float64")
    assert api.lbl_scenarios_slots(False, nlay) == 5 and api.lbl_scenarios_slots(True, nlay) == 7
    sc = _scales(6, 2, nlay, seed=9)
    t_hl, wn, dwn, d_ods = _lw_inputs(ctx, nlay, dtypes)
    dn, up = api.lbl_band_fluxes_lw_scenarios(ctx, t_hl, wn, dwn, d_ods, sc, BEGIN, END)
    ssi, albedo, s_ods = _sw_inputs(ctx, nlay, dtypes)
    mu = np.linspace(0.15, 0.85, 8)
    sdn, sup = api.lbl_band_fluxes_sw_scenarios(ctx, mu, ssi, s_ods, sc[:2], BEGIN, END, albedo=albedo)
    for s in range(6):
        rdn, rup = api.lbl_band_fluxes_lw(ctx, t_hl, wn, dwn, _merged(ctx, d_ods, sc[s]), BEGIN, END)
        # rtol as above scaled to 130 layers: (3 x 130 + 8) 2^-53 = 4.4e-14, the same factor of 50 above it
        assert np.allclose(dn[s], rdn, rtol=2.5e-12, atol=1e-15 * rdn.max()) and np.allclose(up[s], rup, rtol=2.5e-12, atol=1e-15 * rup.max())
    for s in range(2):
        m = _merged(ctx, s_ods, sc[s])
        for a in range(8):
            rdn, rup = api.lbl_band_fluxes_sw(ctx, mu[a], ssi, m, BEGIN, END, albedo=albedo)
            assert np.allclose(sdn[s, a], rdn, rtol=2.5e-12, atol=1e-15 * rdn.max()) and np.allclose(sup[s, a], rup, rtol=2.5e-12, atol=1e-15 * rup.max())


def test_refusals(ctx):
    """Every PARAMETER_ERROR of the two entries; the library is called directly, only the argument under test is wrong."""
    from ecckd_amd import _lib, api
    nlay, ngas, nscen = 3, 2, 2
    t_hl, wn, dwn, d_ods = _lw_inputs(ctx, nlay, ("float32", "float64"))
    ssi, albedo, _ = _sw_inputs(ctx, nlay, ("float32",))
    hp = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
    t = np.ascontiguousarray(t_hl, dtype=np.float64)
    big = 1000                                       # room for the refused layer counts in every host array
    t_big = np.full(big + 1, 250.0)
    sc = np.ones((nscen * 17 * big,))
    b0, b1 = BEGIN.astype(np.int64), END.astype(np.int64)
    dn, up = np.empty(nscen * 8 * 4 * (big + 1)), np.empty(nscen * 8 * 4 * (big + 1))
    ptrs = (C.c_void_p * 17)(*([d_ods[0].data_ptr(), d_ods[1].data_ptr()] + [d_ods[0].data_ptr()] * 15))
    types = (C.c_int * 17)(*([4, 8] + [4] * 15))
    strides = (C.c_size_t * 17)(*([NWAV] * 17))
    mu = np.ascontiguousarray(np.linspace(0.1, 0.9, 9))
    ctx.fence_from_torch()
    ok = dict(h=ctx.handle, nangle=0, nlay=nlay, t=hp(t), wn=wn.data_ptr(), dwn=dwn.data_ptr(), ngas=ngas, od=ptrs, ty=types, st=strides,
              nscen=nscen, sc=hp(sc), nband=4, b0=hp(b0, C.c_int64), b1=hp(b1, C.c_int64), dn=hp(dn), up=hp(up), nsza=2, mu=hp(mu),
              ssi=ssi.data_ptr())

    def lw(**kw):
        a = dict(ok, **kw)
        return ctx.lib.ecckd_lbl_band_fluxes_lw_scenarios(a["h"], a["nangle"], a["nlay"], NWAV, a["t"], a["wn"], a["dwn"], a["ngas"], a["od"],
                                                          a["ty"], a["st"], a["nscen"], a["sc"], a["nband"], a["b0"], a["b1"], a["dn"], a["up"],
                                                          None, None)

    def sw(**kw):
        a = dict(ok, **kw)
        return ctx.lib.ecckd_lbl_band_fluxes_sw_scenarios(a["h"], a["nlay"], NWAV, a["nsza"], a["mu"], a["ssi"], None, a["ngas"], a["od"], a["ty"],
                                                          a["st"], a["nscen"], a["sc"], a["nband"], a["b0"], a["b1"], a["dn"], a["up"], None, None)
    bad = _lib.PARAMETER_ERROR
    assert lw() == 0 and sw() == 0
    for call in (lw, sw):
        for null in ("h", "od", "ty", "st", "sc", "b0", "b1", "dn", "up"):
            assert call(**{null: None}) == bad, null
        assert call(ngas=0) == bad and call(ngas=17) == bad and call(ngas=16) == 0
        assert call(nscen=0) == bad and call(nscen=-1) == bad
        assert call(nlay=0) == bad
    for null in ("t", "wn", "dwn"):
        assert lw(**{null: None}) == bad, null
    for null in ("mu", "ssi"):
        assert sw(**{null: None}) == bad, null
    null_gas = (C.c_void_p * 17)(*([d_ods[0].data_ptr(), None] + [None] * 15))
    assert lw(od=null_gas) == bad and sw(od=null_gas) == bad
    assert lw(ty=(C.c_int * 17)(*([4, 2] + [4] * 15))) == bad and lw(st=(C.c_size_t * 17)(*([NWAV - 1] * 17))) == bad
    assert lw(nangle=-1) == bad and lw(nangle=17) == bad and lw(nangle=16) == 0
    assert sw(nsza=0) == bad and sw(nsza=9) == bad and sw(nsza=8) == 0
    for wrong in (0.0, -0.5, 1.5):
        assert sw(nsza=1, mu=hp(np.array([wrong]))) == bad, wrong
    assert sw(nsza=2, mu=hp(np.array([0.5, 1.5]))) == bad and sw(nsza=1, mu=hp(np.array([1.0]))) == 0
    # the layer counts the block's accumulator does not hold: above 671 longwave, above 927 shortwave (the spectra are never read)
    assert api.lbl_scenarios_slots(False, 672) == 0 and api.lbl_scenarios_slots(True, 928) == 0
    assert lw(nlay=672, t=hp(t_big)) == bad and sw(nlay=928) == bad
    # and through the API
    with pytest.raises(api.EcckdError) as e:
        api.lbl_band_fluxes_sw_scenarios(ctx, [0.5, 1.5], ssi, d_ods, np.ones((1, 2)), BEGIN, END)
    assert e.value.code == bad
    with pytest.raises(api.EcckdError) as e:
        api.lbl_band_fluxes_lw_scenarios(ctx, t_hl, wn, dwn, d_ods, np.ones((1, 2)), BEGIN, END, nangle=17)
    assert e.value.code == bad
    with pytest.raises(ValueError):
        api.lbl_band_fluxes_lw_scenarios(ctx, t_hl, wn, dwn, d_ods, np.ones((1, 3)), BEGIN, END)
