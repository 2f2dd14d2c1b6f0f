"""GPU parity for the fused multi-angle line-by-line shortwave fluxes per g point (ecckd_lbl_gpoint_fluxes_sw) and the
spectral-output mode of the same kernel (ecckd_lbl_spectral_fluxes_sw): against the oracle's radiative_transfer_direct_sw /
_norayleigh_sw summed per g point on the CPU, angle by angle against single-angle calls, against the composed path (spectral
rows + ecckd_gmap_sum_rows), against the band kernel, for reproducibility and for the refusals.

g-point maps: random, with 7 % of the wavenumbers at no g point (-1), a run of -1 at the start of the first tile and - where
there is more than one g point - one g point that owns no wavenumber."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import make_lw_case

pytestmark = pytest.mark.gpu

# (nlay, nwav, ng, nsza, dtype of the optical depths).  The block's accumulator holds 67 column-angles at 54 layers and 176 at
# 20: 17 columns x 3 angles fit in one launch, 201 columns take several launches per angle at either layer count; 2^20 + 4321
# wavenumbers give every block several tiles and every g point many blocks.  The last case is the shape of the shipped models
# (33 columns at 54 layers: five angles go in launches of 2 + 2 + 1), the only one with several launches of several angles.
CASES = [(20, 20011, 1, 1, "float64"), (54, 20011, 16, 3, "float32"), (20, 19999, 200, 5, "float32"),
         (54, 20011, 200, 5, "float32"), (54, 2 ** 20 + 4321, 16, 3, "float32"), (54, 20011, 32, 5, "float32")]
ANGLES = {1: (0.5,), 3: (0.1, 0.5, 0.9), 5: (0.1, 0.3, 0.5, 0.7, 0.9)}
EMPTY_G = 3          # the g point without wavenumbers (ng > 1)


@functools.lru_cache(maxsize=None)
def _case(nlay, nwav, ng, dtype):
    from ecckd_amd import synthetic as syn
    p, wn, dwn, od = make_lw_case(nwav, nlay=nlay, seed=11, dtype=dtype, lo=250.0, hi=50000.0, column_scale=3.0,
                                  nlines=48 if nwav < 100000 else 6)
    ssi = syn.solar_spectral_irradiance(wn, dwn)
    albedo = np.where(wn < 12000.0, 0.2, 0.05)
    rng = np.random.default_rng(4321 + ng + nlay)
    g = rng.integers(0, ng, size=nwav).astype(np.int32)
    if ng > 1:
        g[g == EMPTY_G] = (EMPTY_G + 1) % ng
    g[rng.random(nwav) < 0.07] = -1
    g[:3] = -1                                       # (a run of unassigned points at the start of a tile)
    return wn, dwn, od, ssi, albedo, g


@functools.lru_cache(maxsize=None)
def _oracle_sums(nlay, nwav, ng, nsza, dtype, with_albedo):
    """Per angle: (per-g sums dn, up; broadband dn, up) of the oracle's spectral fluxes, summed with numpy in float64."""
    import pyoracle as oracle
    wn, dwn, od, ssi, albedo, g = _case(nlay, nwav, ng, dtype)
    od64 = od.astype(np.float64)
    out = []
    for mu in ANGLES[nsza]:
        if with_albedo:
            fdn, fup = oracle.radiative_transfer_norayleigh_sw(mu, ssi, od64, albedo)
        else:
            fdn, fup = oracle.radiative_transfer_direct_sw(mu, ssi, od64), np.zeros((nlay + 1, nwav))
        out.append((_sum_per_g(fdn, g, ng), _sum_per_g(fup, g, ng), fdn.sum(1), fup.sum(1)))
    return out


def _sum_per_g(f, g, ng):
    out = np.zeros((f.shape[0], ng))
    for ig in range(ng):
        out[:, ig] = f[:, g == ig].sum(1, dtype=np.float64)
    return out


def _gmap(ctx, g, ng, wn, dwn):
    from ecckd_amd import api
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    return api.GPointMap(ctx, dev(g), ng, dev(wn), dev(dwn))


@pytest.mark.parametrize("with_albedo", [False, True])
@pytest.mark.parametrize("nlay,nwav,ng,nsza,dtype", CASES)
def test_against_the_oracle(ctx, oracle, nlay, nwav, ng, nsza, dtype, with_albedo):
    """1. h_flux_* and h_bb_* of every angle against the oracle's spectral fluxes summed with numpy in float64; rtol 1e-11 is
    what test_lbl_fluxes_gpu.py uses for the band sums of the same arithmetic against the same oracle functions (all terms are
    >= 0, so a per-g sum carries no more relative error than its terms)."""
    wn, dwn, od, ssi, albedo, g = _case(nlay, nwav, ng, dtype)
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    mu = ANGLES[nsza]
    gm = _gmap(ctx, g, ng, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_sw(mu, dev(ssi), dev(od), dev(albedo) if with_albedo else None)
    gm.close()
    assert dn.shape == up.shape == (nsza, nlay + 1, ng) and bdn.shape == bup.shape == (nsza, nlay + 1)
    ref = _oracle_sums(nlay, nwav, ng, nsza, dtype, with_albedo)
    ssi_g = _sum_per_g(ssi[None, :], g, ng)[0]
    for s in range(nsza):
        odn, oup, obdn, obup = ref[s]
        for name, a, b in (("dn", dn[s], odn), ("up", up[s], oup), ("bb_dn", bdn[s], obdn), ("bb_up", bup[s], obup)):
            print("angle", s, name, "max rel diff", np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
        assert np.allclose(dn[s], odn, rtol=1e-11, atol=1e-300)
        assert np.allclose(up[s], oup, rtol=1e-11, atol=1e-300)
        assert np.allclose(bdn[s], obdn, rtol=1e-11, atol=1e-300)
        assert np.allclose(bup[s], obup, rtol=1e-11, atol=1e-300)
        assert np.allclose(dn[s, 0], mu[s] * ssi_g, rtol=1e-12, atol=0.0)
        if ng > 1:
            assert np.all(dn[s][:, EMPTY_G] == 0.0) and np.all(up[s][:, EMPTY_G] == 0.0)    # an empty g point: exactly 0
            assert np.all(dn[s][:, (EMPTY_G + 1) % ng] > 0.0)
    if with_albedo:
        assert np.all(bup > 0.0)
    else:
        assert np.all(up == 0.0) and np.all(bup == 0.0)             # no albedo: no upwelling sweep, exactly 0


@pytest.mark.parametrize("nlay,nwav,ng,nsza,dtype", CASES[1:4] + CASES[5:])
def test_angles_are_independent(ctx, nlay, nwav, ng, nsza, dtype):
    """2. Angle s of a multi-angle call has the bits of a single-angle call with cos_sza[s], in both entry points: the shared
    exp(-2 tau) and the split over launches change nothing."""
    from ecckd_amd import api
    wn, dwn, od, ssi, albedo, g = _case(nlay, nwav, ng, dtype)
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    mu = ANGLES[nsza]
    d_ssi, d_od, d_alb = dev(ssi), dev(od), dev(albedo)
    gm = _gmap(ctx, g, ng, wn, dwn)
    multi = gm.lbl_fluxes_sw(mu, d_ssi, d_od, d_alb)
    smulti = api.lbl_spectral_fluxes_sw(ctx, mu, d_ssi, d_od, d_alb)
    for s in range(nsza):
        one = gm.lbl_fluxes_sw(mu[s], d_ssi, d_od, d_alb)              # a scalar is one angle
        for a, b in zip(multi, one):
            assert b.shape[0] == 1 and np.array_equal(a[s], b[0])
        sone = api.lbl_spectral_fluxes_sw(ctx, mu[s], d_ssi, d_od, d_alb)
        assert torch.equal(smulti[0][s], sone[0][0]) and torch.equal(smulti[1][s], sone[1][0])
        assert np.array_equal(smulti[2][s], sone[2][0]) and np.array_equal(smulti[3][s], sone[3][0])
    gm.close()


@pytest.mark.parametrize("nlay,nwav,ng,nsza,dtype", CASES)
def test_against_the_composed_path(ctx, nlay, nwav, ng, nsza, dtype):
    """3. The spectral-output mode's FLOAT rows, summed per g point by ecckd_gmap_sum_rows, against the fused sums: non-negative
    terms rounded to nearest FLOAT (relative error <= 2^-24 for a normal FLOAT, absolute <= 2^-150 for a subnormal one), the
    reasoning of test_lbl_gpoint_fluxes_gpu.py::test_against_the_composed_path."""
    from ecckd_amd import api
    wn, dwn, od, ssi, albedo, g = _case(nlay, nwav, ng, dtype)
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    mu = ANGLES[nsza]
    d_ssi, d_od, d_alb = dev(ssi), dev(od), dev(albedo)
    gm = _gmap(ctx, g, ng, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_sw(mu, d_ssi, d_od, d_alb)
    sdn, sup, sbdn, sbup = api.lbl_spectral_fluxes_sw(ctx, mu, d_ssi, d_od, d_alb)
    assert sdn.dtype == torch.float32 and tuple(sdn.shape) == (nsza, nlay + 1, nwav) and tuple(sup.shape) == tuple(sdn.shape)
    rtol, atol = 2.0 ** -23 * (0.5 + 1e-6), nwav * 2.0 ** -150
    for s in range(nsza):
        cdn, cup = gm.sum_rows(sdn[s]), gm.sum_rows(sup[s])
        for name, a, b in (("dn", cdn, dn[s]), ("up", cup, up[s])):
            print("angle", s, name, "max rel diff / 2^-23:", np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) * 2.0 ** 23)
        assert np.allclose(cdn, dn[s], rtol=rtol, atol=atol)
        assert np.allclose(cup, up[s], rtol=rtol, atol=atol)
    gm.close()
    assert np.allclose(sbdn, bdn, rtol=1e-12, atol=0.0) and np.allclose(sbup, bup, rtol=1e-12, atol=0.0)
    # without an albedo the spectral mode writes upwelling rows of exactly 0
    _, sup0, _, sbup0 = api.lbl_spectral_fluxes_sw(ctx, mu[0], d_ssi, d_od)
    assert not torch.any(sup0) and np.all(sbup0 == 0.0)


@pytest.mark.parametrize("nlay,nwav,ng,nsza,dtype", CASES[1:3] + CASES[4:])
def test_reproducible_and_float_double_agree(ctx, nlay, nwav, ng, nsza, dtype):
    """4. Two calls give the same bits; DOUBLE optical depths that hold the upcast FLOAT values give the FLOAT path's bits."""
    from ecckd_amd import api
    wn, dwn, od, ssi, albedo, g = _case(nlay, nwav, ng, dtype)
    assert od.dtype == np.float32
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    mu = ANGLES[nsza]
    d_ssi, d_od, d_alb, d_od64 = dev(ssi), dev(od), dev(albedo), dev(od.astype(np.float64))
    gm = _gmap(ctx, g, ng, wn, dwn)
    a = gm.lbl_fluxes_sw(mu, d_ssi, d_od, d_alb)
    b = gm.lbl_fluxes_sw(mu, d_ssi, d_od, d_alb)
    c = gm.lbl_fluxes_sw(mu, d_ssi, d_od64, d_alb)
    gm.close()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    s1 = api.lbl_spectral_fluxes_sw(ctx, mu, d_ssi, d_od, d_alb)
    s2 = api.lbl_spectral_fluxes_sw(ctx, mu, d_ssi, d_od64, d_alb)
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])
    assert np.array_equal(s1[2], s2[2]) and np.array_equal(s1[3], s2[3])


@pytest.mark.parametrize("nlay,nwav,nband,nsza,dtype", [(54, 20011, 13, 3, "float32"), (20, 20011, 5, 5, "float64")])
def test_band_kernel_consistency(ctx, nlay, nwav, nband, nsza, dtype):
    """5. g_point = band index over contiguous bands: the same per-wavenumber arithmetic as ecckd_lbl_band_fluxes_sw (exp, the
    same multiplication order), all terms >= 0, so the two results differ by at most (the longest addition chain of the one +
    that of the other) x 2^-53 relative.  Chains (additions a single addend can pass through):
      fused: 8 (its piece of 8 ranks) + 32 per tile of its block (the pieces of a column's 32 segments into the accumulator)
             x tiles per block + the blocks of the launch (combine, in block order);
      band kernel: 6 (wave tree) + 1 (the wave's accumulator) + 3 (four waves) + the 256-point chunks of the band (host)."""
    from ecckd_amd import api
    wn, dwn, od, ssi, albedo, _ = _case(nlay, nwav, 16, dtype)
    edges = np.linspace(0, nwav, nband + 1).astype(np.int64)
    begin, end = edges[:-1], edges[1:] - 1
    g = np.repeat(np.arange(nband, dtype=np.int32), np.diff(edges))
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    mu = ANGLES[nsza]
    d_ssi, d_od, d_alb = dev(ssi), dev(od), dev(albedo)
    gm = _gmap(ctx, g, nband, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_sw(mu, d_ssi, d_od, d_alb)
    gm.close()
    # the constants of csrc/gpoint_bin.hpp: GB_THREADS = 256 points per tile, GB_TARGET_BLOCKS = 2048,
    # GB_SEGLEN = 8 ranks per piece, GB_SEG = 32 segments per tile
    ntiles = -(-nwav // 256)
    tiles_per_block = max(1, -(-ntiles // 2048))
    nblocks = -(-ntiles // tiles_per_block)
    chain_fused = 8 + 32 * tiles_per_block + nblocks
    chain_band = 6 + 1 + 3 + int(np.max(-(-(end - begin + 1) // 256)))
    bound = (chain_fused + chain_band) * 2.0 ** -53
    print("chains", chain_fused, chain_band, "bound", bound)
    assert bound < 1e-12
    for s in range(nsza):
        bdn_k, bup_k = api.lbl_band_fluxes_sw(ctx, mu[s], d_ssi, d_od, begin, end, albedo=d_alb)      # (nband, nlay+1)
        for name, a, b in (("dn", dn[s], bdn_k.T), ("up", up[s], bup_k.T)):
            print("angle", s, name, "max rel diff", np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
            assert np.allclose(a, b, rtol=bound, atol=0.0)


def test_refusals(ctx):
    """6. PARAMETER_ERROR: nsza of 0 and of 9, cos_sza of 0 and of 1.5, od_stride < nwav, in both entry points."""
    from ecckd_amd import api, _lib
    nlay, nwav, ng = 20, 20011, 1
    wn, dwn, od, ssi, albedo, g = _case(nlay, nwav, ng, "float64")
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    d_ssi, d_od = dev(ssi), dev(od)
    gm = _gmap(ctx, g, ng, wn, dwn)
    nine = np.linspace(0.1, 0.9, 9)
    # the library is called directly: every buffer has room for nine angles, only the argument under test is wrong
    mu_buf = np.ascontiguousarray(nine)
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    dn, up = np.empty((9, nlay + 1, ng)), np.empty((9, nlay + 1, ng))
    bdn, bup = np.empty((9, nlay + 1)), np.empty((9, nlay + 1))
    sdn = torch.empty((9, nlay + 1, nwav), dtype=torch.float32, device=ctx.device)
    sup = torch.empty_like(sdn)
    ctx.fence_from_torch()

    def fused(nsza, mu, stride=nwav):
        return ctx.lib.ecckd_lbl_gpoint_fluxes_sw(gm.handle, nlay, nsza, hp(mu), d_ssi.data_ptr(), None, d_od.data_ptr(), 8, stride,
                                                  hp(dn), hp(up), hp(bdn), hp(bup))

    def spectral(nsza, mu, stride=nwav):
        return ctx.lib.ecckd_lbl_spectral_fluxes_sw(ctx.handle, nlay, nwav, nsza, hp(mu), d_ssi.data_ptr(), None, d_od.data_ptr(), 8,
                                                    stride, sdn.data_ptr(), sup.data_ptr(), nwav, hp(bdn), hp(bup))
    for call in (fused, spectral):
        assert call(1, mu_buf) == 0
        assert call(0, mu_buf) == _lib.PARAMETER_ERROR
        assert call(9, mu_buf) == _lib.PARAMETER_ERROR
        assert call(1, np.array([0.0])) == _lib.PARAMETER_ERROR
        assert call(1, np.array([1.5])) == _lib.PARAMETER_ERROR
        assert call(2, np.array([0.5, 1.5])) == _lib.PARAMETER_ERROR
        assert call(1, mu_buf, stride=nwav - 1) == _lib.PARAMETER_ERROR
    # and through the API
    for bad in ([], list(nine), 0.0, 1.5):
        with pytest.raises(api.EcckdError) as e:
            gm.lbl_fluxes_sw(bad, d_ssi, d_od)
        assert e.value.code == _lib.PARAMETER_ERROR
        with pytest.raises(api.EcckdError) as e:
            api.lbl_spectral_fluxes_sw(ctx, bad, d_ssi, d_od)
        assert e.value.code == _lib.PARAMETER_ERROR
    with pytest.raises(api.EcckdError) as e:
        gm.lbl_fluxes_sw(0.5, d_ssi, d_od[:, :nwav - 5].contiguous())
    assert e.value.code == _lib.PARAMETER_ERROR
    gm.close()
