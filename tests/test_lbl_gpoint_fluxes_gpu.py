"""GPU parity for the fused line-by-line longwave fluxes per g point (ecckd_lbl_gpoint_fluxes_lw, lw_spectra.cpp:222-257) and
the spectral-output mode of the same kernel (ecckd_lbl_spectral_fluxes_lw): against the oracle's planck_function +
radiative_transfer_lw summed per g point on the CPU, against the composed path (spectral rows + ecckd_gmap_sum_rows), against
the band kernel, and for reproducibility.

g-point maps: random, with wavenumbers of no g point (-1) and - where there is more than one g point - one g point that owns
no wavenumber."""
import functools

import numpy as np
import pytest
import torch

from conftest import make_lw_case

pytestmark = pytest.mark.gpu

# (nlay, nwav, ng, dtype of the optical depths).  200 g points need several launches at either layer count (the block's
# accumulator holds 48 columns at 54 layers, 128 at 20); 2^20 + 4321 wavenumbers give every block several tiles and every g
# point many blocks.
CASES = [(20, 20011, 1, "float64"), (54, 20011, 16, "float32"), (20, 19999, 200, "float32"), (54, 20011, 200, "float32"),
         (54, 2 ** 20 + 4321, 16, "float32")]
EMPTY_G = 3          # the g point without wavenumbers (ng > 1)


@functools.lru_cache(maxsize=None)
def _case(nlay, nwav, ng, dtype):
    from ecckd_amd import synthetic as syn
    p, wn, dwn, od = make_lw_case(nwav, nlay=nlay, seed=11, dtype=dtype, nlines=48 if nwav < 100000 else 6)
    t_hl = syn.temperature_profile(p)
    rng = np.random.default_rng(1234 + ng + nlay)
    g = rng.integers(0, ng, size=nwav).astype(np.int32)
    if ng > 1:
        g[g == EMPTY_G] = (EMPTY_G + 1) % ng
    g[rng.random(nwav) < 0.07] = -1
    g[:3] = -1                                       # (a run of unassigned points at the start of a tile)
    return p, wn, dwn, od, t_hl, g


def _oracle_fluxes(oracle, t_hl, wn, dwn, od):
    planck = oracle.planck_function(t_hl, wn, dwn)
    return oracle.radiative_transfer_lw(planck, od.astype(np.float64), np.ones(wn.size), planck[-1])


def _sum_per_g(f, g, ng):
    out = np.zeros((f.shape[0], ng))
    for ig in range(ng):
        out[:, ig] = f[:, g == ig].sum(1, dtype=np.float64)
    return out


def _gmap(ctx, g, ng, wn, dwn):
    from ecckd_amd import api
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    return api.GPointMap(ctx, dev(g), ng, dev(wn), dev(dwn))


@pytest.mark.parametrize("nlay,nwav,ng,dtype", CASES)
def test_against_the_oracle(ctx, oracle, nlay, nwav, ng, dtype):
    """1. h_flux_* and h_bb_* against the oracle's spectral fluxes summed with numpy in float64; rtol 1e-10 is what
    test_lbl_fluxes_gpu.py uses for the band sums of the same arithmetic against the same oracle functions."""
    p, wn, dwn, od, t_hl, g = _case(nlay, nwav, ng, dtype)
    gm = _gmap(ctx, g, ng, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_hl, torch.as_tensor(od, device=ctx.device))
    gm.close()
    fdn, fup = _oracle_fluxes(oracle, t_hl, wn, dwn, od)
    odn, oup = _sum_per_g(fdn, g, ng), _sum_per_g(fup, g, ng)
    for name, a, b in (("dn", dn, odn), ("up", up, oup), ("bb_dn", bdn, fdn.sum(1)), ("bb_up", bup, fup.sum(1))):
        print(name, "max rel diff", np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
    assert np.allclose(dn, odn, rtol=1e-10, atol=1e-300)
    assert np.allclose(up, oup, rtol=1e-10, atol=1e-300)
    assert np.allclose(bdn, fdn.sum(1), rtol=1e-10, atol=1e-300)
    assert np.allclose(bup, fup.sum(1), rtol=1e-10, atol=1e-300)
    assert np.all(dn[0] == 0.0) and bdn[0] == 0.0                 # nothing comes down at the top of the atmosphere
    if ng > 1:
        assert np.all(dn[:, EMPTY_G] == 0.0) and np.all(up[:, EMPTY_G] == 0.0)      # an empty g point: exactly 0
        assert np.all(up[:, (EMPTY_G + 1) % ng] > 0.0)


@pytest.mark.parametrize("nlay,nwav,ng,dtype", CASES)
def test_against_the_composed_path(ctx, nlay, nwav, ng, dtype):
    """2. The spectral-output mode's FLOAT rows, summed per g point by ecckd_gmap_sum_rows, against the fused sums.  A row
    element is the fused path's double flux rounded to nearest FLOAT: relative error <= 2^-24 = 0.5 x 2^-23 for a normal FLOAT,
    absolute error <= 2^-150 for a subnormal one.  All terms are >= 0, so a sum of rounded terms differs from the sum of the
    exact ones by at most 2^-24 relative (+ count x 2^-150); the two double summations add (their addition chains, a few
    hundred, see test_band_kernel_consistency) x 2^-53 ~ 1e-14 = 1e-7 x 2^-23.  Factor: 0.5 + 1e-6."""
    from ecckd_amd import api
    p, wn, dwn, od, t_hl, g = _case(nlay, nwav, ng, dtype)
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    gm = _gmap(ctx, g, ng, wn, dwn)
    d_od = dev(od)
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_hl, d_od)
    sdn, sup, sbdn, sbup = api.lbl_spectral_fluxes_lw(ctx, t_hl, dev(wn), dev(dwn), d_od)
    assert sdn.dtype == torch.float32 and tuple(sdn.shape) == (nlay + 1, nwav)
    cdn, cup = gm.sum_rows(sdn), gm.sum_rows(sup)
    gm.close()
    rtol, atol = 2.0 ** -23 * (0.5 + 1e-6), nwav * 2.0 ** -150
    for name, a, b in (("dn", cdn, dn), ("up", cup, up)):
        print(name, "max rel diff / 2^-23:", np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) * 2.0 ** 23)
    assert np.allclose(cdn, dn, rtol=rtol, atol=atol)
    assert np.allclose(cup, up, rtol=rtol, atol=atol)
    # the broadband sums of the spectral mode are sums of the same doubles over the same wavenumbers as h_bb: only the
    # order differs (<= 2 x the chains of test_band_kernel_consistency x 2^-53 < 1e-12)
    assert np.allclose(sbdn, bdn, rtol=1e-12, atol=0.0) and np.allclose(sbup, bup, rtol=1e-12, atol=0.0)
    assert np.all(sdn[0].cpu().numpy() == 0.0)


@pytest.mark.parametrize("nlay,nwav,ng,dtype", CASES)
def test_g_points_add_up_to_the_broadband_flux(ctx, nlay, nwav, ng, dtype):
    """3. sum_g h_flux[l][g] + (flux of the wavenumbers without a g point) == h_bb[l] to 1e-12.  The flux of the -1 wavenumbers
    comes from the device too: a second map gives them a g point of their own (ng + 1 g points, nothing unassigned).
    This is a consistency check, not an independent closure: the library forms h_bb on the host from the same accumulator
    columns that h_flux returns plus the column of the -1 points, so only that column (through a second map and the same
    kernel) is new information here.  h_bb is compared with the oracle independently in test_against_the_oracle."""
    p, wn, dwn, od, t_hl, g = _case(nlay, nwav, ng, dtype)
    d_od = torch.as_tensor(od, device=ctx.device)
    gm = _gmap(ctx, g, ng, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_hl, d_od)
    gm.close()
    g2 = np.where(g < 0, ng, g).astype(np.int32)
    gm2 = _gmap(ctx, g2, ng + 1, wn, dwn)
    dn2, up2, bdn2, bup2 = gm2.lbl_fluxes_lw(t_hl, d_od)
    gm2.close()
    assert np.allclose(dn2[:, :ng], dn, rtol=1e-12, atol=0.0) and np.allclose(up2[:, :ng], up, rtol=1e-12, atol=0.0)
    assert np.all(up2[:, ng] > 0.0)
    assert np.allclose(dn.sum(1) + dn2[:, ng], bdn, rtol=1e-12, atol=0.0)
    assert np.allclose(up.sum(1) + up2[:, ng], bup, rtol=1e-12, atol=0.0)
    assert np.allclose(bdn2, bdn, rtol=1e-12, atol=0.0) and np.allclose(bup2, bup, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("nlay,nwav,ng,dtype", CASES[1:3] + CASES[4:])
def test_reproducible_and_float_double_agree(ctx, nlay, nwav, ng, dtype):
    """4. Two calls give the same bits; DOUBLE optical depths that hold the upcast FLOAT values give the FLOAT path's bits."""
    from ecckd_amd import api
    p, wn, dwn, od, t_hl, g = _case(nlay, nwav, ng, dtype)
    assert od.dtype == np.float32
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    gm = _gmap(ctx, g, ng, wn, dwn)
    d_od = dev(od)
    a = gm.lbl_fluxes_lw(t_hl, d_od)
    b = gm.lbl_fluxes_lw(t_hl, d_od)
    c = gm.lbl_fluxes_lw(t_hl, dev(od.astype(np.float64)))
    gm.close()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    s1 = api.lbl_spectral_fluxes_lw(ctx, t_hl, dev(wn), dev(dwn), d_od)
    s2 = api.lbl_spectral_fluxes_lw(ctx, t_hl, dev(wn), dev(dwn), dev(od.astype(np.float64)))
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])
    assert np.array_equal(s1[2], s2[2]) and np.array_equal(s1[3], s2[3])


@pytest.mark.parametrize("nlay,nwav,nband,dtype", [(54, 20011, 13, "float32"), (20, 20011, 5, "float64")])
def test_band_kernel_consistency(ctx, nlay, nwav, nband, dtype):
    """5. g_point = band index over contiguous bands: the same per-wavenumber arithmetic as ecckd_lbl_band_fluxes_lw, all terms
    >= 0, so the two results differ by at most (the longest addition chain of the one + that of the other) x 2^-53 relative.
    Chains (additions a single addend can pass through):
      fused: 8 (its piece of 8 ranks) + 32 per tile of its block (the pieces of a column's 32 segments into the accumulator)
             x tiles per block + the blocks of the launch (combine, in block order);
      band kernel: 6 (wave tree) + 1 (the wave's accumulator) + 3 (four waves) + the 256-point chunks of the band (host)."""
    from ecckd_amd import api
    p, wn, dwn, od, t_hl, _ = _case(nlay, nwav, 16, dtype)
    edges = np.linspace(0, nwav, nband + 1).astype(np.int64)
    begin, end = edges[:-1], edges[1:] - 1
    g = np.repeat(np.arange(nband, dtype=np.int32), np.diff(edges))
    dev = lambda a: torch.as_tensor(a, device=ctx.device)
    d_od = dev(od)
    gm = _gmap(ctx, g, nband, wn, dwn)
    dn, up, bdn, bup = gm.lbl_fluxes_lw(t_hl, d_od)
    gm.close()
    bdn_k, bup_k = api.lbl_band_fluxes_lw(ctx, t_hl, dev(wn), dev(dwn), d_od, begin, end)     # (nband, nlay+1)
    ntiles = -(-nwav // 256)
    tiles_per_block = max(1, -(-ntiles // 2048))
    nblocks = -(-ntiles // tiles_per_block)
    chain_fused = 8 + 32 * tiles_per_block + nblocks
    chain_band = 6 + 1 + 3 + int(np.max(-(-(end - begin + 1) // 256)))
    bound = (chain_fused + chain_band) * 2.0 ** -53
    print("chains", chain_fused, chain_band, "bound", bound)
    assert bound < 1e-12
    for name, a, b in (("dn", dn, bdn_k.T), ("up", up, bup_k.T)):
        print(name, "max rel diff", np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
        assert np.allclose(a, b, rtol=bound, atol=0.0)
