"""ecckd_merge_scenario_dev / api.merge_scenario: the merged matrix of a scenario from all its gases in one pass, against what
it replaces - ngas calls of api.merge_spectrum, the first overwriting - bit for bit (array_equal on the downloaded doubles).

The sizes sit at the edges of the kernel's own tile, P consecutive wavenumbers per thread and T threads per block, as
ecckd_merge_scenario_geometry reports them; rows begin on and off 16-byte boundaries (strides nwav, nwav + 1, nwav + 3, views
that begin one element into their allocation), so the 16-byte accesses, the element-by-element ones, the head before the first
boundary and the ragged end of a row are all taken.  The padding of the inputs is NaN and that of the output a sentinel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ecckd_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
GEO = api.merge_scenario_geometry()
P, T = GEO["points_per_thread"], GEO["threads_per_block"]
NWAV = [1, P - 1, P, P + 1, P * T - 1, P * T, P * T + 1, 2 * P * T + 3]
NLAY = [1, 2, 9]
NGAS = [1, 2, 5, 16]
PADS = [0, 1, 3]
SENTINEL = -7.25
# 0 and 1, a negative factor, and one whose product with an optical depth of 1e-30 is subnormal (1e-320)
SCALES = np.array([0.0, 1.0, -2.5, 1.0e-290, 0.37, 3.0])
DEPTHS = np.array([0.0, 1.0e-30, 60.0])


def test_geometry_answers_without_a_device():
    assert P >= 2 and T >= 64 and T % 64 == 0
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\nfrom ecckd_amd import api\n"
                          "g = api.merge_scenario_geometry(); print(g['points_per_thread'], g['threads_per_block'])" % ROOT],
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == [str(P), str(T)], out.stdout + out.stderr
    lib = api._lib.load_library()
    assert lib.ecckd_merge_scenario_geometry(None, None) == 147


def _message():
    return api._lib.load_library().ecckd_last_error().decode()


def _dtypes(kind, ngas):
    if kind == "f32":
        return [np.float32] * ngas
    if kind == "f64":
        return [np.float64] * ngas
    return [np.float32 if g % 2 == 0 else np.float64 for g in range(ngas)]


def _gas(rng, nlay, nwav, dtype):
    """optical depths between 1e-6 and 60 with the three pinned values strewn in"""
    od = np.exp(rng.uniform(np.log(1e-6), np.log(60.0), (nlay, nwav)))
    pick = rng.integers(0, 6, (nlay, nwav))
    for k, v in enumerate(DEPTHS):
        od[pick == k] = v
    return od.astype(dtype)


def _strided(ctx, host, stride, offset, fill):
    """a device view (nlay, nwav) with row stride `stride` that begins `offset` elements into its allocation, the rest `fill`
    -> (view, the whole allocation)"""
    import torch
    nlay, nwav = host.shape
    flat = np.full(offset + nlay * stride, fill, dtype=host.dtype)
    rows = np.lib.stride_tricks.as_strided(flat[offset:], (nlay, nwav), (stride * host.itemsize, host.itemsize))
    rows[...] = host
    d = torch.as_tensor(flat, device=ctx.device)
    return torch.as_strided(d, (nlay, nwav), (stride, 1), offset), d


def _outside(flat, nlay, nwav, stride, offset):
    """the elements of an allocation that are not part of the view"""
    mask = np.ones(flat.size, dtype=bool)
    for l in range(nlay):
        mask[offset + l * stride: offset + l * stride + nwav] = False
    return flat[mask]


@gpu
@pytest.mark.parametrize("kind", ["f32", "f64", "mixed"])
@pytest.mark.parametrize("nwav", NWAV)
def test_one_pass_equals_gas_after_gas(ctx, nwav, kind):
    rng = np.random.default_rng(1000 * nwav + len(kind))
    for nlay in NLAY:
        for ngas in NGAS:
            dtypes = _dtypes(kind, ngas)
            host = [_gas(rng, nlay, nwav, dt) for dt in dtypes]
            scale = SCALES[(np.arange(ngas * nlay) * 5 + nlay + ngas) % SCALES.size].reshape(ngas, nlay)
            for pad in PADS:
                for offset in (0, 1):
                    stride = nwav + pad
                    ods = [_strided(ctx, h, stride, offset, np.nan)[0] for h in host]
                    merged, whole = _strided(ctx, np.full((nlay, nwav), np.nan), stride, offset, SENTINEL)
                    got = api.merge_scenario(ctx, ods, scale, merged=merged)
                    assert got is merged
                    want = None
                    for g in range(ngas):
                        want = api.merge_spectrum(ctx, ods[g], scale[g], want)
                    where = (nwav, kind, nlay, ngas, pad, offset)
                    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), where
                    assert not np.isnan(got.cpu().numpy()).any(), where
                    assert np.all(_outside(whole.cpu().numpy(), nlay, nwav, stride, offset) == SENTINEL), where


@gpu
def test_values_scales_and_numpy_inputs(ctx):
    """the pinned scales and optical depths do occur, a subnormal product among them; numpy arrays and one factor per gas go in"""
    nlay, nwav, ngas = 2, P * T + 1, 5
    rng = np.random.default_rng(7)
    host = [_gas(rng, nlay, nwav, dt) for dt in _dtypes("mixed", ngas)]
    scale = np.array([0.0, 1.0, -2.5, 1.0e-290, 0.37])
    got = api.merge_scenario(ctx, host, scale).cpu().numpy()                   # numpy in, one factor per gas
    want = None
    for g in range(ngas):
        want = api.merge_spectrum(ctx, api._torch().as_tensor(host[g], device=ctx.device), np.full(nlay, scale[g]), want)
    assert np.array_equal(got, want.cpu().numpy())
    for v in DEPTHS:
        assert all(np.any(h == h.dtype.type(v)) for h in host)
    product = host[3].astype(np.float64) * scale[3]
    assert np.any((product != 0.0) & (np.abs(product) < np.finfo(np.float64).tiny))          # subnormal, and not flushed
    alone = api.merge_scenario(ctx, [host[3]], scale[3:4]).cpu().numpy()
    assert np.array_equal(alone, product)
    assert np.any(got < 0.0)                                                   # the negative factor


@gpu
def test_refusals(ctx):
    import torch
    nlay, nwav = 3, 2 * P + 1
    od32 = torch.ones((nlay, nwav), dtype=torch.float32, device=ctx.device)
    od64 = torch.ones((nlay, nwav), dtype=torch.float64, device=ctx.device)
    merged = torch.full((nlay, nwav), SENTINEL, dtype=torch.float64, device=ctx.device)
    scale = np.ones((17, nlay))
    sc = scale.ctypes.data_as(C.POINTER(C.c_double))

    def call(ngas, ptrs, types, strides, merged_stride=nwav, out=merged.data_ptr(), h_scale=sc):
        ctx.fence_from_torch()
        return ctx.lib.ecckd_merge_scenario_dev(ctx.handle, nlay, nwav, ngas, (C.c_void_p * 17)(*ptrs), (C.c_int * 17)(*types),
                                                (C.c_size_t * 17)(*strides), h_scale, C.c_void_p(out), merged_stride)

    ok = ([od32.data_ptr(), od64.data_ptr()] + [od32.data_ptr()] * 15, [4, 8] + [4] * 15, [nwav] * 17)
    assert call(0, *ok) == 147 and "ngas" in _message()
    assert call(17, *ok) == 147 and "ngas" in _message()
    assert call(2, ok[0], [4, 2] + [4] * 15, ok[2]) == 147 and "od_type[1]" in _message()
    assert call(2, ok[0], ok[1], [nwav, nwav - 1] + [nwav] * 15) == 147 and "od_stride[1]" in _message()
    assert call(2, [od32.data_ptr(), None] + [None] * 15, ok[1], ok[2]) == 147 and "d_od[1]" in _message()
    assert call(2, *ok, merged_stride=nwav - 1) == 147 and "merged_stride" in _message()
    assert call(2, *ok, out=None) == 147
    assert call(2, *ok, h_scale=None) == 147
    assert np.all(merged.cpu().numpy() == SENTINEL)                            # nothing was launched
    assert call(2, *ok) == 0
    assert np.array_equal(merged.cpu().numpy(), np.full((nlay, nwav), 2.0))
    with pytest.raises(ValueError):
        api.merge_scenario(ctx, [], np.ones((0, nlay)))
    with pytest.raises(ValueError):
        api.merge_scenario(ctx, [od32, od64], np.ones((3, nlay)))
