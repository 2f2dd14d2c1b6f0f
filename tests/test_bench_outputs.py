"""bench.py --dump-outputs: the arrays of a find_g_points result as DIR/<name>.npy, float32 / float64 only, the per-wavenumber
maps at the same seeded sample of points from run to run, at most 64 MB in all.  Host tensors stand in for the device ones."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _result(torch, nwav, ngas, seed=0):
    g = torch.Generator().manual_seed(seed)
    gases = [dict(name="gas%d" % i, n_g_points=[4], band_number=[0] * 4, rank1=[0, 5, 9, 20], rank2=[4, 8, 19, nwav - 1],
                  error=[0.01, 0.02, 0.03, 0.04], sorting_variable=[1.0, 2.0, 3.0, 4.0], status=[0], comp_cost=[12.0],
                  g_min=np.arange(6), g_max=np.arange(6)) for i in range(ngas)]
    return dict(ng=6, n_unassigned=0, cost_sum=0.1, comp_cost_sum=48.0, points=1e9, band_number=np.zeros(6, dtype=np.int32),
                gases=gases, g_point=torch.randint(0, 6, (nwav,), dtype=torch.int32, generator=g),
                gas_g_point=[torch.randint(0, 4, (nwav,), dtype=torch.int32, generator=g) for _ in range(ngas)])


def test_dump_of_a_find_g_result(tmp_path):
    import torch
    nwav = bench.DUMP_SAMPLE + 12345
    res = _result(torch, nwav, 8)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_arrays(a, bench.find_g_outputs(res, nwav))
    bench.dump_arrays(b, bench.find_g_outputs(res, nwav))
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "g_point.npy" in names and "gas7_error.npy" in names
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= bench.DUMP_LIMIT_BYTES
    idx = np.load(os.path.join(a, "sample_index.npy")).astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < nwav
    assert np.array_equal(np.load(os.path.join(a, "g_point.npy")), res["g_point"].numpy()[idx])
    assert np.array_equal(np.load(os.path.join(a, "gas3_g_point.npy")), res["gas_g_point"][3].numpy()[idx])
    assert np.load(os.path.join(a, "summary.npy"))[0] == 6


def test_dump_refuses_more_than_the_limit(tmp_path):
    with pytest.raises(RuntimeError):
        bench.dump_arrays(str(tmp_path), {"big": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})


def test_plain_run_is_lean_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "d"
