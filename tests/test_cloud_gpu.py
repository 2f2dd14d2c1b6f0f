"""The cloud pseudo-gas of the shortwave chain: the sorting variable of reorder_cloud_spectrum (reorder_cloud_spectrum.cpp:111-123)
against a numpy restatement bit for bit, the bin/reorder_cloud_spectrum tool against the host mirror and a numpy stable sort, the
cloud partition (find_g_points.cpp:586-636) against a numpy restatement, and find_g_points with `cloud <name>` through the tools
(one and two processes) up to create_look_up_table."""
import os

import numpy as np
import pytest
from scipy.io import netcdf_file

from cloud_cases import abs_inf_numpy, partition_numpy, stable_ranks
from ecckd_amd import synthetic as syn
from test_cli_gpu import _nc, _run_ranks, _write_columns_from, run_tool

pytestmark = pytest.mark.gpu

GOLDEN_MIE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mie_droplet_scattering.nc")


def write_mie(path, wn, ssa, g):
    w = netcdf_file(str(path), "w", version=2)
    w.createDimension("effective_radius", ssa.shape[0])
    w.createDimension("wavenumber", wn.size)
    w.createVariable("effective_radius", "f", ("effective_radius",))[:] = 1e-6 * np.arange(1, ssa.shape[0] + 1)
    w.createVariable("wavenumber", "f", ("wavenumber",))[:] = wn
    w.createVariable("single_scattering_albedo", "f", ("effective_radius", "wavenumber"))[:] = ssa
    w.createVariable("asymmetry_factor", "f", ("effective_radius", "wavenumber"))[:] = g
    w.close()


def write_grid(path, wn, ssi=None):
    w = netcdf_file(str(path), "w", version=2)
    w.createDimension("wavenumber", wn.size)
    w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
    if ssi is not None:
        w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = ssi
        w.createVariable("total_solar_irradiance", "d", ())[...] = ssi.sum()
    w.close()


def read_mie(path):
    f = netcdf_file(str(path), "r", mmap=False)
    v = f.variables
    out = (v["wavenumber"][:].astype(np.float64), v["single_scattering_albedo"][:].astype(np.float64),
           v["asymmetry_factor"][:].astype(np.float64))
    f.close()
    return out


def test_sorting_variable_bit_for_bit(ctx):
    import torch
    from ecckd_amd import api
    x, ssa, g = read_mie(GOLDEN_MIE)
    assert ssa.shape == (10, x.size)
    # denser than the knots, the knots themselves, and beyond both ends (extrapolation)
    xi = np.unique(np.concatenate([np.linspace(x[0] - 2.0, x[-1] + 3.0, 20011), x]))
    for isize in range(ssa.shape[0]):
        exp = abs_inf_numpy(x, ssa[isize], g[isize], xi)
        got = api.cloud_sorting_variable(ctx, x, ssa[isize], g[isize], torch.as_tensor(xi, device=ctx.device)).cpu().numpy()
        assert np.isfinite(exp).all()
        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), (isize, np.max(np.abs(got - exp)))
    # a Mie grid that is not strictly ascending
    with pytest.raises(api.EcckdError) as e:
        api.cloud_sorting_variable(ctx, x[::-1], ssa[0], g[0], torch.as_tensor(xi, device=ctx.device))
    assert e.value.code == 147


@pytest.mark.parametrize("ext", ["nc", "h5"])
def test_reorder_cloud_spectrum_tool(ctx, tmp_path, ext):
    from ecckd_amd import ncio, pipeline
    d = tmp_path
    x, ssa, g = read_mie(GOLDEN_MIE)
    rng = np.random.default_rng(7)
    wn = np.sort(np.unique(np.linspace(3.0, 33.0, 30000) + rng.uniform(-1e-4, 1e-4, 30000)))
    write_grid(d / "grid.nc", wn)
    os.symlink(GOLDEN_MIE, d / "mie.nc")
    dwn = np.empty_like(wn)
    dwn[1:-1] = 0.5 * (wn[2:] - wn[:-2])
    dwn[0], dwn[-1] = 0.5 * dwn[1], 0.5 * dwn[-2]
    cases = [(3, None, None), (8, [0.0, 8.0, 12.5, 20.0, 26.0], [8.0, 12.5, 20.0, 26.0, 40.0])]
    for isize, b1, b2 in cases:
        out = f"order_{isize}_cloud.{ext}"
        args = ["input=mie.nc", f"isize={isize}", "wavenumber_input=grid.nc", f"output={out}"]
        if b1 is not None:
            args += ["wavenumber1=" + " ".join(map(str, b1)), "wavenumber2=" + " ".join(map(str, b2))]
        r = run_tool("reorder_cloud_spectrum", *args, cwd=d)
        assert r.returncode == 0, r.stderr + r.stdout
        if ext == "h5":
            import h5_fixture
            if h5_fixture.available():
                assert open(d / out, "rb").read(8) == b"\x89HDF\r\n\x1a\n"
        got = ncio.read_order(d / out)
        exp = pipeline.reorder_cloud_spectrum(ctx, GOLDEN_MIE, d / "grid.nc", d / f"mirror_{isize}.nc", isize, b1, b2)
        key = abs_inf_numpy(x, ssa[isize], g[isize], wn)
        assert np.array_equal(exp["sorting_variable"], key)
        if b1 is None:
            b1n, b2n = [max(0.0, wn[0] - dwn[0])], [wn[-1] + dwn[-1]]
        else:
            b1n, b2n = b1, b2
        nb = len(b1n)
        iband = np.full(wn.size, -1, dtype=np.int16)
        bb, be = [], []
        for b in range(nb):
            m = (wn >= b1n[b]) & ((wn < b2n[b]) if b < nb - 1 else (wn <= b2n[b]))
            iband[m] = b
            idx = np.nonzero(m)[0]
            bb.append(idx[0]); be.append(idx[-1])
        rank = stable_ranks(key, bb, be)
        assert np.array_equal(got["rank"], rank) and np.array_equal(exp["rank"], rank)
        assert np.array_equal(got["band_number"], iband) and np.array_equal(exp["band_number"], iband)
        assert np.array_equal(got["sorting_variable"], key.astype(np.float32).astype(np.float64))
        assert np.array_equal(got["wavenumber"], wn)
        # the bounds clamped to the data (:156-161), as FLOAT
        c1, c2 = np.array(b1n, dtype=np.float64), np.array(b2n, dtype=np.float64)
        c1[0], c2[-1] = max(wn[0], c1[0]), min(wn[-1], c2[-1])
        assert np.array_equal(got["wavenumber1_band"], c1.astype(np.float32).astype(np.float64))
        assert np.array_equal(got["wavenumber2_band"], c2.astype(np.float32).astype(np.float64))
        assert got["molecule"] == "cloud"
        with ncio.NcFile(d / out) as f:
            assert "cloud absorptance" in f.att_text("comment", "sorting_variable")
            assert not f.exist("column_optical_depth")


def test_reorder_cloud_spectrum_exit_codes(tmp_path):
    d = tmp_path
    write_grid(d / "grid.nc", np.linspace(5.0, 30.0, 100))
    os.symlink(GOLDEN_MIE, d / "mie.nc")
    full = ["input=mie.nc", "isize=0", "wavenumber_input=grid.nc", "output=o.nc"]
    messages = ['"input" file not specified', '"isize" not specified', '"wavenumber_input" file not specified', '"output" file not specified']
    for k, msg in enumerate(messages):
        r = run_tool("reorder_cloud_spectrum", *(full[:k] + full[k + 1:]), cwd=d)
        assert r.returncode == 147 and msg in r.stderr, (k, r.stderr)
    for isize in (-1, 10):
        r = run_tool("reorder_cloud_spectrum", "input=mie.nc", f"isize={isize}", "wavenumber_input=grid.nc", "output=o.nc", cwd=d)
        assert r.returncode == 147 and "isize" in r.stderr, r.stderr
    assert not (d / "o.nc").exists()


def _partition_case(seed, nwav=60000, bands=(0, 9000, 21000, 40000, 52000, 60000)):
    rng = np.random.default_rng(seed)
    t = np.linspace(0, 1, nwav)
    sv = 0.5 + 0.3 * np.sin(40 * t + rng.uniform(0, 6)) + 0.2 * rng.standard_normal(nwav) * np.abs(np.sin(7 * t))
    ssi = rng.uniform(0.2, 1.0, nwav) * (1.0 + np.sin(3 * t)) + 1e-3
    iband = np.full(nwav, -1, dtype=np.int16)
    begin, end = [], []
    for b in range(len(bands) - 1):
        lo, hi = bands[b] + (50 if b == 0 else 0), bands[b + 1] - (70 if b == len(bands) - 2 else 0)   # points outside every band
        iband[lo:hi] = b
        begin.append(lo); end.append(hi - 1)
    return ssi, stable_ranks(sv, begin, end), sv, iband, begin, end


@pytest.mark.parametrize("max_range", [0.26, 0.34, 0.05])
def test_cloud_partition_against_numpy(ctx, max_range):
    import torch
    from ecckd_amd import api
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)
    for seed in (1, 2):
        ssi, rank, sv, iband, begin, end = _partition_case(seed)
        exp, margin = partition_numpy(ssi, rank, sv, iband, len(begin), max_range)
        # no running sum within rounding of a boundary: the blocked scan cannot move a point
        assert margin > 1e-10
        got = api.cloud_partition(ctx, dev(ssi), dev(rank), dev(sv), begin, end, max_range)
        assert list(got["n_g_points"]) == exp["n_g_points"]
        assert sum(exp["n_g_points"]) > len(begin)
        for k in ("band_number", "rank1", "rank2", "error"):
            assert np.array_equal(got[k], np.array(exp[k])), k
        assert np.allclose(got["median"], exp["median"], rtol=1e-12, atol=0.0)


def test_cloud_partition_errors(ctx):
    import torch
    from ecckd_amd import api
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)
    ssi, rank, sv, iband, begin, end = _partition_case(3)
    bad = ssi.copy()
    bad[5] = -1e-3                        # outside every band: still refused
    with pytest.raises(api.EcckdError) as e:
        api.cloud_partition(ctx, dev(bad), dev(rank), dev(sv), begin, end, 0.26)
    assert e.value.code == 147 and "negative" in e.value.message
    # one point of band 0 carries nearly all its irradiance: a g point in the middle holds nothing
    spike = ssi.copy()
    ib, ie = begin[0], end[0]
    mid = ib + int(np.nonzero(rank[ib:ie + 1] == ib + (ie - ib) // 2)[0][0])
    spike[mid] = 1e6
    with pytest.raises(api.EcckdError) as e:
        api.cloud_partition(ctx, dev(spike), dev(rank), dev(sv), begin, end, 0.05)
    assert e.value.code == 148 and "Band 0, g point" in e.value.message


def _sw_case(d, nwav=8000, lo=250.0, hi=50000.0):
    nlay = 16
    p1 = syn.pressure_grid(nlay)
    wn, dwn = syn.wavenumber_grid(nwav, lo, hi)
    ssi = syn.solar_spectral_irradiance(wn, dwn)
    write_grid(d / "ssi.nc", wn, ssi)
    t0 = syn.temperature_profile(p1)
    base = {"h2o": (syn.optical_depth(np, p1, wn, syn.SEED_BASE + 81, nlines=60, column_scale=3.0, dtype="float32", lo=lo, hi=hi), 5e-3),
            "o3": (syn.optical_depth(np, p1, wn, syn.SEED_BASE + 83, nlines=30, column_scale=0.8, dtype="float32", lo=lo, hi=hi), 1e-6)}
    for g, (od, vmr) in base.items():
        _write_columns_from(d / f"present_{g}.nc", g, p1, [t0], wn, od, vmr)
        _write_columns_from(d / f"ideal_{g}.nc", g, p1, [t0 - 20.0, t0, t0 + 20.0], wn, od, vmr)
    mwn, mssa, mg = syn.mie_table(5)
    write_mie(d / "mie.nc", mwn, mssa, mg)
    return wn, ssi, p1


GASES_CFG = ("ssi ssi.nc\nheating_rate_tolerance 0.06\nmax_iterations 30\naveraging_method total-transmission\ngases h2o o3\n"
             "\\begin h2o\n input present_h2o.nc\n reordering_input order_h2o.{ext}\n background_input present_o3.nc\n\\end h2o\n"
             "\\begin o3\n input present_o3.nc\n reordering_input order_o3.{ext}\n background_input present_h2o.nc\n\\end o3\n")
CLOUD_CFG = "cloud liquidcloud\n\\begin liquidcloud\n reordering_input {order}\n max_reflectance_range {rng}\n\\end liquidcloud\n"


def test_find_g_points_with_cloud(ctx, tmp_path):
    from ecckd_amd import pipeline
    d = tmp_path
    wn, ssi, p1 = _sw_case(d)
    b1, b2 = "250 2500 10000 25000", "2500 10000 25000 50000"
    for g in ("h2o", "o3"):
        r = run_tool("reorder_spectrum", f"input=present_{g}.nc", f"output=order_{g}.nc", "ssi=ssi.nc", f"wavenumber1={b1}", f"wavenumber2={b2}", cwd=d)
        assert r.returncode == 0, r.stderr
    r = run_tool("reorder_cloud_spectrum", "input=mie.nc", "isize=1", "wavenumber_input=ssi.nc", "output=order_cloud.nc",
                 f"wavenumber1={b1}", f"wavenumber2={b2}", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    (d / "g.cfg").write_text(GASES_CFG.format(ext="nc") + CLOUD_CFG.format(order="order_cloud.nc", rng=0.1))
    r = run_tool("find_g_points", "g.cfg", "output=gpoints.nc", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    f = _nc(d / "order_h2o.nc")
    bb1, bb2 = f.variables["wavenumber1_band"][:].astype(np.float64), f.variables["wavenumber2_band"][:].astype(np.float64)
    f.close()
    specs = [dict(name="h2o", input=d / "present_h2o.nc", reordering_input=d / "order_h2o.nc", background=[dict(path=d / "present_o3.nc")]),
             dict(name="o3", input=d / "present_o3.nc", reordering_input=d / "order_o3.nc", background=[dict(path=d / "present_h2o.nc")])]
    cloud = dict(name="liquidcloud", reordering_input=d / "order_cloud.nc", max_reflectance_range=0.1)
    exp = pipeline.find_g_points(ctx, specs, bb1, bb2, 0.06, averaging_method="total-transmission", max_iterations=30, ssi=ssi, cloud=cloud)
    f = _nc(d / "gpoints.nc")
    v = f.variables
    assert f.constituent_id.split() == [b"liquidcloud", b"h2o", b"o3"]
    assert int(v["n_gases"].getValue()) == 3
    c = exp["gases"][0]
    assert c["name"] == "liquidcloud" and sum(c["n_g_points"]) > 4
    for k in ("n_g_points", "band_number", "rank1", "rank2", "g_min", "g_max", "g_point"):
        assert np.array_equal(v["liquidcloud_" + k][:], np.asarray(c[k])), k
    for k in ("error", "sorting_variable"):
        assert np.array_equal(v["liquidcloud_" + k][:], np.asarray(c[k], dtype=np.float32)), k
    assert np.all(np.asarray(c["sorting_variable"]) < -1.0)
    assert np.array_equal(v["g_point"][:], exp["g_point"])
    f.close()
    # two processes: the same file
    _run_ranks(2, "g.cfg", "output=gpoints_2.nc", "part_timeout=300", cwd=d)
    from test_cli_gpu import _same_files
    _same_files(d / "gpoints.nc", d / "gpoints_2.nc")
    # a cloud ordering on another grid
    write_grid(d / "ssi_other.nc", wn[::2], ssi[::2])
    r = run_tool("reorder_cloud_spectrum", "input=mie.nc", "isize=1", "wavenumber_input=ssi_other.nc", "output=order_other.nc",
                 f"wavenumber1={b1}", f"wavenumber2={b2}", cwd=d)
    assert r.returncode == 0, r.stderr
    (d / "other.cfg").write_text(GASES_CFG.format(ext="nc") + CLOUD_CFG.format(order="order_other.nc", rng=0.1))
    r = run_tool("find_g_points", "other.cfg", "output=gpoints_other.nc", cwd=d)
    assert r.returncode == 147 and "liquidcloud" in r.stderr, r.stderr
    # the longwave (no ssi) refuses the cloud with the reference's message
    (d / "lw.cfg").write_text(GASES_CFG.format(ext="nc").replace("ssi ssi.nc\n", "") + CLOUD_CFG.format(order="order_cloud.nc", rng=0.1))
    r = run_tool("find_g_points", "lw.cfg", "output=gpoints_lw.nc", cwd=d)
    assert r.returncode == 147 and "Don't yet know how to sort cloud properties in the longwave" in r.stderr, r.stderr
    # no reordering_input
    (d / "noorder.cfg").write_text(GASES_CFG.format(ext="nc") + "cloud liquidcloud\n")
    r = run_tool("find_g_points", "noorder.cfg", "output=gpoints_x.nc", cwd=d)
    assert r.returncode == 147 and "No reordering_input found" in r.stderr, r.stderr


def test_sw_chain_with_cloud(ctx, tmp_path):
    """reorder_spectrum (gases) -> reorder_cloud_spectrum (*_cloud.h5, as test/reorder_spectrum_sw.sh names it) -> find_g_points
    with the cloud -> create_look_up_table."""
    d = tmp_path
    _sw_case(d)
    b1, b2 = "250 10000", "10000 50000"
    for g in ("h2o", "o3"):
        r = run_tool("reorder_spectrum", f"input=present_{g}.nc", f"output=order_{g}.h5", "ssi=ssi.nc", f"wavenumber1={b1}", f"wavenumber2={b2}", cwd=d)
        assert r.returncode == 0, r.stderr
    r = run_tool("reorder_cloud_spectrum", "input=mie.nc", "isize=2", "wavenumber_input=ssi.nc", "output=sw_order_test_cloud.h5",
                 f"wavenumber1={b1}", f"wavenumber2={b2}", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    ng = {}
    for tag, extra in (("plain", ""), ("cloud", CLOUD_CFG.format(order="sw_order_test_cloud.h5", rng=0.34))):
        (d / f"g_{tag}.cfg").write_text(GASES_CFG.format(ext="h5") + extra)
        r = run_tool("find_g_points", f"g_{tag}.cfg", f"output=gpoints_{tag}.h5", cwd=d)
        assert r.returncode == 0, r.stderr + r.stdout
        (d / f"lut_{tag}.cfg").write_text(
            f"input gpoints_{tag}.h5\noutput ckd_{tag}.nc\nssi ssi.nc\naveraging_method transmission-3\ngases h2o o3\n"
            "\\begin h2o\n conc_dependence linear\n input ideal_h2o.nc\n\\end h2o\n"
            "\\begin o3\n conc_dependence linear\n input ideal_o3.nc\n\\end o3\n")
        r = run_tool("create_look_up_table", f"lut_{tag}.cfg", cwd=d)
        assert r.returncode == 0, r.stderr + r.stdout
        f = _nc(d / f"ckd_{tag}.nc")
        ng[tag] = f.dimensions["g_point"]
        f.close()
    assert ng["cloud"] >= ng["plain"], ng
