"""bin/merge_spectra and bin/lw_spectra as a user of the reference would run them (`exe [key=value ...] [file.cfg]` on
NetCDF files): variables, dimensions, attributes and values of their output files, exit codes.
The tools' files are also compared bit for bit with the host mirrors pipeline.merge_spectra / pipeline.lw_spectra, which make
the same library calls in the same order."""
import os
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

from ecckd_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
NCOL, NLAY, NWAV = 3, 12, 4003


def run_tool(name, *args, cwd=None):
    exe = os.path.join(BIN, name)
    if not os.path.exists(exe):                      # a fresh checkout: build the library and the tools first
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    assert os.path.exists(exe), f"{exe} not built (python -c 'import __graft_entry__ as g; g.build()')"
    return subprocess.run([exe, *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=600)


def _nc(path):
    return netcdf_file(str(path), "r", mmap=False)


def _make_files(d):
    """Two gas files of NCOL columns; -> pressure_hl, temperature_hl[c], wavenumber, derived d_wavenumber, {gas: od[c]}"""
    p = syn.pressure_grid(NLAY)
    t0 = syn.temperature_profile(p)
    t = np.stack([t0 + 3.0 * c for c in range(NCOL)])
    wn, _ = syn.wavenumber_grid(NWAV)
    ods = {}
    for g, (seed, scale, vmr) in {"h2o": (41, 30.0, 5e-3), "co2": (43, 8.0, 4e-4)}.items():
        od0 = syn.optical_depth(np, p, wn, syn.SEED_BASE + seed, nlines=40, column_scale=scale, dtype="float32")
        od = np.stack([(od0 * np.float32(1.0 + 0.25 * c)).astype(np.float32) for c in range(NCOL)])
        w = netcdf_file(str(d / f"{g}.nc"), "w", version=2)
        for name, n in (("column", NCOL), ("half_level", NLAY + 1), ("level", NLAY), ("wavenumber", NWAV)):
            w.createDimension(name, n)
        w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p, (NCOL, 1))
        w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = t
        w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
        w.createVariable("mole_fraction_fl", "d", ("column", "level"))[:] = np.full((NCOL, NLAY), vmr)
        w.createVariable("optical_depth", "f", ("column", "level", "wavenumber"))[:] = od
        w.createVariable("reference_surface_mole_fraction", "d", ())[...] = vmr
        w.constituent_id = g
        w.close()
        ods[g] = od
    dwn = np.zeros(NWAV)                              # read_spectrum.cpp:55-65: the files carry no d_wavenumber
    dwn[1:-1] = 0.5 * (wn[2:] - wn[:-2])
    dwn[0], dwn[-1] = 0.5 * dwn[1], 0.5 * dwn[-2]
    return p, t, wn, dwn, ods


def _merged(ods):
    """float64 sum of the two gases, co2 scaled by 2.5 (the `scaling` key)"""
    return ods["h2o"].astype(np.float64) + 2.5 * ods["co2"].astype(np.float64)


def test_merge_spectra(ctx, tmp_path):
    """6."""
    p, t, wn, dwn, ods = _make_files(tmp_path)
    out = tmp_path / "merged.nc"
    r = run_tool("merge_spectra", f"append_path={tmp_path}", "input=h2o.nc co2.nc", "scaling=1.0 2.5", f"output={out}")
    assert r.returncode == 0, r.stderr
    f = _nc(out)
    assert f.dimensions == {"column": NCOL, "level": NLAY, "half_level": NLAY + 1, "wavenumber": NWAV}
    assert f.variables["optical_depth"].data.dtype == np.dtype(">f4") and f.variables["optical_depth"].dimensions == ("column", "level", "wavenumber")
    assert f.variables["wavenumber"].data.dtype == np.dtype(">f8")
    assert f.variables["pressure_hl"].data.dtype == np.dtype(">f4") and f.variables["pressure_hl"].dimensions == ("column", "half_level")
    assert f.variables["temperature_hl"].data.dtype == np.dtype(">f4")
    assert f.variables["optical_depth"].long_name == b"Layer optical depth"
    assert f.variables["wavenumber"].units == b"cm-1" and f.variables["pressure_hl"].units == b"Pa"
    # read_merged_spectrum joins the files' constituent_id with a blank (read_merged_spectrum.cpp:114); a comma inside one
    # file's `molecules` attribute is what merge_spectra.cpp:118-121 turns into ", "
    assert f.molecule == b"hybrid:h2o co2"
    assert f.title == b"Merged spectral optical depth profiles of H2O CO2"
    assert b"merge_spectra" in f.history
    cfg = f.config.decode()
    assert "input" in cfg and "h2o.nc" in cfg and "scaling" in cfg and "output" in cfg
    expected = _merged(ods).astype(np.float32)
    for c in range(NCOL):
        assert np.array_equal(f.variables["optical_depth"][c], expected[c])
        assert np.array_equal(f.variables["temperature_hl"][c], t[c].astype(np.float32))
    assert np.array_equal(f.variables["wavenumber"][:], wn)
    # the host mirror: same calls, same bits; its own file through ncio holds the same variables
    from ecckd_amd import pipeline
    m = pipeline.merge_spectra(ctx, [tmp_path / "h2o.nc", tmp_path / "co2.nc"], tmp_path / "mirror.nc", scaling=[1.0, 2.5])
    g = _nc(tmp_path / "mirror.nc")
    assert m["optical_depth"].dtype == np.float32 and np.array_equal(m["optical_depth"], f.variables["optical_depth"][:])
    for name in ("optical_depth", "pressure_hl", "temperature_hl", "wavenumber"):
        assert np.array_equal(g.variables[name][:], f.variables[name][:]) and g.variables[name].dimensions == f.variables[name].dimensions
    assert g.title == f.title and g.molecule == f.molecule
    # a file whose `molecules` attribute lists two gases with a comma: ", " in the title, the attribute as it is in `molecule`
    w = netcdf_file(str(tmp_path / "pair.nc"), "w", version=2)
    for name, n in (("column", 1), ("half_level", NLAY + 1), ("level", NLAY), ("wavenumber", NWAV)):
        w.createDimension(name, n)
    w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = p[None]
    w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = t[:1]
    w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
    w.createVariable("optical_depth", "f", ("column", "level", "wavenumber"))[:] = ods["h2o"][:1]
    w.molecules = "h2o,co2"
    w.close()
    r = run_tool("merge_spectra", f"input={tmp_path / 'pair.nc'}", f"output={tmp_path / 'pair_out.nc'}")
    assert r.returncode == 0, r.stderr
    h = _nc(tmp_path / "pair_out.nc")
    assert h.title == b"Merged spectral optical depth profiles of H2O, CO2" and h.molecule == b"hybrid:h2o,co2"
    assert np.array_equal(h.variables["optical_depth"][0], ods["h2o"][0])
    # exit codes: PARAMETER_ERROR without output / input, 139 for a file that is not there
    assert run_tool("merge_spectra", f"append_path={tmp_path}", "input=h2o.nc").returncode == 147
    assert run_tool("merge_spectra", f"output={out}").returncode == 147
    assert run_tool("merge_spectra", f"append_path={tmp_path}", "input=absent.nc", f"output={tmp_path / 'x.nc'}").returncode == 139


def _oracle_column(oracle, t_hl, wn, dwn, od):
    planck = oracle.planck_function(t_hl, wn, dwn)
    return oracle.radiative_transfer_lw(planck, od, np.ones(wn.size), planck[-1])


F32 = 2.0 ** -23        # FLOAT precision: the files hold FLOAT (half an ulp of rounding, 1e-10 of the device against the oracle)


def test_lw_spectra_per_wavenumber(ctx, oracle, tmp_path):
    """7."""
    from ecckd_amd import ncio
    p, t, wn, dwn, ods = _make_files(tmp_path)
    out = tmp_path / "spectra.nc"
    args = (f"append_path={tmp_path}", "input=h2o.nc co2.nc", "scaling=1.0 2.5")
    r = run_tool("lw_spectra", *args, f"output={out}")
    assert r.returncode == 0, r.stderr
    with ncio.NcFile(out) as g:                       # the repository's classic reader: `column` is unlimited, 3 records
        assert g.dim("column") == NCOL and g.dim("wavenumber") == NWAV and g.dim("gas") == 2
    raw = out.read_bytes()
    assert int.from_bytes(raw[4:8], "big") == NCOL    # numrecs
    f = _nc(out)
    assert f.dimensions["column"] is None and f.dimensions["wavenumber"] == NWAV and "g_point" not in f.dimensions
    assert f.variables["spectral_flux_dn_lw"].dimensions == ("column", "half_level", "wavenumber")
    assert f.variables["optical_depth"].dimensions == ("column", "level", "wavenumber")
    assert f.variables["vmr_fl"].dimensions == ("column", "gas", "level")
    assert f.variables["flux_dn_lw"].long_name == b"Upwelling longwave flux"        # as the reference has it
    assert f.variables["spectral_flux_dn_lw"].long_name == b"Downwelling longwave spectral flux"
    assert f.variables["vmr_fl"].comment == b'The gases are listed in the global attribute "molecules".'
    assert f.molecules == b"h2o co2" and b"lw_spectra" in f.history and b"input" in f.config
    assert f.variables["wavenumber"].data.dtype == np.dtype(">f8") and f.variables["flux_up_lw"].data.dtype == np.dtype(">f4")
    merged = _merged(ods)
    for c in range(NCOL):
        fdn, fup = _oracle_column(oracle, t[c], wn, dwn, merged[c])
        assert np.allclose(f.variables["flux_dn_lw"][c], fdn.sum(1), rtol=F32, atol=0.0)
        assert np.allclose(f.variables["flux_up_lw"][c], fup.sum(1), rtol=F32, atol=0.0)
        assert np.allclose(f.variables["spectral_flux_up_lw"][c], fup, rtol=F32, atol=1e-45)
        assert np.allclose(f.variables["spectral_flux_dn_lw"][c], fdn, rtol=F32, atol=1e-45)
        assert np.array_equal(f.variables["optical_depth"][c], merged[c].astype(np.float32))
        assert np.allclose(f.variables["vmr_fl"][c, 0], 5e-3, rtol=F32)
    # iprofile = 1: exactly one record, equal to record 1 of the full run
    one = tmp_path / "one.nc"
    r = run_tool("lw_spectra", *args, "iprofile=1", f"output={one}")
    assert r.returncode == 0, r.stderr
    h = _nc(one)
    assert h.variables["flux_dn_lw"].shape[0] == 1
    for name in ("pressure_hl", "temperature_hl", "vmr_fl", "flux_dn_lw", "flux_up_lw", "optical_depth", "spectral_flux_dn_lw",
                 "spectral_flux_up_lw"):
        assert np.array_equal(h.variables[name][0], f.variables[name][1]), name
    assert run_tool("lw_spectra", *args).returncode == 147                       # no output
    # a *.h5 output (NetCDF-4, `column` unlimited, optical_depth and wavenumber deflated) reads back identically through the
    # repository's HDF5 reader
    h5 = tmp_path / "spectra.h5"
    r = run_tool("lw_spectra", *args, f"output={h5}")
    assert r.returncode == 0, r.stderr
    assert h5.read_bytes()[:8] == b"\x89HDF\r\n\x1a\n"
    names = ("pressure_hl", "temperature_hl", "vmr_fl", "flux_dn_lw", "flux_up_lw", "optical_depth", "spectral_flux_dn_lw",
             "spectral_flux_up_lw", "wavenumber")
    with ncio.NcFile(h5) as a, ncio.NcFile(out) as b:
        assert a.dim("column") == NCOL and a.dim("wavenumber") == NWAV and a.dim("gas") == 2
        for name in names:
            assert a.var_info(name) == b.var_info(name), name
            assert np.array_equal(a.read(name), b.read(name)), name
        assert a.att_text("long_name", "flux_dn_lw") == "Upwelling longwave flux" and a.att_text("molecules") == "h2o co2"
    # the host mirror, bit for bit (the file holds the FLOAT casts of its arrays)
    from ecckd_amd import pipeline
    m = pipeline.lw_spectra(ctx, [tmp_path / "h2o.nc", tmp_path / "co2.nc"], tmp_path / "mirror.nc", scaling=[1.0, 2.5])
    g = _nc(tmp_path / "mirror.nc")
    for name in names[:-1]:
        assert np.array_equal(m[name].astype(np.float32), f.variables[name][:]), name
        assert np.array_equal(g.variables[name][:], f.variables[name][:]) and g.variables[name].dimensions == f.variables[name].dimensions
    assert g.dimensions["column"] is None and g.molecules == f.molecules


def test_lw_spectra_per_g_point(ctx, oracle, tmp_path):
    """8."""
    p, t, wn, dwn, ods = _make_files(tmp_path)
    ng = 9
    rng = np.random.default_rng(5)
    g_point = rng.integers(0, ng, size=NWAV).astype(np.int32)
    g_point[rng.random(NWAV) < 0.05] = -1
    w = netcdf_file(str(tmp_path / "gpoints.nc"), "w", version=2)
    w.createDimension("wavenumber", NWAV)
    w.createVariable("g_point", "i", ("wavenumber",))[:] = g_point
    w.close()
    out = tmp_path / "gspectra.nc"
    r = run_tool("lw_spectra", f"append_path={tmp_path}", "input=h2o.nc co2.nc", "scaling=1.0 2.5", "gpoints=gpoints.nc", f"output={out}")
    assert r.returncode == 0, r.stderr
    f = _nc(out)
    assert f.dimensions["g_point"] == ng and f.dimensions["column"] is None
    assert "wavenumber" not in f.variables and "wavenumber" not in f.dimensions
    assert f.variables["spectral_flux_up_lw"].dimensions == ("column", "half_level", "g_point")
    merged = _merged(ods)
    for c in range(NCOL):
        fdn, fup = _oracle_column(oracle, t[c], wn, dwn, merged[c])
        gdn = np.stack([fdn[:, g_point == g].sum(1) for g in range(ng)], axis=1)
        gup = np.stack([fup[:, g_point == g].sum(1) for g in range(ng)], axis=1)
        assert np.allclose(f.variables["spectral_flux_dn_lw"][c], gdn, rtol=F32, atol=0.0)
        assert np.allclose(f.variables["spectral_flux_up_lw"][c], gup, rtol=F32, atol=0.0)
        assert np.allclose(f.variables["flux_dn_lw"][c], fdn.sum(1), rtol=F32, atol=0.0)      # every wavenumber, -1 included
        assert np.allclose(f.variables["flux_up_lw"][c], fup.sum(1), rtol=F32, atol=0.0)
        t_fl = 0.5 * (t[c][:-1] * p[:-1] + t[c][1:] * p[1:]) / (0.5 * (p[:-1] + p[1:]))
        planck_fl = oracle.planck_function(t_fl, wn, dwn)
        oma, _, _, ne = oracle.average_optical_depth_to_g_point(ng, 0.0, p, g_point, merged[c], planck_fl, "transmission")
        # test_create_lut_gpu.py: rtol 1e-10 for this method in double; the file holds FLOAT
        assert np.allclose(f.variables["optical_depth"][c], oma, rtol=F32, atol=1e-45)
    # the tool's file and the host mirror's arrays: bit for bit; the mirror's doubles against the oracle at the tolerance
    # test_create_lut_gpu.py uses for this method
    from ecckd_amd import pipeline
    m = pipeline.lw_spectra(ctx, [tmp_path / "h2o.nc", tmp_path / "co2.nc"], scaling=[1.0, 2.5], g_point=g_point)
    for name in ("pressure_hl", "temperature_hl", "vmr_fl", "flux_dn_lw", "flux_up_lw", "optical_depth", "spectral_flux_dn_lw",
                 "spectral_flux_up_lw"):
        assert np.array_equal(m[name].astype(np.float32), f.variables[name][:]), name
    for c in range(NCOL):
        t_fl = 0.5 * (t[c][:-1] * p[:-1] + t[c][1:] * p[1:]) / (0.5 * (p[:-1] + p[1:]))
        oma, _, _, ne = oracle.average_optical_depth_to_g_point(ng, 0.0, p, g_point, merged[c], oracle.planck_function(t_fl, wn, dwn),
                                                                "transmission")
        assert np.allclose(m["optical_depth"][c], oma, rtol=1e-10, atol=1e-300)
