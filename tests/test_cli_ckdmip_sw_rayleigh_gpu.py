"""bin/ckdmip_sw with Rayleigh scattering switched on: --rayleigh FILE in the default mode and --ckd --rayleigh-scattering,
each against the library call it makes, and the combinations the tool refuses."""
import numpy as np
import pytest
from scipy.io import netcdf_file

from ecckd_amd import synthetic as syn
from test_cli_gpu import _nc, run_tool

pytestmark = pytest.mark.gpu

PARAMETER_ERROR = 147
NCOL, NLAY, NWAV = 2, 3, 300
LO, HI = 250.0, 50000.0
MU0 = np.array([0.3, 0.5])


def _write_spectrum_file(path, gas, p1, wn, od, vmr):
    """od (ncol, nlay, nwav), written as FLOAT like the CKDMIP spectra."""
    ncol, nlay = od.shape[:2]
    w = netcdf_file(str(path), "w", version=2)
    for d, n in (("column", ncol), ("half_level", nlay + 1), ("level", nlay), ("wavenumber", wn.size)):
        w.createDimension(d, n)
    w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p1, (ncol, 1))
    w.createVariable("temperature_hl", "d", ("column", "half_level"))[:] = np.tile(syn.temperature_profile(p1), (ncol, 1))
    w.createVariable("wavenumber", "d", ("wavenumber",))[:] = wn
    w.createVariable("mole_fraction_fl", "d", ("column", "level"))[:] = np.full((ncol, nlay), vmr)
    w.createVariable("optical_depth", "f", ("column", "level", "wavenumber"))[:] = od.astype(np.float32)
    w.createVariable("reference_surface_mole_fraction", "d", ())[...] = vmr
    w.constituent_id = gas
    w.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckdmip_sw_rayleigh")
    rng = np.random.default_rng(17)
    p1 = syn.pressure_grid(NLAY)
    wn, dwn = syn.wavenumber_grid(NWAV, LO, HI)
    ssi = syn.solar_spectral_irradiance(wn, dwn)
    w = netcdf_file(str(d / "ssi.nc"), "w", version=2)
    w.createDimension("wavenumber", NWAV)
    w.createVariable("solar_spectral_irradiance", "d", ("wavenumber",))[:] = ssi
    w.close()
    od = {g: np.exp(rng.uniform(np.log(1e-4), np.log(3.0), (NCOL, NLAY, NWAV))).astype(np.float32) for g in ("h2o", "o3")}
    ray = (0.3 * (wn / HI) ** 4 * rng.uniform(0.5, 1.5, (NCOL, NLAY, 1))).astype(np.float32)     # ~ wavenumber^4, per layer and column
    _write_spectrum_file(d / "h2o.nc", "h2o", p1, wn, od["h2o"], 5e-3)
    _write_spectrum_file(d / "o3.nc", "o3", p1, wn, od["o3"], 1e-6)
    _write_spectrum_file(d / "rayleigh.nc", "rayleigh", p1, wn, ray, 1.0)
    nam = ("&shortwave_config\noptical_depth_name = \"optical_depth\",\nsurf_albedo = 0.15,\nuse_mu0_dimension = true,\n"
           "cos_solar_zenith_angle(1:2) = 0.3, 0.5,\nnspectralstride = 1,\nBOUNDARY"
           "band_wavenumber1(1:2) = 250, 10000,\nband_wavenumber2(1:2) = 10000, 50000,\n/\n")
    (d / "sw.nam").write_text(nam.replace("BOUNDARY", ""))
    (d / "sw_b.nam").write_text(nam.replace("BOUNDARY", "do_write_spectral_boundary_fluxes = true,\n"))
    return dict(d=d, p1=p1, wn=wn, ssi=ssi, od=od, ray=ray)


def test_default_mode_with_a_rayleigh_spectrum(ctx, files):
    import torch
    from ecckd_amd import api
    d, wn, ssi = files["d"], files["wn"], files["ssi"]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)
    r = run_tool("ckdmip_sw", "--config", "sw_b.nam", "--scenario", "present", "--ssi", "ssi.nc", "--rayleigh", "rayleigh.nc", "h2o.nc",
                 "--scale", "0.5", "o3.nc", "--output", "lbl_ray.nc", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    f = _nc(d / "lbl_ray.nc")
    assert f.rayleigh_scattering == b"two-stream" and f.constituent_id == b"h2o o3" and f.scenario == b"present"
    assert np.allclose(f.variables["mu0"][:], MU0)
    nband, nhl = 2, NLAY + 1
    for name, shape in (("flux_up_sw", (NCOL, 2, nhl)), ("flux_dn_sw", (NCOL, 2, nhl)), ("flux_dn_direct_sw", (NCOL, 2, nhl)),
                        ("band_flux_up_sw", (NCOL, 2, nhl, nband)), ("band_flux_dn_sw", (NCOL, 2, nhl, nband)),
                        ("band_flux_dn_direct_sw", (NCOL, 2, nhl, nband)), ("spectral_flux_dn_direct_surf_sw", (NCOL, 2, NWAV)),
                        ("spectral_flux_dn_surf_sw", (NCOL, 2, NWAV)), ("spectral_flux_up_toa_sw", (NCOL, 2, NWAV)),
                        ("mole_fraction_fl", (NCOL, 2, NLAY))):
        assert f.variables[name].shape == shape, name
    _, begin, end = api.band_ranges(wn, [LO, 10000.0], [10000.0, HI])
    alb = dev(np.full(NWAV, 0.15))
    close = lambda a, b: np.allclose(a, b, rtol=3e-7, atol=1e-30)          # the FLOAT rounding of the file
    for c in range(NCOL):
        tau = files["od"]["h2o"][c].astype(np.float64) + 0.5 * files["od"]["o3"][c].astype(np.float64)
        direct, dn, up, sdir, sdn, tup = api.lbl_band_fluxes_sw_rayleigh(ctx, MU0, dev(ssi), dev(tau), dev(files["ray"][c]), begin, end,
                                                                         albedo=alb, boundary=True)
        assert close(f.variables["band_flux_dn_direct_sw"][c], direct.transpose(0, 2, 1))
        assert close(f.variables["band_flux_dn_sw"][c], dn.transpose(0, 2, 1))
        assert close(f.variables["band_flux_up_sw"][c], up.transpose(0, 2, 1))
        assert close(f.variables["flux_dn_direct_sw"][c], direct.sum(1)) and close(f.variables["flux_dn_sw"][c], dn.sum(1))
        assert close(f.variables["flux_up_sw"][c], up.sum(1))
        assert close(f.variables["spectral_flux_dn_direct_surf_sw"][c], sdir.cpu().numpy())
        assert close(f.variables["spectral_flux_dn_surf_sw"][c], sdn.cpu().numpy())
        assert close(f.variables["spectral_flux_up_toa_sw"][c], tup.cpu().numpy())
        assert np.all(dn[:, :, 1:] > direct[:, :, 1:])                       # there is a diffuse downwelling flux now
    f.close()
    # without the boundary key: the same band fluxes, no spectral variables
    r = run_tool("ckdmip_sw", "--config", "sw.nam", "--ssi", "ssi.nc", "h2o.nc", "--scale", "0.5", "o3.nc", "--rayleigh", "rayleigh.nc",
                 "--output", "lbl_ray2.nc", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    f, g = _nc(d / "lbl_ray.nc"), _nc(d / "lbl_ray2.nc")
    assert "spectral_flux_dn_surf_sw" not in g.variables and g.rayleigh_scattering == b"two-stream"
    for name in ("band_flux_dn_sw", "band_flux_up_sw", "band_flux_dn_direct_sw"):
        assert np.array_equal(f.variables[name][...], g.variables[name][...]), name
    f.close(); g.close()
    # the same files with the Rayleigh spectrum as one more absorber (today's treatment): no new variable, no attribute
    r = run_tool("ckdmip_sw", "--config", "sw.nam", "--ssi", "ssi.nc", "h2o.nc", "--scale", "0.5", "o3.nc", "rayleigh.nc", "--output", "lbl_abs.nc", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    g = _nc(d / "lbl_abs.nc")
    assert "band_flux_dn_sw" not in g.variables and not hasattr(g, "rayleigh_scattering")
    assert np.array_equal(g.variables["flux_dn_sw"][...], g.variables["flux_dn_direct_sw"][...])
    g.close()


def test_ckd_mode_with_rayleigh_scattering(ctx, files):
    from ecckd_amd import api
    d, p1 = files["d"], files["p1"]
    rs = np.random.RandomState(5)
    ng = 7
    odg = rs.uniform(0.0, 0.4, (NCOL, NLAY, ng))
    ray = rs.uniform(0.0, 0.05, (NCOL, NLAY, ng))
    ray[:, 1, 2] = 0.0
    inc = rs.uniform(10.0, 300.0, (NCOL, ng))

    def write(path, with_ray):
        w = netcdf_file(str(path), "w", version=2)
        for dim, n in (("column", NCOL), ("half_level", NLAY + 1), ("level", NLAY), ("g_point", ng)):
            w.createDimension(dim, n)
        w.createVariable("pressure_hl", "d", ("column", "half_level"))[:] = np.tile(p1, (NCOL, 1))
        w.createVariable("optical_depth", "d", ("column", "level", "g_point"))[:] = odg
        if with_ray:
            w.createVariable("rayleigh_optical_depth", "d", ("column", "level", "g_point"))[:] = ray
        w.createVariable("incoming_sw", "d", ("column", "g_point"))[:] = inc
        w.close()
    write(d / "od_sw.nc", True)
    write(d / "od_sw_noray.nc", False)
    r = run_tool("ckdmip_sw", "--config", "sw.nam", "--ckd", "od_sw.nc", "--rayleigh-scattering", "--output", "fluxes_ray.nc", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    r = run_tool("ckdmip_sw", "--config", "sw.nam", "--ckd", "od_sw.nc", "--output", "fluxes_abs.nc", cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    f, g = _nc(d / "fluxes_ray.nc"), _nc(d / "fluxes_abs.nc")
    assert f.rayleigh_scattering == b"two-stream" and not hasattr(g, "rayleigh_scattering")
    assert "spectral_flux_dn_sw" in f.variables and "spectral_flux_dn_sw" not in g.variables
    close = lambda a, b: np.allclose(a, b, rtol=3e-7, atol=1e-30)
    for k, mu in enumerate(MU0):
        direct, dn, up = api.rt_sw_gpoints_rayleigh(ctx, mu, 0.15, inc, odg, ray)
        assert close(f.variables["spectral_flux_dn_direct_sw"][:, k], direct) and close(f.variables["spectral_flux_dn_sw"][:, k], dn)
        assert close(f.variables["spectral_flux_up_sw"][:, k], up)
        assert close(f.variables["flux_dn_direct_sw"][:, k], direct.sum(-1)) and close(f.variables["flux_dn_sw"][:, k], dn.sum(-1))
        assert close(f.variables["flux_up_sw"][:, k], up.sum(-1))
    # the direct beam is the one of the run without the switch; what scatters is no longer lost
    assert np.allclose(f.variables["flux_dn_direct_sw"][...], g.variables["flux_dn_direct_sw"][...], rtol=3e-7)
    assert np.all(f.variables["flux_dn_sw"][:, :, 1:] > g.variables["flux_dn_sw"][:, :, 1:] * (1 + 1e-4))
    assert np.all(f.variables["flux_up_sw"][:, :, 0] > g.variables["flux_up_sw"][:, :, 0] * (1 + 1e-4))
    f.close(); g.close()
    r = run_tool("ckdmip_sw", "--config", "sw.nam", "--ckd", "od_sw_noray.nc", "--rayleigh-scattering", "--output", "x.nc", cwd=d)
    assert r.returncode == PARAMETER_ERROR and "--rayleigh-scattering" in r.stderr and "rayleigh_optical_depth" in r.stderr


@pytest.mark.parametrize("tool,args,switch", [
    ("ckdmip_sw", ("--merge-only", "--rayleigh", "rayleigh.nc", "h2o.nc", "--output", "x.nc"), "--rayleigh"),
    ("ckdmip_sw", ("--merge-only", "--rayleigh-scattering", "h2o.nc", "--output", "x.nc"), "--rayleigh-scattering"),
    ("ckdmip_sw", ("--config", "sw.nam", "--ssi", "ssi.nc", "--rayleigh", "rayleigh.nc", "--scenarios", "table.txt", "h2o.nc"), "--rayleigh"),
    ("ckdmip_sw", ("--config", "sw.nam", "--ssi", "ssi.nc", "--rayleigh-scattering", "--scenarios", "table.txt", "h2o.nc"), "--rayleigh-scattering"),
    ("ckdmip_lw", ("--rayleigh", "rayleigh.nc", "h2o.nc", "--output", "x.nc"), "--rayleigh"),
    ("ckdmip_lw", ("--ckd", "od.nc", "--rayleigh-scattering", "--output", "x.nc"), "--rayleigh-scattering"),
])
def test_refused_combinations(files, tool, args, switch):
    d = files["d"]
    (d / "table.txt").write_text("present out.nc asis\n")
    r = run_tool(tool, *args, cwd=d)
    assert r.returncode == PARAMETER_ERROR, r.stderr + r.stdout
    assert f"\"{switch}\"" in r.stderr
    assert not (d / "x.nc").exists() and not (d / "out.nc").exists()
