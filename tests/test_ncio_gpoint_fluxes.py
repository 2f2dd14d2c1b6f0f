"""ncio.read_gpoint_fluxes: the per-g-point flux profiles of a `lw_spectra gpoints=` file as the optimiser's per-g truth.  Tiny
files written with ncio itself; no GPU."""
import numpy as np
import pytest

NCOL, NLAY, NG = 2, 3, 5


def _spectra(ng=NG, nangle=0):
    rs = np.random.RandomState(4)
    nhl = NLAY + 1
    s = dict(ng=ng, nangle=nangle, molecules="h2o co2",
             pressure_hl=np.tile(np.array([1.0, 100.0, 5000.0, 101325.0]), (NCOL, 1)), temperature_hl=200.0 + 80.0 * rs.uniform(size=(NCOL, nhl)),
             vmr_fl=1e-3 * rs.uniform(size=(NCOL, 2, NLAY)), flux_dn_lw=rs.uniform(size=(NCOL, nhl)), flux_up_lw=rs.uniform(size=(NCOL, nhl)),
             optical_depth=rs.uniform(size=(NCOL, NLAY, (ng or 7))), spectral_flux_dn_lw=rs.uniform(size=(NCOL, nhl, (ng or 7))),
             spectral_flux_up_lw=1.0 + rs.uniform(size=(NCOL, nhl, (ng or 7))))
    if ng == 0:
        s["wavenumber"] = np.arange(7.0)
    return s


@pytest.mark.parametrize("nangle", [0, 2])
def test_shapes_values_and_the_nangle_attribute(tmp_path, nangle):
    from ecckd_amd import ncio
    s = _spectra(nangle=nangle)
    path = tmp_path / "gp.nc"
    ncio.write_lw_spectra(str(path), s)
    t = ncio.read_gpoint_fluxes(str(path))
    assert t["flux"].shape == (NCOL, 2, NLAY + 1, NG) and t["flux"].dtype == np.float64 and t["flux"].flags["C_CONTIGUOUS"]
    assert t["pressure_hl"].shape == (NCOL, NLAY + 1) and t["pressure_hl"].dtype == np.float64
    assert t["nangle"] == nangle and isinstance(t["nangle"], int)                 # absent = 0
    # the file stores FLOAT: the values are the float32 roundings, down in [:, 0], up in [:, 1]
    assert np.array_equal(t["flux"][:, 0], s["spectral_flux_dn_lw"].astype(np.float32).astype(np.float64))
    assert np.array_equal(t["flux"][:, 1], s["spectral_flux_up_lw"].astype(np.float32).astype(np.float64))
    assert np.array_equal(t["pressure_hl"], s["pressure_hl"].astype(np.float32).astype(np.float64))
    assert t["flux"][:, 1].min() >= 1.0 > t["flux"][:, 0].max()


def test_a_file_without_the_variables_is_refused(tmp_path):
    from ecckd_amd import ncio
    path = tmp_path / "bands.nc"
    w = ncio.NcWriter(str(path))
    w.define_dimension("column", NCOL)
    w.define_dimension("half_level", NLAY + 1)
    w.define_variable("pressure_hl", "float", "column", "half_level")
    w.define_variable("spectral_flux_dn_lw", "float", "column", "half_level")      # one of the two is not enough
    w.end_define_mode()
    w.write("pressure_hl", np.ones((NCOL, NLAY + 1)))
    w.write("spectral_flux_dn_lw", np.ones((NCOL, NLAY + 1)))
    w.close()
    with pytest.raises(ValueError, match="spectral_flux_up_lw"):
        ncio.read_gpoint_fluxes(str(path))


def test_a_per_wavenumber_file_is_refused(tmp_path):
    """lw_spectra without gpoints= writes the same two variables on a wavenumber axis: not a per-g truth"""
    from ecckd_amd import ncio
    path = tmp_path / "wn.nc"
    ncio.write_lw_spectra(str(path), _spectra(ng=0))
    with pytest.raises(ValueError, match="g_point"):
        ncio.read_gpoint_fluxes(str(path))
