"""ecckd_nc_write_subslice_double (no GPU): a (column, angle, level, point) record variable written one (column, angle) at a
time gives the bytes of the same variable written record by record in a classic file, reads back equal from a NetCDF-4
file, and the calls that do not fit are refused."""
import numpy as np
import pytest

from ecckd_amd import _lib, ncio

NREC, NANG, NLEV, NPT = 3, 4, 5, 37


def _data():
    rng = np.random.default_rng(7)
    return rng.random((NREC, NANG, NLEV, NPT)).astype(np.float32).astype(np.float64), rng.random((NREC, NLEV))


def _write(path, by_angle, deflate=False):
    flux, other = _data()
    w = ncio.NcWriter(path)
    w.define_dimension("column", 0)
    w.define_dimension("mu0", NANG)
    w.define_dimension("half_level", NLEV)
    w.define_dimension("wavenumber", NPT)
    w.define_variable("pressure_hl", "float", "column", "half_level")
    w.define_variable("flux", "float", "column", "mu0", "half_level", "wavenumber")
    w.define_variable("fixed", "double", "mu0", "half_level", "wavenumber")
    if deflate:
        w.deflate_variable("flux")
    w.end_define_mode()
    for r in range(NREC):
        w.write_slice("pressure_hl", r, other[r])
        if by_angle:
            for a in reversed(range(NANG)):           # (in any order)
                w.write_subslice("flux", r, a, flux[r, a])
        else:
            w.write_slice("flux", r, flux[r])
    for a in range(NANG):
        for l in range(NLEV):
            w.write_subslice("fixed", a, l, flux[0, a, l])
    return w


def test_classic_file_has_the_bytes_of_whole_records(tmp_path):
    a, b = tmp_path / "a.nc", tmp_path / "b.nc"
    _write(a, True).close()
    _write(b, False).close()
    assert a.read_bytes() == b.read_bytes()
    flux, other = _data()
    with ncio.NcFile(a) as f:
        assert np.array_equal(f.read("flux"), flux) and np.array_equal(f.read("fixed"), flux[0])
        assert np.array_equal(f.read("pressure_hl"), other.astype(np.float32))


def test_netcdf4_file_reads_back_equal(tmp_path):
    a = tmp_path / "a.h5"
    _write(a, True).close()
    assert a.read_bytes()[:8] == b"\x89HDF\r\n\x1a\n"
    flux, _ = _data()
    with ncio.NcFile(a) as f:
        assert np.array_equal(f.read("flux"), flux) and np.array_equal(f.read("fixed"), flux[0])
        assert np.array_equal(f.read("flux", 1), flux[1])


@pytest.mark.parametrize("name", ["a.nc", "a.h5"])
def test_refusals(tmp_path, name):
    flux, other = _data()
    w = _write(tmp_path / name, True)
    for args in (("flux", 0, NANG, flux[0, 0]),                 # no such angle
                 ("flux", 0, 0, flux[0]),                       # a whole record
                 ("pressure_hl", 0, 0, other[0]),               # not one index of two dimensions
                 ("fixed", NANG, 0, flux[0, 0, 0])):            # past a fixed slowest dimension
        with pytest.raises(_lib.EcckdError) as e:
            w.write_subslice(*args)
        assert e.value.code == _lib.PARAMETER_ERROR
    w.close()


def test_a_deflated_netcdf4_variable_is_refused(tmp_path):
    flux, _ = _data()
    w = ncio.NcWriter(tmp_path / "d.h5")
    w.define_dimension("column", 0)
    w.define_dimension("mu0", NANG)
    w.define_dimension("wavenumber", NPT)
    w.define_variable("flux", "float", "column", "mu0", "wavenumber")
    w.deflate_variable("flux")
    w.end_define_mode()
    with pytest.raises(_lib.EcckdError) as e:
        w.write_subslice("flux", 0, 0, flux[0, 0, 0])
    assert e.value.code == _lib.PARAMETER_ERROR
    w.close()
