"""The classic NetCDF writer's record variables (CPU): a file with an unlimited first dimension and two record variables of
different types, written record by record and read back with the repository's reader; numrecs and the interleaving of the
records checked against the layout rule at the head of csrc/nc_classic.cpp (big-endian; header = magic numrecs dim_list
gatt_list var_list; fixed-size variables contiguous at `begin`, then record r of every record variable at begin + r * recsize,
recsize = the sum of the record variables' sizes, each padded to 4 bytes).  A file WITHOUT record variables must come out
byte for byte as before: its expected bytes are generated here from the same rule."""
import struct

import numpy as np
import pytest


def _name(s):
    b = s.encode()
    return struct.pack(">I", len(b)) + b + b"\0" * (-len(b) % 4)


def _text_att(name, text):
    b = text.encode()
    return _name(name) + struct.pack(">II", 2, len(b)) + b + b"\0" * (-len(b) % 4)      # NC_CHAR = 2


def _att_list(atts):
    if not atts:
        return struct.pack(">II", 0, 0)
    return struct.pack(">II", 0x0C, len(atts)) + b"".join(atts)


def _var(name, dimids, atts, nc_type, vsize, begin):
    return (_name(name) + struct.pack(">I", len(dimids)) + b"".join(struct.pack(">I", d) for d in dimids) + _att_list(atts) +
            struct.pack(">III", nc_type, vsize, begin))


def _header(numrecs, dims, gatts, vars_):
    """CDF-1 header; vars_ = [(name, dimids, atts, nc_type, vsize, begin)]"""
    h = b"CDF\x01" + struct.pack(">I", numrecs)
    h += struct.pack(">II", 0x0A, len(dims)) + b"".join(_name(n) + struct.pack(">I", l) for n, l in dims)
    h += _att_list(gatts)
    h += struct.pack(">II", 0x0B, len(vars_)) + b"".join(_var(*v) for v in vars_)
    return h


def test_fixed_dimension_file_is_byte_identical(tmp_path):
    from ecckd_amd import ncio
    a = np.arange(6, dtype=np.float64).reshape(3, 2) + 0.5
    b = np.array([1e-3, -2.0])
    path = tmp_path / "fixed.nc"
    w = ncio.NcWriter(path)
    w.define_dimension("x", 3)
    w.define_dimension("y", 2)
    w.define_variable("a", "float", "x", "y")
    w.write_attribute("units", "m", var="a")
    w.define_variable("b", "double", "y")
    w.write_attribute("title", "fixed", None)
    w.end_define_mode()
    w.write("a", a)
    w.write_slice("a", 1, a[1] * 2.0)
    w.write("b", b)
    w.close()
    a[1] *= 2.0
    dims = [("x", 3), ("y", 2)]
    gatts = [_text_att("title", "fixed")]

    def hdr(begin_a, begin_b):
        return _header(0, dims, gatts, [("a", [0, 1], [_text_att("units", "m")], 5, 24, begin_a), ("b", [1], [], 6, 16, begin_b)])
    n = len(hdr(0, 0))
    expected = hdr(n, n + 24) + a.astype(">f4").tobytes() + b.astype(">f8").tobytes()
    assert path.read_bytes() == expected


def test_record_variables_numrecs_and_interleaving(tmp_path):
    from ecckd_amd import ncio
    path = tmp_path / "records.nc"
    nrec, nlev = 3, 2
    p = np.array([[1.5, 2.5], [3.5, 4.5], [5.5, 6.5]])
    k = np.array([7.0, -8.0, 9.0])
    lev = np.array([10.0, 20.0])
    w = ncio.NcWriter(path)
    w.define_dimension("column", 0)                  # unlimited
    w.define_dimension("level", nlev)
    w.define_variable("p", "float", "column", "level")
    w.define_variable("level_value", "double", "level")       # a fixed-size variable defined between the record variables
    w.define_variable("k", "short", "column")
    w.end_define_mode()
    w.write("level_value", lev)
    # the header says 0 records until one is written
    assert struct.unpack(">I", path.read_bytes()[4:8])[0] == 0
    w.write_slice("p", 0, p[0])
    w.write_slice("k", 0, k[:1])
    assert struct.unpack(">I", path.read_bytes()[4:8])[0] == 1
    w.write_slice("k", 2, k[2:])                     # record 2 before record 1: the count follows the highest record
    w.write_slice("p", 2, p[2])
    w.write_slice("p", 1, p[1])
    w.write_slice("k", 1, k[1:2])
    with pytest.raises(Exception):
        w.write("p", p)                              # record variables are written record by record
    w.close()
    raw = path.read_bytes()
    dims = [("column", 0), ("level", nlev)]

    def hdr(b_p, b_l, b_k):
        return _header(nrec, dims, [], [("p", [0, 1], [], 5, 8, b_p), ("level_value", [1], [], 6, 16, b_l), ("k", [0], [], 3, 4, b_k)])
    n = len(hdr(0, 0, 0))
    # fixed-size data first (level_value), then the records: p (8 bytes) and k (a SHORT padded to 4) interleaved, recsize 12
    head = hdr(n + 16, n, n + 16 + 8)
    assert raw[:n] == head
    assert raw[n:n + 16] == lev.astype(">f8").tobytes()
    recs = b"".join(p[r].astype(">f4").tobytes() + k[r:r + 1].astype(">i2").tobytes() + b"\0\0" for r in range(nrec))
    assert raw[n + 16:] == recs and len(raw) == n + 16 + nrec * 12
    with ncio.NcFile(path) as f:
        assert f.dim("column") == nrec and f.dim("level") == nlev
        assert f.var_info("p") == (5, (nrec, nlev)) and f.var_info("k") == (3, (nrec,))
        assert np.array_equal(f.read("p"), p) and np.array_equal(f.read("k"), k) and np.array_equal(f.read("level_value"), lev)
        assert np.array_equal(f.read("p", 1), p[1])


def test_a_single_record_variable_and_unwritten_records(tmp_path):
    """One record variable: its records follow each other without padding (recsize = its unpadded size); a record written past
    the end leaves the records before it zero."""
    from ecckd_amd import ncio
    path = tmp_path / "single.nc"
    w = ncio.NcWriter(path)
    w.define_dimension("column", 0)
    w.define_dimension("three", 3)
    w.define_variable("s", "short", "column", "three")
    w.end_define_mode()
    w.write_slice("s", 1, [4, 5, 6])
    w.close()
    raw = path.read_bytes()
    assert struct.unpack(">I", raw[4:8])[0] == 2
    assert raw[-12:] == b"\0" * 6 + np.array([4, 5, 6], dtype=">i2").tobytes()
    with ncio.NcFile(path) as f:
        assert np.array_equal(f.read("s"), [[0, 0, 0], [4, 5, 6]])
    # a second unlimited dimension, or one that is not the slowest, is refused
    w = ncio.NcWriter(tmp_path / "bad.nc")
    w.define_dimension("column", 0)
    with pytest.raises(Exception):
        w.define_dimension("other", 0)
    w.define_dimension("n", 2)
    with pytest.raises(Exception):
        w.define_variable("v", "float", "n", "column")


def test_large_records_choose_the_64_bit_offset_variant(tmp_path):
    """The record variables begin inside the first record, after the fixed-size data: when one record is so large that a later
    record variable begins at or above 2^31, CDF-1's 4-byte `begin` cannot hold the offset and the file must be CDF-2 (8-byte
    begins).  Defined only, never written: the file stays a header."""
    from ecckd_amd import ncio
    nwav, nhl = 7_200_000, 55                         # one record of lw_spectra's spectral fluxes: 1.58 GB per variable
    path = tmp_path / "large.nc"
    w = ncio.NcWriter(path)
    w.define_dimension("column", 0)
    w.define_dimension("half_level", nhl)
    w.define_dimension("wavenumber", nwav)
    for name in ("a", "b", "c"):
        w.define_variable(name, "float", "column", "half_level", "wavenumber")
    w.end_define_mode()
    w.close()
    raw = path.read_bytes()
    assert raw[:4] == b"CDF\x02"
    vsize = nhl * nwav * 4
    dims = struct.pack(">II", 0x0A, 3) + b"".join(_name(n) + struct.pack(">I", l) for n, l in
                                                   (("column", 0), ("half_level", nhl), ("wavenumber", nwav)))

    def var(name, begin):
        return (_name(name) + struct.pack(">I", 3) + struct.pack(">III", 0, 1, 2) + _att_list([]) +
                struct.pack(">II", 5, vsize) + struct.pack(">Q", begin))
    n = len(b"CDF\x02" + struct.pack(">I", 0) + dims + _att_list([]) + struct.pack(">II", 0x0B, 3) + b"".join(var(x, 0) for x in "abc"))
    expected = (b"CDF\x02" + struct.pack(">I", 0) + dims + _att_list([]) + struct.pack(">II", 0x0B, 3) +
                var("a", n) + var("b", n + vsize) + var("c", n + 2 * vsize))
    assert n + 2 * vsize > 2 ** 31 and raw == expected
    with ncio.NcFile(path) as f:
        assert f.dim("column") == 0 and f.dim("wavenumber") == nwav and f.var_info("a") == (5, (0, nhl, nwav))
    # the same three variables at a size whose first record stays below 2^31: still CDF-1
    small = tmp_path / "small.nc"
    w = ncio.NcWriter(small)
    w.define_dimension("column", 0)
    w.define_dimension("n", 1000)
    for name in ("a", "b", "c"):
        w.define_variable(name, "float", "column", "n")
    w.end_define_mode()
    w.close()
    assert small.read_bytes()[:4] == b"CDF\x01"


def test_netcdf4_unlimited_dimension_round_trip(tmp_path):
    """The same calls on a file named *.h5: chunked datasets with an unlimited first dimension, extended record by record;
    read back through the repository's HDF5 reader.  One record variable is deflated (chunks built by the worker threads)."""
    from ecckd_amd import ncio
    path = tmp_path / "records.h5"
    nrec, nlev, nw = 3, 2, 700
    rng = np.random.default_rng(3)
    p = rng.random((nrec, nlev)).astype(np.float32).astype(np.float64)
    od = rng.random((nrec, nlev, nw)).astype(np.float32).astype(np.float64)
    wn = np.arange(nw, dtype=np.float64)
    w = ncio.NcWriter(path)
    assert w.is_netcdf4
    w.define_dimension("column", 0)
    w.define_dimension("level", nlev)
    w.define_dimension("wavenumber", nw)
    w.define_variable("p", "float", "column", "level")
    w.define_variable("wavenumber", "double", "wavenumber")
    w.define_variable("od", "float", "column", "level", "wavenumber")
    w.deflate_variable("od")
    w.write_attribute("units", "Pa", var="p")
    w.end_define_mode()
    w.write("wavenumber", wn)
    for r in (0, 2, 1):                              # out of order: the count follows the highest record
        w.write_slice("p", r, p[r])
        w.write_slice("od", r, od[r])
    with pytest.raises(Exception):
        w.write("p", p)
    w.close()
    assert path.read_bytes()[:8] == b"\x89HDF\r\n\x1a\n"
    with ncio.NcFile(path) as f:
        assert f.dim("column") == nrec and f.dim("level") == nlev
        assert f.var_info("p") == (5, (nrec, nlev)) and f.var_info("od") == (5, (nrec, nlev, nw))
        assert np.array_equal(f.read("p"), p) and np.array_equal(f.read("od"), od)
        assert np.array_equal(f.read("od", 1), od[1]) and np.array_equal(f.read("wavenumber"), wn)
        assert f.att_text("units", "p") == "Pa"
