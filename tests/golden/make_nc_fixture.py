"""Generates tests/golden/mie_droplet_scattering.nc: the reference's NetCDF-classic data file data/mie_droplet_scattering.nc
cut to the first NRAD effective radii and NWN wavenumbers.  Every header byte is the reference's own except the dimension
lengths and each variable's vsize and begin, which are patched in place (fixed-size fields); each variable's data is the
leading block of the original.  Run from the repo root:
    python tests/golden/make_nc_fixture.py REFERENCE/data/mie_droplet_scattering.nc"""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KEEP = {"effective_radius": 10, "wavenumber": 40}
SIZES = {1: 1, 2: 1, 3: 2, 4: 4, 5: 4, 6: 8}           # NC_BYTE, CHAR, SHORT, INT, FLOAT, DOUBLE
DTYPES = {1: ">i1", 2: "S1", 3: ">i2", 4: ">i4", 5: ">f4", 6: ">f8"}


def main():
    src = open(sys.argv[1], "rb").read()
    assert src[:4] == b"CDF\x01" and struct.unpack(">i", src[4:8])[0] == 0      # CDF-1, no records
    hdr = bytearray(src)
    pos = 8
    u32 = lambda: struct.unpack(">i", src[pos:pos + 4])[0]

    def name():
        nonlocal pos
        n = u32()
        s = src[pos + 4:pos + 4 + n].decode()
        pos += 4 + (n + 3) // 4 * 4
        return s

    def atts():
        nonlocal pos
        tag, n = struct.unpack(">ii", src[pos:pos + 8])
        pos += 8
        for _ in range(n):
            name()
            t, cnt = struct.unpack(">ii", src[pos:pos + 8])
            pos += 8 + (cnt * SIZES[t] + 3) // 4 * 4

    pos += 4                                               # NC_DIMENSION
    ndim = u32(); pos += 4
    dims = []
    for _ in range(ndim):
        dn = name()
        old = u32()
        new = KEEP.get(dn, old)
        struct.pack_into(">i", hdr, pos, new)
        dims.append((old, new))
        pos += 4
    atts()                                                 # global attributes
    pos += 4
    nvar = u32(); pos += 4
    variables = []
    for _ in range(nvar):
        name()
        nd = u32()
        ids = struct.unpack(">%di" % nd, src[pos + 4:pos + 4 + 4 * nd])
        pos += 4 + 4 * nd
        atts()
        t = u32()
        variables.append((t, ids, pos + 4, pos + 8, struct.unpack(">i", src[pos + 8:pos + 12])[0]))
        pos += 12
    begin = variables[0][4]                                # the reference's header, padding included, up to its first variable
    first = begin
    out = [None]
    for t, ids, at_vsize, at_begin, old_begin in variables:
        shape_old = tuple(dims[i][0] for i in ids)
        data = np.frombuffer(src, DTYPES[t], int(np.prod(shape_old)), old_begin).reshape(shape_old)
        block = data[tuple(slice(0, dims[i][1]) for i in ids) + (Ellipsis,)].tobytes()
        vsize = (len(block) + 3) // 4 * 4
        struct.pack_into(">ii", hdr, at_vsize, vsize, begin)
        out.append(block + b"\0" * (vsize - len(block)))
        begin += vsize
    out[0] = bytes(hdr[:first])
    with open(os.path.join(HERE, "mie_droplet_scattering.nc"), "wb") as f:
        f.write(b"".join(out))


if __name__ == "__main__":
    main()
