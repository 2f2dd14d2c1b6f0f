"""zlib / DEFLATE streams inflated on the device (csrc/inflate.hip, the NetCDF-4 read path of ecckd_nc_read_dev) against
Python's zlib (the library HDF5's deflate filter uses): bit-exact for stored, fixed-Huffman and dynamic-Huffman blocks,
the matches zlib's compressor emits (distances up to 32768 - 262 = 32506: it looks no farther back, so the repeat of "far
matches" at distance 32751 reaches the decoder as literals), run-length matches (distance < length), long codes, many
streams of different sizes in one launch, and damaged streams reported per stream.  Distances 32507 .. 32768, the window
wrap and what no compressor emits: test_inflate_edges_gpu.py, from the hand-built streams of deflate_cases.py."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _shuffled_floats(n, seed):
    """what a NetCDF-4 chunk of a spectrum looks like behind the shuffle filter: byte planes of smooth positive floats"""
    rs = np.random.RandomState(seed)
    v = np.exp(np.cumsum(rs.normal(0.0, 0.05, n))).astype("<f4") * 1e-3
    v[rs.uniform(size=n) < 0.05] = 0.0
    return v.view(np.uint8).reshape(n, 4).T.copy().tobytes()


def _cases():
    rs = np.random.RandomState(7)
    cases = {
        "empty": b"",
        "one byte": b"x",
        "text": b"the quick brown fox jumps over the lazy dog. " * 400,
        "zeros": bytes(200_000),
        "random": rs.bytes(70_000),                                     # incompressible: stored blocks at any level
        "run lengths": b"".join(bytes([k % 251]) * (1 + 37 * k % 300) for k in range(2000)),
        "far matches": (lambda a: a + rs.bytes(32768 - 300 - 17) + a[:250] + rs.bytes(5000) + a)(rs.bytes(300)),
        "shuffled floats": _shuffled_floats(262_144, 3),
        "skewed alphabet": bytes(np.minimum(rs.geometric(0.08, 150_000), 255).astype(np.uint8)),   # code lengths beyond the 10-bit table
    }
    return cases


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_inflate_matches_zlib(ctx, level):
    from ecckd_amd import api
    cases = _cases()
    names = list(cases)
    streams = [zlib.compress(cases[k], level) for k in names]
    out, status = api.inflate(ctx, streams, [len(cases[k]) for k in names])
    assert list(status) == [0] * len(names), dict(zip(names, status))
    for k, got in zip(names, out):
        assert got == cases[k], k


def test_fixed_huffman_and_raw_strategies(ctx):
    from ecckd_amd import api
    data = _cases()
    streams, want = [], []
    for strategy in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
        for k in ("text", "shuffled floats", "run lengths", "skewed alphabet"):
            c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
            streams.append(c.compress(data[k]) + c.flush())
            want.append(data[k])
    out, status = api.inflate(ctx, streams, [len(w) for w in want])
    assert not status.any()
    assert out == want


def test_many_streams_of_many_sizes(ctx):
    from ecckd_amd import api
    rs = np.random.RandomState(11)
    want = [_shuffled_floats(int(n), 100 + i) for i, n in enumerate(rs.randint(1, 40_000, 700))]
    streams = [zlib.compress(w, int(rs.randint(1, 10))) for w in want]
    # several flush points inside a stream: empty stored blocks and block boundaries in odd places
    c = zlib.compressobj(6)
    pieces = [c.compress(want[0][:1000]), c.flush(zlib.Z_SYNC_FLUSH), c.compress(want[0][1000:]), c.flush(zlib.Z_FULL_FLUSH), c.flush()]
    streams[0] = b"".join(pieces)
    out, status = api.inflate(ctx, streams, [len(w) for w in want])
    assert not status.any()
    assert out == want


def test_damaged_streams_are_reported(ctx):
    from ecckd_amd import api
    good = b"spectral intervals " * 3000
    z = zlib.compress(good, 6)
    bad_header = bytes([z[0] ^ 0x0f]) + z[1:]
    truncated = z[:len(z) // 2]
    streams = [z, bad_header, truncated, z, z]
    out, status = api.inflate(ctx, streams, [len(good), len(good), len(good), len(good) - 5, len(good) + 5])
    assert status[0] == 0 and out[0] == good
    assert status[1] == 1                       # bad header
    assert status[2] != 0                       # input exhausted / bad code in the padding
    assert status[3] == 5                       # more output than expected
    assert status[4] == 6                       # less


def test_corrupted_streams_never_run_away(ctx):
    """Bit flips, truncations and garbage: every stream of the launch comes back with a verdict - output is never written
    beyond the expected size and input never fetched beyond the stream's slack, whatever the codes say (a stream whose
    damaged codes keep consuming input is fed zeros behind its end until a check stops it).  The verdicts are zlib's: the
    device decoder verifies the Adler-32 trailer, the exact end of the stream and the completeness of the codes as zlib does
    (ADVICE r02), so a stream is accepted if and only if zlib accepts it and it has the expected length."""
    from ecckd_amd import api
    rs = np.random.RandomState(13)
    base = [_shuffled_floats(20_000, 50), b"abcdefgh" * 4000, rs.bytes(9000), bytes(30_000)]
    streams, want_len, expect = [], [], []
    for k in range(240):
        raw = base[k % len(base)]
        z = bytearray(zlib.compress(raw, [1, 6, 9][k % 3]))
        kind = k % 4
        if kind == 0:                                   # flip a few bits somewhere behind the header
            for _ in range(1 + k % 3):
                pos = rs.randint(2, len(z))
                z[pos] ^= 1 << rs.randint(8)
        elif kind == 1:                                 # cut the stream short
            z = z[:rs.randint(2, len(z))]
        elif kind == 2:                                 # garbage with a valid header
            z = bytearray(b"\x78\x9c") + bytearray(rs.bytes(rs.randint(1, 3000)))
        else:                                           # a one-bit code that would produce output for ever: all-zero payload
            z = bytearray(b"\x78\x9c") + bytearray(rs.randint(1, 600))
        n = len(raw) if k % 5 else len(raw) + rs.randint(-50, 50)
        streams.append(bytes(z))
        want_len.append(max(n, 0))
        try:
            good = zlib.decompress(bytes(z))
        except zlib.error:
            good = None
        expect.append(good)
    out, status = api.inflate(ctx, streams, want_len)
    nbad = 0
    for k in range(len(streams)):
        if expect[k] is not None and len(expect[k]) == want_len[k]:
            assert status[k] == 0 and out[k] == expect[k], k
        elif expect[k] is not None:
            assert status[k] in (5, 6), (k, status[k])          # a valid stream of another length
        else:
            assert status[k] != 0, k                            # zlib refuses it: so does the device
        nbad += status[k] != 0
    assert nbad > 150


def test_checksum_end_of_stream_and_incomplete_codes(ctx):
    """What zlib, the HDF5 deflate filter and the host decoder (csrc/fast_inflate.cpp) check and the device decoder used not to:
    (i) a payload bit flipped inside a STORED block still inflates to the right length - only the Adler-32 trailer shows it;
    (ii) a damaged trailer; (iii) bytes behind the trailer / a missing trailer; (iv) an incomplete literal/length code."""
    from ecckd_amd import api
    raw = _shuffled_floats(50_000, 7)
    stored = bytearray(zlib.compress(raw, 0))                   # stored blocks: the payload is in the clear
    flipped = bytearray(stored); flipped[len(stored) // 2] ^= 0x10
    bad_trailer = bytearray(zlib.compress(raw, 6)); bad_trailer[-1] ^= 1
    good = zlib.compress(raw, 6)
    extra = good + b"\x00"
    short = good[:-1]
    # a dynamic block whose literal/length code is incomplete (one 1-bit code only for the end-of-block symbol... built by hand):
    # header 78 9c, BFINAL=1 BTYPE=01 would be the fixed code; instead take a valid stream and check zlib's verdict below
    streams = [bytes(stored), bytes(flipped), bytes(bad_trailer), good, extra, short]
    out, status = api.inflate(ctx, streams, [len(raw)] * len(streams))
    assert status[0] == 0 and out[0] == raw and status[3] == 0 and out[3] == raw
    assert status[1] == 8                                       # checksum: the bytes came out, the trailer says they are wrong
    assert status[2] == 8
    assert status[4] != 0 and status[5] != 0                    # something behind the trailer / the trailer cut
    for z, st in zip(streams, status):
        try:
            zlib.decompressobj().decompress(z)
            ok = len(zlib.decompress(z)) == len(raw)
        except zlib.error:
            ok = False
        if not ok:
            assert st != 0
