"""The host decoder (csrc/fast_inflate.cpp, through ecckd_inflate_host) on the hand-built streams of deflate_cases.py: what
zlib's compressor never emits (distances above 32506, length 258 as 284 + 31, a block without a distance code, distance
codes behind the 8-bit primary table), and streams laid against the decoder's own machinery - the switch between the fast
loop and the careful tail (eight bytes of input, 300 of output room), the three copy variants (distance >= 8, 1, 2 .. 7),
the eight-byte overshoot of a copy, the SSE2 Adler-32 at its 16-byte and 5552-byte blocks.

The reference is Python's zlib, bit for bit.  The decoder's contract lets it decline a valid stream (its caller then asks
zlib); of this table it declines none.  The output buffer lies between guard zones, as in test_fast_inflate.py."""
import ctypes as C

import numpy as np
import pytest

import deflate_cases as dc
from ecckd_amd import _lib

# Valid streams the decoder may leave to zlib: name -> reason.  Empty, and meant to stay so.
DECLINED = {}
MAX_DECLINED = 0


@pytest.fixture(scope="module")
def lib():
    return _lib.load_library()


def _inflate(lib, stream, out_len, guard=64):
    """(ok, bytes): the output buffer sits between two guard zones that must stay untouched."""
    src = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(0, np.uint8)
    buf = np.full(out_len + 2 * guard, 0xA5, dtype=np.uint8)
    ok = C.c_int(-1)
    rc = lib.ecckd_inflate_host(src.ctypes.data_as(C.c_void_p), src.size, (buf.ctypes.data + guard), out_len, C.byref(ok))
    assert rc == 0 and ok.value in (0, 1)
    assert (buf[:guard] == 0xA5).all() and (buf[out_len + guard:] == 0xA5).all(), "wrote outside the output buffer"
    return bool(ok.value), buf[guard:guard + out_len].tobytes()


def test_the_exception_list_stays_this_small():
    assert len(DECLINED) <= MAX_DECLINED
    assert set(DECLINED) <= {c.name for c in dc.accepted()}


@pytest.mark.parametrize("case", dc.accepted(), ids=lambda c: c.name)
def test_accepted_cases_decode_to_zlibs_bytes(lib, case):
    ok, out = _inflate(lib, case.stream, case.out_len)
    if case.name in DECLINED:
        assert not ok, "declined by the list, yet decoded: take it off the list"
        return
    assert ok, "a valid stream was declined"
    assert out == case.expect


@pytest.mark.parametrize("case", dc.refused(), ids=lambda c: c.name)
def test_refused_cases_are_refused(lib, case):
    assert not _inflate(lib, case.stream, case.out_len)[0]


@pytest.mark.parametrize("case", dc.accepted(), ids=lambda c: c.name)
def test_another_length_is_refused(lib, case):
    """one byte less room than the stream fills, and one byte more than it fills"""
    if case.out_len:
        assert not _inflate(lib, case.stream, case.out_len - 1)[0]
    assert not _inflate(lib, case.stream, case.out_len + 1)[0]
