"""The device decoder (csrc/inflate.hip, one wavefront per stream) on the hand-built streams of deflate_cases.py, against
Python's zlib bit for bit.  test_inflate_gpu.py feeds it what zlib's compressor emits, which never reaches a match distance
above 32506 and places nothing on purpose; the table here does, group by group:

  window wrap          distance 32768, where the source slot (pos - dist + i) & 32767 IS the destination slot, with runs that
                       cross a multiple of 32768; distances 32506 .. 32768 at the first position that allows them; stored
                       blocks across the wrap and a match at distance 32768 behind 65535 stored bytes
  reposition()         small fixed, dynamic and stored blocks behind k stored bytes, k = 0 .. one unit: every stored block
                       ends at every `at` mod 512 - both fetches, the first only (at a multiple of 512: refill() fetches the
                       next half), neither - and at every at & 3; LEN/NLEN straddle byte 512; block headers at every bit of
                       the bytes 508 .. 516 and 1020 .. 1028, where refill() changes halves
  limit                compressed lengths 512 m + r, r = -5 .. 5: at r = 0 the trailer ends at the half's last byte and
                       limit = in_bytes + 512; r = 1 .. 3 have the trailer across the boundary
  run-length copy      every distance 1 .. 258 with length 258, and lengths 3 .. 258 around the 64-lane strides at distances
                       1, 2, 7, 8, 9, 63, 64, 65: the distance < length path with its five bytes per lane
  decode_long          literal/length codes of 11 .. 15 bits and distance codes of 9 .. 15 bits (behind the 10- and 8-bit
                       tables), for literals, the end-of-block code, length symbols and sixteen distance symbols
  Adler-32             two streams of 64 * 65536 + 65 bytes: every lane's slice is 65537 bytes, one more than the interval
                       of the in-slice reduction

Refused streams carry the status the decoder's checks lead to.  They lie between accepted ones, whose outputs are directly
behind theirs in the output buffer: whatever a refused stream wrote, its neighbours come back intact."""
import numpy as np
import pytest

import deflate_cases as dc

pytestmark = pytest.mark.gpu


def _interleaved(order):
    acc, ref = list(dc.accepted()), list(dc.refused())
    if order == "backwards":
        acc, ref = acc[::-1], ref[::-1]
    step = len(acc) // len(ref)
    seq = []
    for i, c in enumerate(acc):
        if order == "backwards" and i % step == 0 and i // step < len(ref):
            seq.append(ref[i // step])                      # (a refused stream first)
        seq.append(c)
        if order == "forwards" and i % step == step - 1 and i // step < len(ref):
            seq.append(ref[i // step])
    assert len(seq) == len(acc) + len(ref)
    return seq


@pytest.mark.parametrize("order", ["forwards", "backwards"])
def test_the_whole_table_in_one_launch(ctx, order):
    from ecckd_amd import api
    seq = _interleaved(order)
    out, status = api.inflate(ctx, [c.stream for c in seq], [c.out_len for c in seq])
    wrong = []
    for c, got, st in zip(seq, out, status):
        if c.expect is not None:
            if st != 0 or got != c.expect:
                wrong.append((c.name, int(st), "bytes differ" if st == 0 else "refused"))
        elif st == 0 or (c.status is not None and st != c.status):
            wrong.append((c.name, int(st), f"expected status {c.status}"))
    assert not wrong, wrong


def test_one_byte_less_and_one_byte_more_than_the_stream_holds(ctx):
    """every accepted stream asked for out_bytes - 1 (status 5: the output would overrun) and out_bytes + 1 (6: short)"""
    from ecckd_amd import api
    acc = dc.accepted()
    less = [c for c in acc if c.out_len]
    streams = [c.stream for c in less] + [c.stream for c in acc]
    want = [c.out_len - 1 for c in less] + [c.out_len + 1 for c in acc]
    expect = [dc.OVERRUN] * len(less) + [dc.SHORT] * len(acc)
    _, status = api.inflate(ctx, streams, want)
    wrong = [(c.name, int(st), e) for c, st, e in zip(less + acc, status, expect) if st != e]
    assert not wrong, wrong
    assert np.count_nonzero(status) == len(streams)
