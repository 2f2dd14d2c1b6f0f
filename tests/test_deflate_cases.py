"""The hand-built DEFLATE streams of deflate_cases.py against Python's zlib, and what they reach.  No project library is
needed here: these tests say that the table is what it claims to be - every accepted stream is a valid zlib stream of the
expected bytes, zlib refuses every refused one - and that the streams themselves (parsed back by the module's own token
reader, not the builder's intent) reach the places the two decoders' edge tests (test_fast_inflate_edges.py,
test_inflate_edges_gpu.py) rely on."""
import zlib

import numpy as np
import pytest

import deflate_cases as dc


def zlib_verdict(stream):
    """zlib's answer to the whole stream: its bytes, or None where it reports an error, wants more input, or leaves input
    unread behind the trailer."""
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None


@pytest.fixture(scope="module")
def parsed():
    return {c.name: dc.read_stream(c.stream) for c in dc.accepted()}


def test_table_is_deterministic_and_complete():
    names = [c.name for c in dc.cases()]
    assert len(set(names)) == len(names)
    assert len(dc.accepted()) > 200 and len(dc.refused()) >= 40
    dc.cases.cache_clear()
    again = dc.cases()
    assert [(c.name, c.stream, c.out_len, c.expect, c.status) for c in again] == \
           [(c.name, c.stream, c.out_len, c.expect, c.status) for c in dc.cases()]


@pytest.mark.parametrize("case", dc.accepted(), ids=lambda c: c.name)
def test_zlib_inflates_every_accepted_case_to_the_expected_bytes(case):
    assert case.status == dc.OK and len(case.expect) == case.out_len
    assert zlib.decompress(case.stream) == case.expect
    assert zlib_verdict(case.stream) == case.expect


@pytest.mark.parametrize("case", dc.refused(), ids=lambda c: c.name)
def test_zlib_refuses_every_refused_case(case):
    got = zlib_verdict(case.stream)
    if case.zlib_len is None:
        assert got is None
    else:
        # the length cases (the output overrun by one byte, or one byte short): the stream is valid, of another length
        assert got is not None and len(got) == case.zlib_len and case.zlib_len != case.out_len
        assert case.status == (dc.OVERRUN if case.zlib_len > case.out_len else dc.SHORT)


def test_the_reader_agrees_with_zlib_on_every_accepted_stream(parsed):
    for c in dc.accepted():
        p = parsed[c.name]
        assert p["out_len"] == c.out_len and p["end_byte"] + 4 == len(c.stream), c.name
        assert p["blocks"][-1].final and not any(b.final for b in p["blocks"][:-1]), c.name


def _matches(parsed):
    return [m for p in parsed.values() for b in p["blocks"] for m in b.matches]


def test_matches_reach_the_far_end_of_the_window(parsed):
    ms = _matches(parsed)
    dist = {m.distance for m in ms}
    assert {32506, 32507, 32767, 32768} <= dist
    for d in (32506, 32507, 32767, 32768):
        assert {3, 258} <= {m.length for m in ms if m.distance == d}
    assert set(range(1, 259)) <= {m.distance for m in ms if m.length == 258}
    lens = {3, 4, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258}
    for d in (1, 2, 7, 8, 9, 63, 64, 65):
        assert lens <= {m.length for m in ms if m.distance == d}
    # the 32 KB window of the device decoder: distance 32768 whose run crosses a multiple of 32768, 100 bytes before it
    assert any(m.distance == 32768 and m.out_pos % 32768 == 32768 - 100 and m.length > 100 for m in ms)
    assert any(m.distance == 32768 and m.out_pos % 32768 > 32768 - m.length and m.out_pos % 32768 != 32768 - 100 for m in ms)
    assert any(m.distance == m.out_pos for m in ms)
    assert any(m.distance == 32768 and m.out_pos == 65535 for m in ms)


def test_every_symbol_and_both_spellings_of_258_occur(parsed):
    ms = _matches(parsed)
    for s in range(257, 286):
        n = dc.LEN_EXTRA[s - 257]
        assert {0, (1 << n) - 1} <= {m.length_extra for m in ms if m.length_symbol == s}, s
    for s in range(30):
        n = dc.DIST_EXTRA[s]
        assert {0, (1 << n) - 1} <= {m.distance_extra for m in ms if m.distance_symbol == s}, s
    assert any(m.length == 258 and m.length_symbol == 285 for m in ms)
    assert any(m.length == 258 and m.length_symbol == 284 and m.length_extra == 31 for m in ms)


def test_code_lengths_at_and_behind_the_primary_tables(parsed):
    """10 is the last literal/length code length inside the decoders' 10-bit primary tables, 11 the first outside, 15 the
    longest; 8, 9, 15 the same for the 8-bit distance tables.  Each must have been DECODED (a used symbol's code), for a
    literal, the end-of-block code and a length symbol."""
    lit = {"literal": set(), "end": set(), "length": set()}
    dist = set()
    for p in parsed.values():
        for b in p["blocks"]:
            if b.type != 2:
                continue
            for s in b.symbols:
                lit["literal" if s < 256 else "end" if s == 256 else "length"].add(b.lit_lens[s])
            dist |= {m.distance_bits for m in b.matches}
    for kind, seen in lit.items():
        assert {10, 11, 15} <= seen, kind
    assert {8, 9, 15} <= dist


def test_header_fields_and_run_length_items(parsed):
    dyn = [b for p in parsed.values() for b in p["blocks"] if b.type == 2]
    assert {257, 286} <= {b.hlit for b in dyn}
    assert {1, 30} <= {b.hdist for b in dyn}
    assert {5, 19} <= {b.hclen for b in dyn}                      # 4 cannot be valid: see the refused case "HCLEN 4"
    assert any(b.hdist == 1 and b.dist_lens == [1] and b.matches for b in dyn)               # a single one-bit distance code
    assert any(b.hdist == 1 and b.dist_lens == [0] and b.out_end > b.out_start for b in dyn)   # no distance code at all
    assert any([l for l in b.lit_lens if l] == [1] and b.lit_lens[256] == 1 and b.out_end == b.out_start for b in dyn)
    assert any(b.type == 1 and b.out_end == b.out_start for p in parsed.values() for b in p["blocks"])   # empty fixed block
    assert any(len(b.rle_items) > 1 and b.rle_items[1][0] == 16 for b in dyn)
    after = {(b.rle_items[i - 1][0], it[0]) for b in dyn for i, it in enumerate(b.rle_items) if i}
    assert {(17, 16), (18, 16)} <= after
    crossing = {it[0] for b in dyn for it in b.rle_items if it[1] < b.hlit < it[1] + it[2]}
    assert {16, 18} <= crossing


def test_block_headers_cover_every_bit_around_the_input_halves(parsed):
    """The device decoder fetches its input in 512-byte halves: a block header at every bit of the bytes 508 .. 516 and
    1020 .. 1028, for each of the three block types somewhere."""
    bits = {}
    for p in parsed.values():
        for b in p["blocks"]:
            bits.setdefault(b.header_bit, set()).add(b.type)
    for first in (508, 1020):
        for bit in range(8 * first, 8 * (first + 9)):
            assert bit in bits, divmod(bit, 8)
    mod = {bit % 4096 for bit in bits}
    assert set(range(8 * 508, 4096)) | set(range(0, 8 * 5)) <= mod
    assert mod == set(range(4096))
    near = set().union(*(t for bit, t in bits.items() if 8 * 500 <= bit < 8 * 524))
    assert near == {0, 1, 2}


def test_stored_blocks_end_and_straddle_at_the_input_halves(parsed):
    stored = [b for p in parsed.values() for b in p["blocks"] if b.type == 0]
    ends = {b.stored_end % 512 for b in stored}
    assert {0, 1, 2, 3, 4, 508, 509, 510, 511} <= ends
    assert ends == set(range(512))         # so each branch of the device decoder's reposition() at each `at & 3`
    # LEN/NLEN are the four bytes before the payload
    first = {b.stored_end - b.stored_len - 4 for b in stored}
    assert {509, 510, 511} <= first and {1021, 1022, 1023} <= first
    assert any(p["blocks"][-1].type == 0 and p["blocks"][-1].stored_len == 0 for p in parsed.values())
    # a stored block over the 32 KB window wrap
    assert any(b.out_start < 32768 < b.out_end for b in stored)


def test_compressed_and_inflated_lengths():
    have = {len(c.stream) for c in dc.accepted()}
    assert {512 * m + r for m in (1, 2) for r in range(-5, 6)} <= have
    outs = {c.out_len for c in dc.accepted()}
    assert {0, 1, 15, 16, 17, 63, 64, 65, 299, 300, 301, 5551, 5552, 5553, 5552 + 65, 2 * 5552 + 65} <= outs
    assert sum(c.out_len == 64 * 65536 + 65 for c in dc.accepted()) == 2
    assert max(outs) == 64 * 65536 + 65


def test_zlib_never_emits_a_distance_above_32506():
    """The gap these tables close: the "far matches" payload of test_inflate_gpu.py repeats 250 bytes at distance 32751;
    zlib's compressor codes that as literals, because it looks back 32768 - 262 bytes at the most."""
    rs = np.random.RandomState(7)
    rs.bytes(70_000)                                                # (the payloads before it in that file's _cases)
    a = rs.bytes(300)
    payload = a + rs.bytes(32768 - 300 - 17) + a[:250] + rs.bytes(5000) + a
    assert payload[32751:32751 + 250] == payload[:250]
    p = dc.read_stream(zlib.compress(payload, 9))
    assert p["out_len"] == len(payload)
    far = [m.distance for b in p["blocks"] for m in b.matches]
    assert far and max(far) <= 32506
    # a repeat at exactly 32506 is found, one byte farther is not
    for dist, found in ((32506, True), (32507, False), (32768, False)):
        data = a + rs.bytes(dist - 300) + a
        p = dc.read_stream(zlib.compress(data, 9))
        assert (dist in {m.distance for b in p["blocks"] for m in b.matches}) == found, dist
