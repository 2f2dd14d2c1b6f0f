"""Hand-built zlib / DEFLATE streams (RFC 1950, RFC 1951) for the two inflate decoders, csrc/fast_inflate.cpp and
csrc/inflate.hip.  Pure Python and numpy; nothing of the project is imported.

A compressor only ever emits what its heuristics choose: zlib never codes a match farther back than 32768 - 262 = 32506
bytes, never spells length 258 as symbol 284 with 31 in its extra bits, never leaves out the distance code.  The builder here
writes exactly the tokens, code lengths and header fields it is told to, so that a stream can be laid against the decoders' own
machinery (window wrap, 512-byte input halves, copy variants, checksum blocks), and it can break one thing at a time.

  Stream        the builder: stored(), fixed(), dynamic() blocks between the zlib header and the Adler-32 trailer
  read_stream   a slow, separate reader that parses a stream's bits back into blocks and tokens; the coverage facts of
                test_deflate_cases.py are computed with it from the streams, not from what the builder was asked to do
  cases()       the table: named streams with the expected length and bytes (accepted) or None (refused)

Tokens: an int is a literal byte, (length, distance) a match.  Three raw forms exist for what no valid encoder writes:
("m", length symbol, extra bits, distance symbol, extra bits), ("s", literal/length symbol) and ("b", value, nbits).
"""
import functools
import heapq
import zlib
from collections import namedtuple

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# the status enum of csrc/inflate.hip
OK, BAD_HEADER, BAD_BLOCK, BAD_CODE, BAD_DISTANCE, OVERRUN, SHORT, INPUT, CHECKSUM = range(9)


# ---------------------------------------------------------------------------------------------------------- the builder

class BitWriter:
    """DEFLATE's bit order: values least significant bit first, Huffman codes most significant bit first."""

    def __init__(self):
        self.data = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.data.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, length):
        rev = 0
        for _ in range(length):
            rev = (rev << 1) | (code & 1)
            code >>= 1
        self.put(rev, length)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def put_bytes(self, data):
        assert self.n == 0
        self.data += data


def canonical_codes(lengths):
    """{symbol: (code, length)} of the canonical Huffman code; the lengths are taken as they are (also a broken set)."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = {}
    for s, l in enumerate(lengths):
        if l:
            codes[s] = (nxt[l], l)
            nxt[l] += 1
    return codes


_FIXED_LIT_CODES, _FIXED_DIST_CODES = canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST)


def huffman_lengths(freqs, maxbits):
    """Code lengths of a Huffman code for the symbols with freqs > 0, none longer than maxbits (the frequencies are halved
    until the tree is flat enough).  At least two symbols get a code, as in zlib's compressor, so the code is complete."""
    freqs = list(freqs)
    used = [s for s, f in enumerate(freqs) if f > 0]
    for s in range(len(freqs)):
        if len(used) >= 2:
            break
        if s not in used:
            used.append(s)
            freqs[s] = 1
    f = {s: freqs[s] for s in used}
    while True:
        depth = dict.fromkeys(used, 0)
        heap = [(f[s], s, [s]) for s in used]
        heapq.heapify(heap)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= maxbits:
            break
        f = {s: (v + 1) // 2 for s, v in f.items()}
    lengths = [0] * len(freqs)
    for s, d in depth.items():
        lengths[s] = d
    return lengths


def length_symbol(length, long258=False):
    if length == 258:
        return (284, 31) if long258 else (285, 0)
    for i in range(27, -1, -1):
        if LEN_BASE[i] <= length:
            return 257 + i, length - LEN_BASE[i]
    raise ValueError(length)


def distance_symbol(dist):
    for i in range(29, -1, -1):
        if DIST_BASE[i] <= dist:
            return i, dist - DIST_BASE[i]
    raise ValueError(dist)


def _raw_tokens(tokens, long258):
    raw = []
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            raw.append(("l", int(t)))
        elif len(t) == 2 and not isinstance(t[0], str):
            raw.append(("m",) + length_symbol(t[0], long258) + distance_symbol(t[1]))
        else:
            raw.append(tuple(t))
    return raw


def rle_auto(lengths):
    """The run-length items a compressor would choose: ints are lengths as they are, (16|17|18, count) are repeats."""
    items, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                c = min(run, 138)
                items.append((18, c))
                run -= c
            if run >= 3:
                items.append((17, run))
                run = 0
            items += [0] * run
        else:
            items.append(v)
            run -= 1
            while run >= 3:
                c = min(run, 6)
                items.append((16, c))
                run -= c
            items += [v] * run
        i = j
    return items


class Stream:
    """One zlib stream under construction.  `out` is what its blocks inflate to so far (worked out from the tokens here;
    the tests hold it against zlib's answer)."""

    def __init__(self, cmf=0x78, flg=None):
        self.w = BitWriter()
        if flg is None:
            flg = (31 - (cmf << 8) % 31) % 31
        self.w.put(cmf, 8)
        self.w.put(flg, 8)
        self.out = bytearray()

    # -- blocks

    def stored(self, data=b"", final=False, len_field=None, nlen_field=None):
        """Stored block(s); more than 65535 bytes are split.  len_field / nlen_field overwrite what the header says."""
        data = bytes(data)
        pieces = [data[i:i + 65535] for i in range(0, len(data), 65535)] or [b""]
        for k, piece in enumerate(pieces):
            self.w.put(1 if final and k == len(pieces) - 1 else 0, 1)
            self.w.put(0, 2)
            self.w.align()
            ln = len(piece) if len_field is None else len_field
            self.w.put(ln, 16)
            self.w.put(ln ^ 0xffff if nlen_field is None else nlen_field, 16)
            self.w.put_bytes(piece)
            self.out += piece
        return self

    def fixed(self, tokens, final=False, long258=False, eob=True):
        self.w.put(1 if final else 0, 1)
        self.w.put(1, 2)
        self._tokens(_raw_tokens(tokens, long258), _FIXED_LIT_CODES, _FIXED_DIST_CODES, eob)
        return self

    def dynamic(self, tokens, final=False, long258=False, eob=True, lit_lens=None, dist_lens=None, hlit=None, hdist=None,
                hclen=None, rle="auto", cl_lens=None, hlit_field=None, hdist_field=None):
        """A dynamic-Huffman block.  lit_lens / dist_lens: {symbol: length} or a list, else a Huffman code from the tokens'
        frequencies limited to 15 bits.  hlit / hdist / hclen: the counts the header announces (default: the smallest that
        hold the codes).  rle: "auto", "plain" (every length on its own) or the list of items itself, which is then written
        as it stands - also where it does not add up.  cl_lens: {symbol: length} of the code-length code, else a Huffman code
        of the items limited to 7 bits.  hlit_field / hdist_field: raw 5-bit header values.  tokens=None: header only."""
        raw = _raw_tokens(tokens or [], long258)
        if lit_lens is None or dist_lens is None:
            lf, df = [0] * 286, [0] * 30
            lf[256] = 1
            for t in raw:
                if t[0] == "l":
                    lf[t[1]] += 1
                elif t[0] == "m":
                    lf[t[1]] += 1
                    df[t[3]] += 1
            if lit_lens is None:
                lit_lens = huffman_lengths(lf, 15)
            if dist_lens is None:
                dist_lens = huffman_lengths(df, 15)
        lit_lens, dist_lens = _as_list(lit_lens), _as_list(dist_lens)
        if hlit is None:
            hlit = max(257, len(lit_lens) - _trailing_zeros(lit_lens))
        if hdist is None:
            hdist = max(1, len(dist_lens) - _trailing_zeros(dist_lens))
        assert not any(lit_lens[hlit:]) and not any(dist_lens[hdist:]), "hlit / hdist cut a code off"
        lit_lens = (lit_lens + [0] * hlit)[:hlit]
        dist_lens = (dist_lens + [0] * hdist)[:hdist]
        both = lit_lens + dist_lens
        items = rle_auto(both) if rle == "auto" else list(both) if rle == "plain" else list(rle)
        if cl_lens is None:
            cf = [0] * 19
            for it in items:
                cf[it if isinstance(it, int) else it[0]] += 1
            cl = huffman_lengths(cf, 7)
        else:
            cl = [cl_lens.get(s, 0) for s in range(19)]
        if hclen is None:
            hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl[s]))
        assert all(cl[s] == 0 for s in CL_ORDER[hclen:]), "hclen cuts a code-length code off"
        w = self.w
        w.put(1 if final else 0, 1)
        w.put(2, 2)
        w.put(hlit - 257 if hlit_field is None else hlit_field, 5)
        w.put(hdist - 1 if hdist_field is None else hdist_field, 5)
        w.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.put(cl[s], 3)
        cl_codes = canonical_codes(cl)
        for it in items:
            if isinstance(it, int):
                w.put_code(*cl_codes[it])
            else:
                w.put_code(*cl_codes[it[0]])
                w.put(it[1] - (11 if it[0] == 18 else 3), 7 if it[0] == 18 else 3 if it[0] == 17 else 2)
        if tokens is not None:
            self._tokens(raw, canonical_codes(lit_lens), canonical_codes(dist_lens), eob)
        return self

    def _tokens(self, raw, lit, dist, eob):
        w, out = self.w, self.out
        for t in raw:
            if t[0] == "l":
                w.put_code(*lit[t[1]])
                out.append(t[1])
            elif t[0] == "s":
                w.put_code(*lit[t[1]])
            elif t[0] == "b":
                w.put(t[1], t[2])
            else:
                _, ls, le, ds, de = t
                w.put_code(*lit[ls])
                w.put(le, LEN_EXTRA[ls - 257])
                w.put_code(*dist[ds])
                if ds < 30:
                    w.put(de, DIST_EXTRA[ds])
                    length, d = LEN_BASE[ls - 257] + le, DIST_BASE[ds] + de
                    if 0 < d <= len(out):                      # (a match that no decoder may take adds nothing)
                        if d >= length:
                            out += out[len(out) - d:len(out) - d + length]
                        else:
                            for _ in range(length):
                                out.append(out[-d])
        if eob:
            w.put_code(*lit[256])

    # -- the end

    def finish(self, trailer=True, adler=None, extra=b""):
        self.w.align()
        if trailer:
            self.w.put_bytes((zlib.adler32(bytes(self.out)) if adler is None else adler).to_bytes(4, "big"))
        self.w.put_bytes(extra)
        return bytes(self.w.data)


def _as_list(lens):
    if isinstance(lens, dict):
        full = [0] * (max(lens) + 1)
        for s, l in lens.items():
            full[s] = l
        return full
    return list(lens)


def _trailing_zeros(lens):
    n = 0
    while n < len(lens) and lens[len(lens) - 1 - n] == 0:
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------------ the reader

Block = namedtuple("Block", "type final header_bit lit_lens dist_lens hlit hdist hclen rle_items matches symbols "
                            "stored_len stored_end out_start out_end")
Block.__doc__ = """type 0 / 1 / 2; header_bit: where the block's first bit lies in the stream (byte header_bit // 8, bit header_bit % 8);
lit_lens, dist_lens, hlit, hdist, hclen, rle_items (symbol, first index, count): a dynamic header as read; symbols: the
literal/length symbols that were decoded; stored_end: the byte behind a stored block; out_start, out_end: its output."""
Match = namedtuple("Match", "length distance out_pos length_symbol length_extra distance_symbol distance_extra "
                            "length_bits distance_bits")


class _Bits:
    def __init__(self, data, pos):
        self.data, self.pos = data, pos

    def take(self, n):
        v = 0
        for i in range(n):
            p = self.pos + i
            if (p >> 3) >= len(self.data):
                raise ValueError("ran out of input")
            v |= ((self.data[p >> 3] >> (p & 7)) & 1) << i
        self.pos += n
        return v

    def symbol(self, table):
        code = 0
        for l in range(1, 16):
            code = (code << 1) | self.take(1)
            s = table.get((l, code))
            if s is not None:
                return s, l
        raise ValueError("no such code")


def _decode_table(lengths):
    """{(length, code): symbol}, written out on its own (RFC 1951 3.2.2): shorter codes first, symbols in order"""
    table, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lengths):
            if sl == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table


_FIXED_LIT_TABLE, _FIXED_DIST_TABLE = _decode_table(FIXED_LIT), _decode_table(FIXED_DIST)


def read_stream(stream):
    """Parse a valid zlib stream -> dict(blocks=[Block], out_len, end_byte): for every block its type, where its header
    starts (bit position in the stream, the zlib header included), the code lengths and run-length items of a dynamic header
    (symbol, first index, count), its matches with their output positions, and for a stored block the byte behind it.
    Positions only - no output is produced.  ValueError for anything it cannot follow."""
    b = _Bits(stream, 16)
    blocks, opos = [], 0
    while True:
        header_bit = b.pos
        final, btype = b.take(1), b.take(2)
        start = opos
        if btype == 0:
            b.pos = (b.pos + 7) & ~7
            ln, nl = b.take(16), b.take(16)
            if ln ^ nl != 0xffff:
                raise ValueError("stored lengths")
            b.pos += 8 * ln
            if b.pos > 8 * len(stream):
                raise ValueError("ran out of input")
            opos += ln
            blocks.append(Block(0, final, header_bit, None, None, None, None, None, None, [], set(), ln, b.pos // 8, start, opos))
        elif btype == 3:
            raise ValueError("block type 3")
        else:
            hlit = hdist = hclen = items = None
            if btype == 1:
                lit_lens, dist_lens, lit, dist = FIXED_LIT, FIXED_DIST, _FIXED_LIT_TABLE, _FIXED_DIST_TABLE
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl[s] = b.take(3)
                cl_table, lens, items = _decode_table(cl), [], []
                while len(lens) < hlit + hdist:
                    s, _ = b.symbol(cl_table)
                    if s < 16:
                        items.append((s, len(lens), 1))
                        lens.append(s)
                    else:
                        rep = 3 + b.take(2) if s == 16 else 3 + b.take(3) if s == 17 else 11 + b.take(7)
                        if s == 16 and not lens:
                            raise ValueError("repeat without a length")
                        items.append((s, len(lens), rep))
                        lens += [lens[-1] if s == 16 else 0] * rep
                if len(lens) > hlit + hdist:
                    raise ValueError("too many lengths")
                lit_lens, dist_lens = lens[:hlit], lens[hlit:]
                lit, dist = _decode_table(lit_lens), _decode_table(dist_lens)
            matches, symbols = [], set()
            while True:
                s, sl = b.symbol(lit)
                symbols.add(s)
                if s < 256:
                    opos += 1
                elif s == 256:
                    break
                else:
                    le = b.take(LEN_EXTRA[s - 257])
                    ds, dl = b.symbol(dist)
                    de = b.take(DIST_EXTRA[ds])
                    length, d = LEN_BASE[s - 257] + le, DIST_BASE[ds] + de
                    if d > opos:
                        raise ValueError("distance too far back")
                    matches.append(Match(length, d, opos, s, le, ds, de, sl, dl))
                    opos += length
            blocks.append(Block(btype, final, header_bit, list(lit_lens), list(dist_lens), hlit, hdist, hclen, items, matches,
                                symbols, None, None, start, opos))
        if final:
            break
    return dict(blocks=blocks, out_len=opos, end_byte=(b.pos + 7) // 8)


# ------------------------------------------------------------------------------------------------------------- the table

Case = namedtuple("Case", "name stream out_len expect status zlib_len")
Case.__doc__ = """stream -> expect (out_len bytes), or expect None: the decoders must refuse it.  status: the device decoder's
verdict where the stream has one fault that leads to one answer.  zlib_len: set where the stream itself is valid and only
the asked-for length is not what it inflates to (zlib then returns that many bytes instead of raising)."""

ADLER_BIG = 64 * 65536 + 65


def _rs(seed):
    return np.random.RandomState(seed)


def _ladder(symbols, rotation):
    """Lengths 1, 2, ..., 14, 15, 15 (a complete code) handed to the 16 symbols, rotated."""
    ladder = list(range(1, 15)) + [15, 15]
    return {s: ladder[(i + rotation) % 16] for i, s in enumerate(symbols)}


def _random_tokens(rs, nbytes, have=0):
    """literals and matches that produce exactly nbytes more bytes behind `have` existing ones"""
    tokens, n = [], 0
    while n < nbytes:
        pos = have + n
        if pos == 0 or rs.uniform() < 0.6 or nbytes - n < 3:
            tokens.append(int(rs.randint(256)))
            n += 1
        else:
            length = int(min(nbytes - n, rs.choice([3, 4, 5, 8, 9, 20, 64, 130, 257, 258])))
            dist = int(min(pos, rs.choice([1, 2, 3, 7, 8, 9, 16, 100, 1000, 5000, 32768])))
            tokens.append((length, dist))
            n += length
    return tokens


LADDER_LIT = [0x41 + i for i in range(12)] + [256, 257, 265, 285]
LADDER_DIST = [0, 1, 2, 3, 5, 8, 10, 13, 16, 17, 20, 23, 25, 27, 28, 29]


def _ladder_tokens(first_258):
    """the twelve literals and one match per distance symbol of the ladder; lengths 258, 12, 3, 12, 3, ... are the symbols 285,
    265 (extra bit set) and 257.  With the long match first, all that follows lies in the stream's last 300 bytes."""
    matches = [(258 if i == 0 else 12 if i % 2 else 3, DIST_BASE[d] + (1 << DIST_EXTRA[d]) - 1) for i, d in enumerate(LADDER_DIST)]
    lits = LADDER_LIT[:12]
    return (matches[:1] + lits + matches[1:]) if first_258 else (lits + matches)


def _position_unit(s, u, k):
    a, b = 144 + (u + k) % 100, 32 + (u + k) % 90                  # a nine-bit and an eight-bit literal of the fixed code
    s.fixed([a]).fixed([b]).dynamic([66, 67, 66]).fixed([a]).fixed([a + 1]).fixed([b + 1]).fixed([a])
    s.dynamic([68, (3, 1), 69]).fixed([a]).fixed([b]).fixed([a]).fixed([(4, 2)]).fixed([a]).fixed([a]).fixed([a + 1]).fixed([a])
    return s.stored(bytes([u, k, 7]))


def _position_stream(k):
    """Many small blocks, fixed, dynamic and stored in turn, behind k stored bytes.  A fixed block of one literal is 18 or 19
    bits, so the headers behind a stored block walk through all eight bit phases; a unit ends with a stored block and is
    POSITION_UNIT_BYTES long, so k = 0 .. POSITION_UNIT_BYTES - 1 put every header at every byte and bit, every LEN/NLEN
    and every stored block's end at every byte of the 512-byte input halves.  The last block is an empty stored one."""
    s = Stream().stored(_rs(1000 + k).bytes(k))
    for u in range(-(-1100 // POSITION_UNIT_BYTES)):
        _position_unit(s, u, k)
    return s.stored(b"", final=True)


POSITION_UNIT_BYTES = len(_position_unit(Stream().stored(b"x"), 0, 0).w.data) - 8


def _sized_stream(total, seed):
    """a stream of exactly `total` compressed bytes: a stored block of random bytes, then a short fixed block"""
    rs = _rs(seed)
    s = Stream().stored(rs.bytes(total - 15)).fixed([1, 2], final=True)
    z = s.finish()
    assert len(z) == total
    return bytes(s.out), z


@functools.lru_cache(maxsize=None)
def cases():
    """The table, in a fixed order.  Built once per process."""
    table = []

    def accept(name, s, **kw):
        z = s.finish(**kw) if isinstance(s, Stream) else s[1]
        out = bytes(s.out if isinstance(s, Stream) else s[0])
        table.append(Case(name, z, len(out), out, OK, None))

    def refuse(name, z, out_len, status, zlib_len=None):
        table.append(Case(name, bytes(z), out_len, None, status, zlib_len))

    def both_ends(name, prefix, tokens, **kw):
        """the tokens once with 400 more bytes behind them (the host decoder's fast loop takes them) and once as the end
        of the stream (its careful tail takes the last 300 bytes); a dynamic block, and a fixed one"""
        s = Stream().stored(prefix).dynamic(tokens, **kw).stored(_rs(len(prefix) + 5).bytes(400), final=True)
        accept(name + " / dynamic, more behind", s)
        accept(name + " / fixed, at the end", Stream().stored(prefix).fixed(tokens, final=True, long258=kw.get("long258", False)))

    # ------------------------------------------------------------------------------------------------------ matches
    far = _rs(1).bytes(40_000)
    both_ends("distances 32506 32507 32767 32768, lengths 3 and 258", far,
              [t for d in (32506, 32507, 32767, 32768) for t in ((3, d), 7, (258, d), 9)])
    for d in (32506, 32507, 32767, 32768):                      # and each alone, directly at that output position
        accept(f"distance {d} at output position {d}", Stream().stored(far[:d]).fixed([(258, d), (3, d)], final=True))
    # the window of the device decoder: slot (pos - 32768 + i) & 32767 is slot (pos + i) & 32767
    accept("distance 32768, source run crosses the window wrap",
           Stream().stored(_rs(2).bytes(2 * 32768 - 100)).fixed([(258, 32768), 1, (258, 32768)], final=True))
    accept("distance 32768, destination run crosses the window wrap",
           Stream().stored(_rs(3).bytes(3 * 32768 - 1)).fixed([(3, 32768), (258, 32768)]).stored(_rs(4).bytes(32768 - 261 - 130))
           .dynamic([(258, 32768), (258, 32767), 5], final=True))
    both_ends("distance equal to the output position", _rs(5).bytes(1), [(258, 1), (258, 259), 3, (5, 518)])
    accept("distance equal to the output position, small", Stream().fixed([77, (3, 1), (4, 4), (258, 8), (10, 266)], final=True))
    both_ends("every distance 1 to 258 with length 258", _rs(6).bytes(300), [(258, d) for d in range(1, 259)])
    lens = (3, 4, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258)
    both_ends("run-length copies, distances around 1 8 64", _rs(7).bytes(100),
              [t for d in (1, 2, 7, 8, 9, 63, 64, 65) for n in lens for t in ((n, d), d)])
    both_ends("length 258 as symbol 285", _rs(8).bytes(300), [(258, 1), (258, 7), (258, 300)])
    both_ends("length 258 as symbol 284 with 31 extra", _rs(8).bytes(300), [(258, 1), (258, 7), (258, 300)], long258=True)
    both_ends("every length symbol, extra bits zero and one", _rs(9).bytes(300),
              [t for i in range(29) for t in ((LEN_BASE[i], 9), i, (LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1, 9))])
    both_ends("every distance symbol, extra bits zero and one", far,
              [t for i in range(30) for t in ((5, DIST_BASE[i]), i, (5, DIST_BASE[i] + (1 << DIST_EXTRA[i]) - 1))])

    # -------------------------------------------------------------------------------------------------------- codes
    # sixteen rotations of a 1..15,15 ladder: every literal, the end-of-block code and three length symbols get every code
    # length once, so 10 (last of the primary table), 11 (first behind it) and 15; the same for sixteen distance symbols
    # with 8, 9 and 15
    s = Stream().stored(far)
    for r in range(16):
        s.dynamic(_ladder_tokens(False), lit_lens=_ladder(LADDER_LIT, r), dist_lens=_ladder(LADDER_DIST, r))
    accept("ladder codes, every rotation, more behind", s.stored(_rs(10).bytes(400), final=True))
    for r in range(16):
        accept(f"ladder codes, rotation {r}, at the end",
               Stream().stored(far).dynamic(_ladder_tokens(True), final=True, lit_lens=_ladder(LADDER_LIT, r),
                                            dist_lens=_ladder(LADDER_DIST, r)))
    accept("long codes from skewed frequencies",
           Stream().stored(far[:5000]).dynamic(_skewed_tokens(), final=True))
    text = [int(c) for c in b"code lengths"]
    accept("HLIT 257, HDIST 1", Stream().dynamic(text, final=True, hlit=257, dist_lens=[1], hdist=1))
    full_lit = huffman_lengths([1] * 286, 15)
    full_dist = huffman_lengths([1] * 30, 15)
    accept("HLIT 286, HDIST 30, HCLEN 19",
           Stream().stored(far).dynamic(text + [(258, 32768), (227 + 31, 24577), (3, 1)], final=True, lit_lens=full_lit,
                                        dist_lens=full_dist, hlit=286, hdist=30, hclen=19, long258=True))
    # the smallest HCLEN of a block that can be valid is 5: with four, only the lengths 0 exist and there is no end-of-block
    # code (see the refused "HCLEN 4").  With five, every code is eight bits long: 256 literal/length codes, complete.
    eights = {s_: 8 for s_ in list(range(255)) + [256]}
    accept("HCLEN 5", Stream().dynamic([0, 1, 254, 128], final=True, lit_lens=eights, dist_lens=[0], cl_lens={0: 1, 8: 1}, hclen=5,
                                        rle="plain"))
    accept("single one-bit distance code", Stream().dynamic([65, (258, 1), 66, (3, 1)], final=True, dist_lens=[1], hdist=1))
    accept("no distance code, all literals", Stream().dynamic(text, final=True, dist_lens=[0], hdist=1))
    accept("no distance code, all literals, more behind",
           Stream().dynamic(text * 40, dist_lens=[0], hdist=1).stored(_rs(11).bytes(400), final=True))
    accept("end-of-block code alone: an empty dynamic block",
           Stream().dynamic([], lit_lens={256: 1}, dist_lens=[1, 1]).fixed(text, final=True))
    accept("empty fixed block", Stream().fixed([]).fixed([], final=True))
    accept("empty fixed block only", Stream().fixed([], final=True))
    accept("symbol 16 as the second item",
           Stream().dynamic([0, 1, 2, 3, 3], final=True, lit_lens={0: 3, 1: 3, 2: 3, 3: 3, 256: 1}, dist_lens=[1, 1],
                            rle=[3, (16, 3), (18, 138), (18, 114), 1, 1, 1]))
    accept("symbol 16 behind 17 and 18 repeats zero",
           Stream().dynamic([65, 65], final=True, lit_lens={65: 1, 256: 1}, dist_lens=[1, 1],
                            rle=[(18, 62), (16, 3), 1, (18, 138), (17, 10), (16, 6), (18, 36), 1, 1, 1]))
    accept("a run crosses from the literal lengths into the distance lengths",
           Stream().stored(b"abcdefgh").dynamic([97, (4, 8), 98], final=True, hlit=270,
                                                lit_lens={97: 2, 98: 2, 256: 2, 258: 2}, dist_lens=[0, 0, 0, 0, 0, 1, 1]))
    accept("a repeat of a length crosses from the literal lengths into the distance lengths",
           Stream().dynamic([97, (3, 1), 98], final=True, hlit=258,
                            lit_lens={97: 2, 98: 2, 256: 2, 257: 2}, dist_lens=[2, 2, 2, 2],
                            rle=[(18, 97), 2, 2, (18, 138), (18, 19), 2, (16, 5)]))

    # ---------------------------------------------------------------------------------- input position (device decoder)
    for k in range(POSITION_UNIT_BYTES):
        accept(f"small blocks behind {k} stored bytes", _position_stream(k))
    for m in (1, 2):
        for r in range(-5, 6):
            accept(f"compressed length 512*{m}{r:+d}", _sized_stream(512 * m + r, 20 + r))
    n = len(Stream().stored(bytes(200)).dynamic(_random_tokens(_rs(32), 200, 200), final=True).finish())
    s = Stream().stored(_rs(31).bytes(200 + 514 - n)).dynamic(_random_tokens(_rs(32), 200, 200), final=True)
    assert len(s.w.data) in (509, 510) and len(s.out) >= 400
    accept("trailer straddles byte 512 behind a dynamic block", s)

    # ---------------------------------------------------------------------------------------------- output position
    accept("stored 65535, then distance 32768 and distance 1",
           Stream().stored(_rs(40).bytes(65535)).fixed([(258, 32768), (258, 1), (3, 32768)], final=True))
    accept("stored block crosses the window wrap",
           Stream().stored(_rs(41).bytes(30_000)).stored(_rs(42).bytes(10_000)).fixed([(258, 32768), (100, 5000), (258, 7233)], final=True))
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 299, 300, 301, 5551, 5552, 5553, 5552 + 65, 2 * 5552 + 65, 12 * 5552 + 65):
        accept(f"output of {n} bytes, dynamic", Stream().dynamic(_random_tokens(_rs(50 + n % 97), n), final=True))
        accept(f"output of {n} bytes, fixed", Stream().fixed(_random_tokens(_rs(51 + n % 97), n), final=True))
    accept("output of 5552*6+65 bytes of 0xff", Stream().fixed([255, (258, 1)] + [(258, 1)] * 128 + [(94, 1)], final=True))
    for d in (1, 3, 8, 300):
        for n in (258, 3):
            for gap in (0, 1, 7, 8, 9, 41, 42, 299, 300):
                accept(f"match {n} at distance {d} ends {gap} before the end",
                       Stream().fixed(_random_tokens(_rs(60), 700) + [(n, d)] + [int(v) for v in _rs(61).bytes(gap)], final=True))
            for gap in (0, 1, 5):
                # the same with input left behind it: empty blocks, so that only the output room can end the fast loop
                s = Stream().fixed(_random_tokens(_rs(60), 700) + [(n, d)] + [int(v) for v in _rs(61).bytes(gap)])
                for _ in range(12):
                    s.fixed([])
                accept(f"match {n} at distance {d} ends {gap} before the end, empty blocks behind", s.stored(b"", final=True))

    # -------------------------------------------------------------------------------------------------------- Adler
    accept("Adler: 64*65536+65 random bytes, stored", Stream().stored(_rs(70).bytes(ADLER_BIG), final=True))
    ff = b"\xff" * ADLER_BIG
    accept("Adler: 64*65536+65 bytes 0xff, zlib level 1", (ff, zlib.compress(ff, 1)))

    # ====================================================================================================== refused
    hello = [int(c) for c in b"hello, hello"]
    good = Stream().fixed(hello + [(5, 7)], final=True)
    z_good, n_good = good.finish(), len(good.out)

    # ---- structure
    s = Stream().fixed(hello)
    s.w.put(1, 1), s.w.put(3, 2)
    refuse("block type 3", s.finish(), len(s.out), BAD_BLOCK)
    s = Stream().stored(b"stored bytes", final=True, nlen_field=0xfff2)
    refuse("stored NLEN mismatch", s.finish(), 12, BAD_BLOCK)
    s = Stream().stored(_rs(80).bytes(99), final=True, len_field=100)
    refuse("stored LEN one byte beyond the input", s.finish(trailer=False), 100, INPUT)
    s = Stream().fixed(hello).stored(b"12345678", final=True)
    refuse("stored LEN overruns the output by 1", s.finish(), len(s.out) - 1, OVERRUN, zlib_len=len(s.out))
    # behind the last block the decoder meets the trailer and reads it as a block header: what it then says depends on the
    # checksum's bits, so no single status
    s = Stream().fixed(hello).stored(b"not final")
    refuse("final block missing", s.finish(), len(s.out), None)

    # ---- block header
    lit_ok, dist_ok = {104: 2, 105: 2, 256: 2, 257: 2}, [1, 1]

    def header_only(**kw):
        s = Stream().fixed(hello)
        base = dict(tokens=None, final=True, lit_lens=lit_ok, dist_lens=dist_ok)
        base.update(kw)
        s.dynamic(**base)
        return s.finish(), len(s.out)

    refuse("HLIT 287", *header_only(hlit_field=30), BAD_BLOCK)
    refuse("HLIT 288", *header_only(hlit_field=31), BAD_BLOCK)
    refuse("HDIST 31", *header_only(hdist_field=30), BAD_BLOCK)
    refuse("HDIST 32", *header_only(hdist_field=31), BAD_BLOCK)
    refuse("code-length code over-subscribed", *header_only(cl_lens={0: 1, 1: 1, 2: 1, 18: 2}), BAD_CODE)
    refuse("code-length code incomplete", *header_only(cl_lens={0: 2, 1: 2, 2: 2, 18: 3}), BAD_CODE)
    refuse("HCLEN 4: no length but 0 can be coded", *header_only(lit_lens=[0] * 257, dist_lens=[0], cl_lens={0: 1, 18: 1}, hclen=4), BAD_CODE)
    refuse("symbol 16 as the first item",
           *header_only(rle=[(16, 3), (18, 101), 2, 2, (18, 138), (18, 12), 2, 2, 1, 1], cl_lens={1: 2, 2: 2, 16: 2, 18: 2}), BAD_CODE)
    refuse("a repeat runs 1 past HLIT + HDIST",
           *header_only(lit_lens={104: 2, 105: 2, 256: 1}, hlit=257, rle=[(18, 104), 2, 2, (18, 138), (18, 12), 1, (16, 3)],
                        dist_lens=[1, 1]), BAD_CODE)
    refuse("no end-of-block code", *header_only(lit_lens={104: 1, 105: 1}, hlit=257), BAD_CODE)
    refuse("literal code over-subscribed", *header_only(lit_lens={104: 1, 105: 1, 256: 1}), BAD_CODE)
    refuse("distance code over-subscribed", *header_only(dist_lens=[1, 1, 1]), BAD_CODE)
    refuse("literal code incomplete", *header_only(lit_lens={104: 1, 256: 2}), BAD_CODE)
    refuse("distance code incomplete, more than one code", *header_only(dist_lens=[2, 2]), BAD_CODE)

    # ---- symbols
    for sym in (286, 287):
        s = Stream().fixed(hello + [("s", sym)], final=True)
        refuse(f"fixed block, literal/length symbol {sym}", s.finish(), len(s.out), BAD_CODE)
    for sym in (30, 31):
        s = Stream().fixed(hello + [("m", 257, 0, sym, 0)], final=True)
        refuse(f"fixed block, distance symbol {sym}", s.finish(), len(s.out) + 3, BAD_CODE)
    s = Stream().dynamic(hello + [("s", 257)], final=True, lit_lens=huffman_lengths([1 if c in hello + [256, 257] else 0 for c in range(258)], 15),
                         dist_lens=[0], hdist=1)
    refuse("length symbol in a block without a distance code", s.finish(), len(s.out) + 3, BAD_CODE)
    s = Stream().dynamic(hello + [("s", 257), ("b", 1, 1)], final=True,
                         lit_lens=huffman_lengths([1 if c in hello + [256, 257] else 0 for c in range(258)], 15), dist_lens=[1], hdist=1)
    refuse("the unused half of a lone one-bit distance code", s.finish(), len(s.out) + 3, BAD_CODE)
    s = Stream().fixed([("m", 257, 0, 0, 0)], final=True)
    refuse("distance 1 at output position 0", s.finish(), 3, BAD_DISTANCE)
    s = Stream().stored(far[:32767]).fixed([("m", 257, 0, 29, 8191)], final=True)
    refuse("distance 32768 at output position 32767", s.finish(), 32767 + 3, BAD_DISTANCE)
    s = Stream().fixed(hello + [(258, 3)], final=True)
    refuse("a match overruns the output by 1", s.finish(), len(s.out) - 1, OVERRUN, zlib_len=len(s.out))
    s = Stream().stored(_rs(81).bytes(600)).fixed([(258, 300)] + hello, final=True)
    refuse("a match overruns the output by 1, more behind", s.finish(), 600 + 257, OVERRUN, zlib_len=len(s.out))
    s = Stream().fixed(hello + [(5, 7), 33], final=True)
    refuse("a literal overruns the output by 1", s.finish(), len(s.out) - 1, OVERRUN, zlib_len=len(s.out))

    # ---- the ends of the stream
    refuse("output one byte short", z_good, n_good + 1, SHORT, zlib_len=n_good)
    for k in range(4):
        bad = bytearray(z_good)
        bad[len(bad) - 4 + k] ^= 0x10
        refuse(f"trailer wrong in byte {k}", bad, n_good, CHECKSUM)
    refuse("trailer missing", z_good[:-4], n_good, INPUT)
    refuse("one byte behind the trailer", z_good + b"\x00", n_good, INPUT)
    for name, cmf, flg in (("method 9", 0x79, None), ("window 64 KB", 0x88, None), ("check bits", 0x78, 0x9d),
                           ("preset dictionary", 0x78, 0xbb)):
        s = Stream(cmf, flg).fixed(hello + [(5, 7)], final=True)
        refuse("header: " + name, s.finish(), n_good, BAD_HEADER)

    names = [c.name for c in table]
    assert len(set(names)) == len(names)
    return tuple(table)


def _skewed_tokens():
    """frequencies that fall off geometrically: Huffman lengths up to the 15-bit limit, for literals and for distances"""
    tokens = []
    for i in range(24):
        tokens += [i] * max(1, 16_384 >> i)
    for i in range(20):
        tokens += [(4, DIST_BASE[i])] * max(1, 16_384 >> i)
    order = _rs(12).permutation(len(tokens))
    return [tokens[j] for j in order]


def accepted():
    return [c for c in cases() if c.expect is not None]


def refused():
    return [c for c in cases() if c.expect is None]
