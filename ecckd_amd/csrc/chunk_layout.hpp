// chunk_layout.hpp - how an interval of the error sweep (K5c, find_g.hip) is cut into chunks, written once: eval_intervals
// lays the batch out with it, the sweep kernels find a chunk's points with it.  Plain C++ (no HIP in it apart from the
// host / device marks): tools/check_chunk_layout.cpp includes it as it is.
//
// A chunk is what one block sums by itself into its own row of partials.  The layout is a function of the interval alone -
// its first index and its length -, so an interval's error has the same bits whether it is evaluated alone, beside its
// neighbours or beside other bands' intervals, and the memo keyed on the interval stays valid.
//
// aligned: the chunks are counted from the 128-byte line that holds the interval's first point, A = i1 - head with
// head = i1 mod LINE_PTS, so that every tile of every chunk starts on a line (a wave's 64 doubles of a row are then four
// whole lines instead of five touched); the `head` points below i1 are dead lanes of the first chunk's first tile.
// Not aligned: head = 0, the chunks are counted from i1.
#pragma once

#if defined(__HIPCC__)
#define ECCKD_CHUNK_HD __host__ __device__
#else
#define ECCKD_CHUNK_HD
#endif

namespace ecckd {
namespace chunk_layout {

constexpr long long LINE_PTS = 16;      // doubles (and FLOAT pairs) per 128-byte line
constexpr int COST_GROUPS = 64;         // the cost kernels (K5d) add an interval's chunk partials in groups of 32 and have room for
                                        // this many groups: an interval may have at most 32 * COST_GROUPS chunks

// Chunk size of `len` points: the smallest multiple of `gran` that covers them with at most `blocks` chunks.
ECCKD_CHUNK_HD inline long long interval_chunk_pts(long long len, long long blocks, long long gran) {
  long long c = (len + blocks - 1) / blocks;
  c = (c + gran - 1) / gran * gran;
  return c < gran ? gran : c;
}

struct Layout {
  long long chunk_pts;   // points per chunk, a multiple of gran
  long long head;        // points between the aligned origin and i1: 0 .. LINE_PTS - 1
  long long nchunks;     // ceil((len + head) / chunk_pts) <= blocks
};

// The chunks of the interval [i1, i2] (inclusive) for one round of `target_blocks` blocks of `gran` points per iteration.
ECCKD_CHUNK_HD inline Layout of_interval(long long i1, long long i2, long long target_blocks, long long gran, bool aligned) {
  Layout L;
  L.head = aligned ? i1 % LINE_PTS : 0;
  const long long span = i2 - i1 + 1 + L.head;
  L.chunk_pts = interval_chunk_pts(span, target_blocks, gran);
  L.nchunks = (span + L.chunk_pts - 1) / L.chunk_pts;
  return L;
}

struct Span {
  long long base;        // where the chunk's first tile begins: A + c * chunk_pts (below i1 only in chunk 0, by `head` points)
  long long p0, p1;      // the chunk's points, inclusive: never empty for c < nchunks
};

// Chunk c of the interval [i1, i2] laid out with (chunk_pts, head).
ECCKD_CHUNK_HD inline Span chunk_span(long long i1, long long i2, long long chunk_pts, long long head, long long c) {
  Span s;
  s.base = i1 - head + c * chunk_pts;
  s.p0 = s.base < i1 ? i1 : s.base;
  s.p1 = s.base + chunk_pts - 1;
  if (s.p1 > i2) s.p1 = i2;
  return s;
}

}  // namespace chunk_layout
}  // namespace ecckd
