// sweep_layout.hpp - the line-blocked layout of the operands of the longwave mirror sweep (k_rt_lw_bb_mirror<.., .., true>,
// find_g.hip), written once: the host code sizes and fills the blocked copies with it, the kernels address them with it.
// Plain C++ (no HIP in it apart from the host / device marks): tools/check_sweep_layout.cpp includes it as it is.
//
// A row-major matrix [rows][n] of 8-byte elements (a DOUBLE, or a FLOAT pair) whose rows are whole 128-byte lines (n a
// multiple of 16) is stored as [n / 16][rows][16]: the 16 points of a line stay together, and the lines of the `rows` rows
// that belong to the same 16 points follow one another.  Every tile of the mirror sweep starts on a line of every row
// (chunk_layout.hpp), so the 64 points a wave takes from H rows are 4 pieces of H * 128 contiguous bytes instead of H pieces
// of 512 bytes that lie a whole row apart, and a chunk's tiles are read in ascending address order.
#pragma once

#if defined(__HIPCC__)
#define ECCKD_SWEEP_HD __host__ __device__
#else
#define ECCKD_SWEEP_HD
#endif

namespace ecckd {
namespace sweep_layout {

constexpr unsigned long long LINE_PTS = 16;       // 8-byte elements per 128-byte line (chunk_layout::LINE_PTS)
constexpr unsigned long long ELEM_BYTES = 8;
constexpr unsigned long long LINE_BYTES = LINE_PTS * ELEM_BYTES;

// Byte offset of (row r, point i) in the blocked matrix of `rows` rows.
ECCKD_SWEEP_HD inline unsigned long long offset(unsigned long long rows, unsigned long long r, unsigned long long i) {
  return (i / LINE_PTS) * rows * LINE_BYTES + r * LINE_BYTES + (i % LINE_PTS) * ELEM_BYTES;
}

// Byte offset of point i in row 0: what a lane computes once per tile; row r is then the constant r * LINE_BYTES further on.
ECCKD_SWEEP_HD inline unsigned long long point_base(unsigned long long rows, unsigned long long i) { return offset(rows, 0, i); }

// Bytes of the blocked matrix of `rows` rows and n points: those of the row-major one (n is a multiple of LINE_PTS).
ECCKD_SWEEP_HD inline unsigned long long bytes(unsigned long long rows, unsigned long long n) { return n * rows * ELEM_BYTES; }

// A matrix can be blocked if its rows are whole lines.
ECCKD_SWEEP_HD inline bool whole_lines(unsigned long long n) { return n > 0 && n % LINE_PTS == 0; }

// Every offset of the matrix fits 32 bits: the sweep keeps a lane's offset in one register.
ECCKD_SWEEP_HD inline bool fits_32bit(unsigned long long rows, unsigned long long n) { return bytes(rows, n) < (1ULL << 32); }

// An address lies on a line: the sweep's tiles start on a line of every row only if the matrices do.
inline bool on_line(const void* p) { return (unsigned long long)p % LINE_BYTES == 0; }

// A longwave gas of nlay layers and n points may hold the operands of its mirror sweep blocked: the aligned mirror sweep exists
// for 54 and 30 layers and needs the chunks counted from a line (not ECCKD_RT_UNALIGNED), rows of whole lines and offsets
// of 32 bits (the Planck matrix, nlay + 1 rows, is the larger one); ECCKD_RT_ROWMAJOR keeps the row-major matrices.  The
// bases of the matrices must be on_line as well: the caller knows them.
inline bool gas_can_block(int nlay, bool chunks_from_line, bool rowmajor_knob, unsigned long long n) {
  return (nlay == 54 || nlay == 30) && chunks_from_line && !rowmajor_knob && whole_lines(n) &&
         fits_32bit((unsigned long long)nlay + 1, n);
}

// The gas preparation writes the blocked operands itself (k_gas_prep_lw_mirror<.., true>, find_g.hip) where its column-staged
// kernel runs - 54 layers, a FLOAT target spectrum, not the logarithmic method - and the gas can be blocked; with ECCKD_BG64
// the preparation keeps to the row-major DOUBLE rows, which are blocked by a copy afterwards.
inline bool prep_writes_blocked(int nlay, bool od_is_float, bool is_log, bool bg64_knob, bool chunks_from_line, bool rowmajor_knob,
                                unsigned long long n) {
  return nlay == 54 && od_is_float && !is_log && !bg64_knob && gas_can_block(nlay, chunks_from_line, rowmajor_knob, n);
}

}  // namespace sweep_layout
}  // namespace ecckd
