// Everything the host decides for the int8 row-wise quantized embedding kernels (quant_embedding.hip): the row format's
// offsets, lanes per row, rows per workgroup, passes per row, grid and grid cap.  Host-only, plain C++ with no HIP in it, and
// every function a pure function of its arguments -- the CU count is a parameter, the unit passes cu_count().
// tests/test_quant_embedding_host.py compiles this header alone and sweeps it.
//
// Row format (fbgemm's "fused 8-bit row-wise" arithmetic, row starts aligned for 16-byte loads): a row of `dim` columns is
// `row_stride(dim)` bytes -- codes in [0, dim), fp32 scale at meta_offset(dim), fp32 bias behind it, zeros elsewhere.
//
// A lane owns one PIECE of consecutive codes per pass: piece q = pass * lanes + lane covers code bytes [piece q, piece (q + 1)).
//   quantize: 16 codes -- the lane's one 16-byte store of the quantized row; a row stays inside one wave (its min / max is a
//             wave-level exchange), so rows wider than 64 pieces take a second pass
//   gather:   the codes of ONE 16-byte store of the output, 4 for fp32 and 8 for 16-bit outputs, so that the lanes of a row
//             write consecutive 16-byte pieces; no lane talks to another, so a row may span the whole workgroup
#pragma once
#include <cstdint>

#include "row_slots.h"

namespace hstu {
namespace quant_embedding {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxDim = 2048;
constexpr int kMaxPasses = 2;        // 2048 codes: 128 quantize pieces on 64 lanes, 512 fp32 gather pieces on 256 lanes
constexpr int kQuantizePiece = 16;
constexpr int kGatherChunks = 4;     // chunks of rows a gather workgroup has in flight per loop step (a lane's loads are narrow)
constexpr int kBlocksPerCu = 8;      // 8 x 256 threads = the 32 waves a CU holds; steps beyond the cap are grid-strided

inline bool dim_ok(int dim) { return dim >= 1 && dim <= kMaxDim; }

// the byte offset of scale (bias: + 4) and the bytes of a row
inline int meta_offset(int dim) { return (dim + 3) & ~3; }
inline int row_stride(int dim) { return (meta_offset(dim) + 8 + 15) & ~15; }

// how a workgroup's threads split over rows: the slot rule of row_slots.h on the row's pieces
struct Split {
  int piece;          // codes (= code bytes) a lane owns per pass
  int pieces;         // pieces that hold codes
  int lanes;          // lanes per row, a power of two
  int rows;           // rows per workgroup = one chunk
  int passes;         // passes per row
  int chunks;         // chunks a workgroup takes per loop step
};
inline Split split(int dim, int piece, int max_lanes, int chunks_per_step) {
  Split s;
  s.piece = piece;
  s.pieces = (dim + piece - 1) / piece;
  s.lanes = threads_per_row(s.pieces, max_lanes);
  s.rows = kThreads / s.lanes;
  s.passes = (s.pieces + s.lanes - 1) / s.lanes;
  s.chunks = chunks_per_step;
  return s;
}
inline Split quantize_split(int dim) { return split(dim, kQuantizePiece, kWave, 1); }
inline int gather_piece(int out_elem_bytes) { return 16 / out_elem_bytes; }
inline Split gather_split(int dim, int out_elem_bytes) { return split(dim, gather_piece(out_elem_bytes), kThreads, kGatherChunks); }

// 16-byte pieces of the whole quantized row: the code pieces of the quantize split, or one more (the meta data's)
inline int row_pieces(int dim) { return row_stride(dim) / 16; }

// the first code byte of (lane, pass), or -1 where that lane has no piece in that pass
inline int piece_offset(const Split& s, int lane, int pass) {
  const int q = pass * s.lanes + lane;
  return q < s.pieces ? q * s.piece : -1;
}

// a loop step = s.chunks chunks of s.rows rows; workgroup b takes steps b, b + grid, ..
inline int64_t steps(int64_t n, const Split& s) {
  const int64_t per = (int64_t)s.rows * s.chunks;
  return (n + per - 1) / per;
}
inline int64_t grid_cap(int cus) { return (int64_t)(cus < 1 ? 1 : cus) * kBlocksPerCu; }
inline int grid(int64_t n, const Split& s, int cus) {
  int64_t g = steps(n, s);
  if (g > grid_cap(cus)) g = grid_cap(cus);
  return g < 1 ? 1 : (int)g;
}
// the most steps any workgroup walks
inline int64_t steps_per_workgroup(int64_t n, const Split& s, int cus) {
  const int g = grid(n, s, cus);
  return (steps(n, s) + g - 1) / g;
}

}  // namespace quant_embedding
}  // namespace hstu
