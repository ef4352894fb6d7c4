// Everything the host decides for the input-stage kernels (preprocess_ops.hip, research_preprocess.hip): grids, slab and
// group counts, piece widths, workspace sizes.  Host-only, plain C++ with no HIP in it, and every function a pure function
// of its arguments -- the CU count is a parameter, the units pass cu_count().  tests/test_input_stage_classes_host.py
// compiles this header alone and holds the Python restatement of tests/input_stage_class_cases.py against it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "row_slots.h"

namespace hstu {
namespace input_stage {

// ---------------------------------------------------------------------------------------------------- preprocess_ops.hip
constexpr int kPreThreads = 256;
constexpr int kPreBlocksPerCu = 8;
constexpr int kActionBwdGroupsMax = 512;
constexpr int kActionBwdRowsPerSlot = 8;     // the action backward's slabs: at least 8 rows per row slot
constexpr int kActionBwdWgsPerCu = 2;        // 2 workgroups per CU keep every CU reading
constexpr int kCombineSum = 0, kCombineInterleaveAll = 1;      // HSTU_COMBINE_* (the units assert the equality)

// the grid of the three slab kernels: the resident workgroups, one slab of rows each
inline int resident_blocks(int64_t rows, int rows_par, int cus) {
  int64_t b = (rows + rows_par - 1) / rows_par;
  const int64_t cap = (int64_t)cus * kPreBlocksPerCu;
  if (b > cap) b = cap;
  return b < 1 ? 1 : (int)b;
}

// grid.x of the action backward = the slabs whose partials its finish kernel adds
inline int action_bwd_groups(int64_t rows, int units, int cus) {
  const int rows_par = rows_in_flight(units, kPreThreads);
  int64_t g = (rows + kActionBwdRowsPerSlot * rows_par - 1) / (kActionBwdRowsPerSlot * rows_par);
  const int64_t cap = (int64_t)cus * kActionBwdWgsPerCu;
  if (g > cap) g = cap;
  if (g > kActionBwdGroupsMax) g = kActionBwdGroupsMax;
  return g < 1 ? 1 : (int)g;
}
// grid.y of the action backward: columns of threads_per_row pieces
inline int action_bwd_grid_y(int units) { return (units + kPreThreads - 1) / kPreThreads; }

// grid of its finish kernel: one thread of 256 per column of the two tables
inline int action_bwd_finish_blocks(int width) { return (2 * width + 255) / 256; }

inline size_t action_bwd_workspace_bytes(int32_t width) {
  if (width <= 0) return 0;
  return (size_t)kActionBwdGroupsMax * 2 * (size_t)width * sizeof(float);
}

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d)) & 15) == 0;
}
// Elements per piece, one function per launcher: the 16-byte piece (16 / elem_bytes elements) when it divides the row
// elements -- Da for the action ops, D for combine -- and the pointers THAT launcher's kernel touches in pieces are 16-byte
// aligned (NULL = absent = aligned); 1 otherwise
inline int piece_elems(int row_elems, int elem_bytes, bool aligned) {
  const int N = 16 / elem_bytes;
  return row_elems % N == 0 && aligned ? N : 1;
}
inline int action_fwd_piece(int da, int elem_bytes, const void* table, const void* target_table, const void* out) {
  return piece_elems(da, elem_bytes, aligned16(table, target_table, out));
}
inline int action_bwd_piece(int da, int elem_bytes, const void* d_out, const void* partial) {
  return piece_elems(da, elem_bytes, aligned16(d_out, partial));
}
inline int combine_fwd_piece(int D, int elem_bytes, const void* content, const void* action, const void* contextual,
                             const void* out) {
  return piece_elems(D, elem_bytes, aligned16(content, action, contextual, out));
}
inline int combine_bwd_piece(int D, int elem_bytes, const void* d_out, const void* d_content, const void* d_action,
                             const void* d_contextual) {
  return piece_elems(D, elem_bytes, aligned16(d_out, d_content, d_action, d_contextual));
}

inline int64_t combine_out_rows(int mode, int64_t total_uih, int64_t total_targets, int batch, int C) {
  const int64_t ctx = (int64_t)batch * C;
  if (mode == kCombineSum) return ctx + total_uih + total_targets;
  if (mode == kCombineInterleaveAll) return ctx + 2 * (total_uih + total_targets);
  return ctx + 2 * total_uih + total_targets;
}
// the rows the combine backward walks: the source rows, then the contextual rows when their gradient is asked for
inline int64_t combine_bwd_rows(int64_t total_rows, int batch, int C, bool contextual) {
  return total_rows + (contextual ? (int64_t)batch * C : 0);
}

// ------------------------------------------------------------------------------------------------ research_preprocess.hip
constexpr int kThreads = 256;
constexpr int kMaxUnitBlocks = 1024;      // grid.x cap; the pieces beyond are grid-strided
constexpr int kFwdBlocks = 2048;          // 256 CUs x 8 resident workgroups
constexpr int kBwdBlocks = 2048;
constexpr int kBwdGroupsMax = 64;         // slabs of users whose d_pos partials the finish kernel adds
constexpr int kBwdUsersPerGroupMin = 8;
constexpr int kRatingGroupsMax = 256;
constexpr int kRatingRowsPerGroup = 64;   // the d_rating slabs: at least 64 source rows each
constexpr int kLayoutPlain = 0;           // HSTU_PREPROCESS_PLAIN (the unit asserts the equality)

struct Dims {
  int B, N, Nout, Di, Dr, Do, R, P, layout;
};

inline int unit_blocks(const Dims& d, int V) {
  const int64_t units = (int64_t)d.Nout * (d.Do / V);
  const int64_t b = (units + kThreads - 1) / kThreads;
  return (int)(b > kMaxUnitBlocks ? kMaxUnitBlocks : (b < 1 ? 1 : b));
}

// the user slabs of the forward (and of a backward without d_pos): enough workgroups to fill the chip, at most one per user
inline int fwd_user_groups(const Dims& d, int gx) {
  int groups = (kFwdBlocks + gx - 1) / gx;
  if (groups > d.B) groups = d.B;
  return groups;
}

// the d_pos slabs: enough workgroups to fill the chip, at least kBwdUsersPerGroupMin users each (the partials are traffic).
// Sized from the widest pieces (8 elements: the fewest unit blocks) whatever V is, so that the workspace size depends on the
// shapes alone
inline int bwd_groups(const Dims& d) {
  int64_t ub = ((int64_t)d.Nout * d.Do + 8 * kThreads - 1) / (8 * kThreads);
  ub = ub > kMaxUnitBlocks ? kMaxUnitBlocks : (ub < 1 ? 1 : ub);
  int g = (int)((kBwdBlocks + ub - 1) / ub);
  const int by_users = (d.B + kBwdUsersPerGroupMin - 1) / kBwdUsersPerGroupMin;
  if (g > by_users) g = by_users;
  if (g > kBwdGroupsMax) g = kBwdGroupsMax;
  return g < 1 ? 1 : g;
}

// B users in at most `groups` slabs of *users_per_group: the number of slabs
inline int slab_count(int B, int groups, int* users_per_group) {
  *users_per_group = (B + groups - 1) / groups;
  return (B + *users_per_group - 1) / *users_per_group;
}

inline int rating_groups(const Dims& d) {
  int64_t g = ((int64_t)d.B * d.N + kRatingRowsPerGroup - 1) / kRatingRowsPerGroup;
  if (g > kRatingGroupsMax) g = kRatingGroupsMax;
  return g < 1 ? 1 : (int)g;
}
// grid.z of the rating backward: columns of threads_per_row pieces
inline int rating_grid_z(const Dims& d, int V) {
  const int units = d.Dr / V;
  const int tpr = threads_per_row(units, kThreads);
  return (units + tpr - 1) / tpr;
}

// grids of the two finish kernels: grid-strided over the `total` elements of the position table, one thread per column of
// the rating table
inline int pos_finish_blocks(int64_t total) {
  int64_t blocks = (total + kThreads - 1) / kThreads;
  if (blocks > kFwdBlocks) blocks = kFwdBlocks;
  return (int)blocks;
}
inline int rating_finish_blocks(int width) { return (width + kThreads - 1) / kThreads; }

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t pos_partial_bytes(const Dims& d) { return align256((size_t)bwd_groups(d) * d.Nout * d.Do * sizeof(float)); }
inline size_t rating_partial_bytes(const Dims& d) {
  return d.layout == kLayoutPlain ? 0 : align256((size_t)rating_groups(d) * d.R * d.Dr * sizeof(float));
}

inline bool aligned_to(size_t bytes, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (p && ((uintptr_t)p & (bytes - 1))) return false;
  return true;
}

// the widest piece: at most 16 bytes of the output dtype, dividing every row width, every base pointer aligned to it
inline int pick_vec(const Dims& d, size_t emb_size, size_t out_size, std::initializer_list<const void*> emb_ptrs,
                    std::initializer_list<const void*> out_ptrs) {
  for (int V = (int)(16 / out_size); V > 1; V >>= 1) {
    if (d.Do % V || d.Di % V || (d.layout != kLayoutPlain && d.Dr % V)) continue;
    if (!aligned_to(V * emb_size, emb_ptrs) || !aligned_to(V * out_size, out_ptrs)) continue;
    return V;
  }
  return 1;
}

}  // namespace input_stage
}  // namespace hstu
