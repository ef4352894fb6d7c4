// The threads of a workgroup as (rows in flight) x (lanes per row): the one statement of the split, for the kernels that
// walk rows with it (jagged_ops.hip, preprocess_ops.hip, research_preprocess.hip) and for the hosts that size their grids
// from it (input_stage_dispatch.h).  Plain C++ outside the __HIPCC__ part: the host tests compile it alone.
#pragma once
#include <cstdint>

namespace hstu {

// lanes per row: the smallest power of two >= units, at most `threads` (a power of two), at least 1
constexpr int threads_per_row(int units, int threads) {
  int tpr = 1;
  while (tpr < units && tpr < threads) tpr <<= 1;
  return tpr;
}
constexpr int rows_in_flight(int units, int threads) { return threads / threads_per_row(units, threads); }

#ifdef __HIPCC__
// a thread's place: lane `lane` of the tpr lanes of row slot `slot` (of rows_par)
struct RowSlots {
  int tpr, rows_par, lane, slot;
};
__device__ __forceinline__ RowSlots row_slots(int units, int threads) {
  RowSlots s;
  s.tpr = threads_per_row(units, threads);
  s.rows_par = threads / s.tpr;
  s.lane = threadIdx.x % s.tpr;
  s.slot = threadIdx.x / s.tpr;
  return s;
}

// the workgroup's slab [r0, r1) of `rows` rows
__device__ __forceinline__ void slab_of(int64_t rows, int64_t* r0, int64_t* r1) {
  const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
  *r0 = (int64_t)blockIdx.x * per;
  *r1 = min(*r0 + per, rows);
}

// the largest b in [0, batch) with off(b) <= r
template <typename F>
__device__ __forceinline__ int find_user(F off, int batch, int64_t r) {
  int lo = 0, hi = batch - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off(mid) <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}
#endif  // __HIPCC__

}  // namespace hstu
