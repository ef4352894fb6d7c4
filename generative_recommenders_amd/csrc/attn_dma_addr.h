// When may the folded / four-wave backward kernels address their LDS-DMA requests as (scalar tile base) + 32-bit lane offset
// (hstu_attn_bwd_fold.cuh, fold_tile_dma: row x stride by one 24-bit multiply-add) instead of 64-bit addresses per lane?
// Host-only, plain C++ with no HIP in it: the dispatch plan (attn_misc.hip) asks once per launch and hands the answer to the
// kernel as an argument; tests/test_attn_dma_addr_host.py compiles this header alone.
//
// The answer depends on nothing but the four row strides and the longest sequence the launch takes (32 x tmax rows): launch
// constants.  The kernels used to evaluate it per problem; the last 64-bit compare's constant lived in a spilled register
// pair, and its reload (a scratch load + s_waitcnt vmcnt(0)) stood in front of every problem's first request
// (docs/EXPERIMENTS.md R21).
#pragma once
#include <cstdint>

namespace hstu {

constexpr int64_t kDmaStrideLimit = int64_t(1) << 24;   // v_mul_u32_u24: row and stride below 2^24 each
constexpr int64_t kDmaSpanLimit = int64_t(1) << 32;     // 32-bit offset: a sequence's rows within 4 GiB of its first

// one tensor: rows [0, len_max) of `row_stride_bytes` each
inline bool dma_fast_tensor(int64_t row_stride_bytes, int64_t len_max) {
  return row_stride_bytes < kDmaStrideLimit && len_max * row_stride_bytes < kDmaSpanLimit;
}

// all four tensors a backward problem requests tiles of (strides in bytes; len_max = 32 x tmax)
inline bool attn_bwd_dma_fast(int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t do_rs, int64_t len_max) {
  return dma_fast_tensor(q_rs, len_max) && dma_fast_tensor(k_rs, len_max) && dma_fast_tensor(v_rs, len_max) &&
         dma_fast_tensor(do_rs, len_max);
}

}  // namespace hstu
