// Launchers of the general attention kernels and the per-dtype switch on the plan's schedule.  Everything a launch needs
// beyond the kernel's instantiation -- grid, LDS bytes, workspace offsets -- comes from the plan (attn_misc.hip).
#pragma once
#include "capi_internal.h"
#include "hstu_attn_bwd_fold.cuh"

namespace hstu {

template <typename T, int DQK, int DV, bool BIAS>
static int launch_fwd_inst(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st) {
  const AttnLaunch& l = pl.launch[0];
  auto kern = hstu_attn_fwd_kernel<T, DQK, DV, BIAS, false>;
  // research-path bias, short sequences: one workgroup per (user, query block) walks the heads with the time buckets of
  // its tile pairs as bytes in LDS (hstu_attn_fwd.cuh)
  if constexpr (BIAS && sizeof(T) == 2) {   // (fp32 I/O: the plain kernel; its head-loop variant spills at 128 x 128)
    if (pl.head_loop) kern = hstu_attn_fwd_kernel<T, DQK, DV, true, true>;
  }
  if constexpr (!BIAS && sizeof(T) == 2 && DQK == DV && (DQK == 64 || DQK == 128)) {
    if (pl.precise) kern = hstu_attn_fwd_kernel<T, DQK, DV, false, false, true>;
  }
  if (int e = reserve_lds((const void*)kern, l.smem, "hstu_attn_fwd")) return e;
  hipLaunchKernelGGL(kern, dim3(l.grid), dim3(kFwdThreads), l.smem, st, p, pl.nqb, l.tables);
  return check_launch("hstu_attn_fwd");
}

// research-path bias on the folded schedule (hstu_attn_bwd_fold_bias_kernel): head dim 64, 16-bit I/O
template <typename T, int D>
static int launch_bwd_fold_bias_inst(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st) {
  const AttnLaunch& l = pl.launch[0];
  auto kern = hstu_attn_bwd_fold_bias_kernel<T, D>;
  if (int e = reserve_lds((const void*)kern, l.smem, "hstu_attn_bwd")) return e;
  float* partial = (float*)((char*)bp.workspace + pl.partial_off);
  int* const next_user = (int*)((char*)bp.workspace + pl.counter_off);
  if (int e = zero_workspace(partial, pl.zero_bytes, st)) return e;
  hipLaunchKernelGGL(kern, dim3(l.grid), dim3(kBwdThreads), l.smem, st, bp, pl.nw, pl.dma_fast ? 1 : 0, partial, l.ts_copies, l.hist, l.tables, next_user);
  if (int rc = check_launch("hstu_attn_bwd(fold, bias)")) return rc;
  return launch_bias_grad_reduce(pl, bp.workspace, 2 * bp.fwd.max_seq_len - 1, bp.dpos_w, bp.dts_w, st);
}

template <typename T, int DQK, int DV, bool BIAS>
static int launch_bwd_inst(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st) {
  const HstuAttnParams& p = bp.fwd;
  const AttnLaunch& l = pl.launch[0];
  auto kern = hstu_attn_bwd_kernel<T, DQK, DV, BIAS>;
  if (int e = reserve_lds((const void*)kern, l.smem, "hstu_attn_bwd")) return e;
  // workspace layout: [fp32 dq accumulator (several key blocks only)] [bias-gradient partial rows] [their chunk sums]
  float* acc = pl.slab_bytes ? (float*)bp.workspace : nullptr;
  float* partial = BIAS ? (float*)((char*)bp.workspace + pl.partial_off) : nullptr;
  const int64_t slab_stride = (int64_t)(pl.slab_bytes / sizeof(float));
  if (int e = zero_workspace(acc, pl.slab_bytes * pl.n_slabs, st)) return e;
  if (int e = zero_workspace(partial, BIAS ? pl.zero_bytes : 0, st)) return e;
  hipLaunchKernelGGL(kern, dim3(l.grid), dim3(kBwdThreads), l.smem, st, bp, pl.nkb, pl.nw, acc, partial, l.ts_copies, l.hist,
                     pl.n_slabs > 1 ? slab_stride : (int64_t)0);   // deterministic: key block kb stores (not adds) into slab kb
  if (int e = check_launch("hstu_attn_bwd")) return e;
  if (acc) {
    hipLaunchKernelGGL(hstu_dq_convert_kernel<T>, dim3(pl.launch[1].grid), dim3(256), 0, st, acc, bp.dq, bp.total_rows, p.heads,
                       p.dqk, bp.dq_row_stride, bp.dq_head_stride, pl.n_slabs, slab_stride);
    if (int e = check_launch("hstu_attn_bwd(dq convert)")) return e;
  }
  if (BIAS) return launch_bias_grad_reduce(pl, bp.workspace, 2 * p.max_seq_len - 1, bp.dpos_w, bp.dts_w, st);
  return HSTU_OK;
}

// the instantiations of the general kernels: every pair of padded head dims without the bias, dqk == dv with it
#define HSTU_DIM_CASES CASE(32, 32) CASE(32, 64) CASE(32, 128) CASE(64, 32) CASE(64, 64) CASE(64, 128) CASE(128, 32) CASE(128, 64) CASE(128, 128)
template <typename T>
static int launch_fwd_general(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st) {
#define CASE(A, V) if (pl.a == A && pl.v == V) return launch_fwd_inst<T, A, V, false>(pl, p, st);
  HSTU_DIM_CASES
#undef CASE
  return HSTU_EUNSUPPORTED;   // (the plan refuses other head dims)
}
template <typename T>
static int launch_bwd_general(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st) {
#define CASE(A, V) if (pl.a == A && pl.v == V) return launch_bwd_inst<T, A, V, false>(pl, bp, st);
  HSTU_DIM_CASES
#undef CASE
  return HSTU_EUNSUPPORTED;
}
#undef HSTU_DIM_CASES

template <typename T>
int launch_fwd_bias(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st) {
  if (pl.a == 32) return launch_fwd_inst<T, 32, 32, true>(pl, p, st);
  if (pl.a == 64) return launch_fwd_inst<T, 64, 64, true>(pl, p, st);
  return launch_fwd_inst<T, 128, 128, true>(pl, p, st);
}
template <typename T>
int launch_bwd_bias(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st) {
  if constexpr (sizeof(T) == 2) {
    if (pl.sched == kSchedFoldBias) return launch_bwd_fold_bias_inst<T, 64>(pl, bp, st);
  }
  if (pl.a == 32) return launch_bwd_inst<T, 32, 32, true>(pl, bp, st);
  if (pl.a == 64) return launch_bwd_inst<T, 64, 64, true>(pl, bp, st);
  return launch_bwd_inst<T, 128, 128, true>(pl, bp, st);
}

// one switch on the plan's schedule for every dtype (the schedules above the general kernels are 16-bit only)
template <typename T>
int launch_attn_fwd(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st) {
  if constexpr (sizeof(T) == 2) {
    if (pl.sched == kSchedSolo) return launch_fwd_solo<T>(pl, p, st);
    if (pl.sched == kSchedSoloBias) return launch_fwd_solo_bias<T>(pl, p, st);
  }
  return pl.bias ? launch_fwd_bias<T>(pl, p, st) : launch_fwd_general<T>(pl, p, st);
}
template <typename T>
int launch_attn_bwd(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st) {
  if constexpr (sizeof(T) == 2) {
    switch (pl.sched) {
      case kSchedSolo: return launch_bwd_solo<T>(pl, bp, st);
      case kSchedSoloBias: return launch_bwd_solo_bias<T>(pl, bp, st);
      case kSchedQuad:
      case kSchedFold: return launch_bwd_fold<T>(pl, bp, st);
      case kSchedLong: return launch_bwd_long<T>(pl, bp, st);
      default: break;
    }
  }
  return pl.bias ? launch_bwd_bias<T>(pl, bp, st) : launch_bwd_general<T>(pl, bp, st);   // kSchedGeneral, kSchedFoldBias
}

}  // namespace hstu
