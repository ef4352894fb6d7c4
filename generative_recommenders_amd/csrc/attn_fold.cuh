// Launcher of the folded backward schedule (hstu_attn_bwd_fold.cuh).
#pragma once
// The folded and four-wave backward kernels read every tile of q / k / v / dO exactly once, from one CU: their LDS-DMA requests
// carry the non-temporal hint (-0.5 % M-full, -1.4 % M-jag, bit-identical: profiles/r04_dma_nt.txt).  The forward must NOT: its
// query blocks share a problem's K / V through L2 (+18..24 % with the hint).
#ifndef HSTU_DMA_NT
#define HSTU_DMA_NT 1
#endif
#include "capi_internal.h"
#include "hstu_attn_bwd_quad.cuh"

namespace hstu {

// folded schedule: one persistent workgroup per CU; head dim 64 (kSchedQuad): 4-wave workgroups, two per CU, one per problem
template <typename T>
int launch_bwd_fold(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st) {
  const AttnLaunch& l = pl.launch[0];
  const bool quad = pl.sched == kSchedQuad;
  auto kern = quad ? hstu_attn_bwd_quad_kernel<T, 64> : (pl.a == 128 ? hstu_attn_bwd_fold_kernel<T, 128, 128> : hstu_attn_bwd_fold_kernel<T, 64, 64>);
  if (int e = reserve_lds((const void*)kern, l.smem, "hstu_attn_bwd")) return e;
  hipLaunchKernelGGL(kern, dim3(l.grid), dim3(quad ? kQuadThreads : kBwdThreads), l.smem, st, bp, pl.nw, pl.dma_fast ? 1 : 0);
  return check_launch(quad ? "hstu_attn_bwd(quad)" : "hstu_attn_bwd(fold)");
}

}  // namespace hstu
