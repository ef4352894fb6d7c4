// Launchers of the short-sequence kernels (hstu_attn_solo.cuh): one wave per (user, head).  The plan holds one entry per
// launch: the backward kernels run as two launches by length class, instantiated for one (tpt = 1) or two tiles per tensor.
#pragma once
#include "capi_internal.h"
#include "hstu_attn_solo.cuh"

namespace hstu {

template <typename T>
int launch_fwd_solo(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st) {
  const AttnLaunch& l = pl.launch[0];
  hipLaunchKernelGGL((hstu_attn_fwd_solo_kernel<T, 2>), dim3(l.grid), dim3(kSoloThreads), l.smem, st, p, l.len_lo, l.len_hi);
  return check_launch("hstu_attn_fwd(solo)");
}

template <typename T>
int launch_bwd_solo(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st) {
  for (int i = 0; i < pl.n_launch; ++i) {
    const AttnLaunch& l = pl.launch[i];
    auto kern = l.tpt == 1 ? hstu_attn_bwd_solo_kernel<T, 1> : hstu_attn_bwd_solo_kernel<T, 2>;
    if (int e = reserve_lds((const void*)kern, l.smem, "hstu_attn_bwd")) return e;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(kSoloThreads), l.smem, st, bp, l.len_lo, l.len_hi);
    if (int rc = check_launch("hstu_attn_bwd(solo)")) return rc;
  }
  return HSTU_OK;
}

// research path (relative bias) at the short-sequence shapes
template <typename T>
int launch_fwd_solo_bias(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st) {
  const AttnLaunch& l = pl.launch[0];
  auto kern = hstu_attn_fwd_solo_bias_kernel<T, 2>;
  if (int e = reserve_lds((const void*)kern, l.smem, "hstu_attn_fwd")) return e;
  hipLaunchKernelGGL(kern, dim3(l.grid), dim3(kSoloThreads), l.smem, st, p, l.tables, l.len_lo, l.len_hi);
  return check_launch("hstu_attn_fwd(solo, bias)");
}

template <typename T>
int launch_bwd_solo_bias(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st) {
  float* partial = (float*)((char*)bp.workspace + pl.partial_off);
  if (int e = zero_workspace(partial, pl.zero_bytes, st)) return e;
  for (int i = 0; i < pl.n_launch; ++i) {
    const AttnLaunch& l = pl.launch[i];
    auto kern = l.tpt == 1 ? hstu_attn_bwd_solo_bias_kernel<T, 1> : hstu_attn_bwd_solo_bias_kernel<T, 2>;
    if (int e = reserve_lds((const void*)kern, l.smem, "hstu_attn_bwd")) return e;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(kSoloThreads), l.smem, st, bp, partial, l.ts_copies, l.hist, l.tables, l.len_lo, l.len_hi, l.row0);
    if (int rc = check_launch("hstu_attn_bwd(solo, bias)")) return rc;
  }
  return launch_bias_grad_reduce(pl, bp.workspace, 2 * bp.fwd.max_seq_len - 1, bp.dpos_w, bp.dts_w, st);
}

}  // namespace hstu
