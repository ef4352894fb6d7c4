// e4m3 attention forward and the jagged e4m3 quantizer (hstu_attn_fwd_fp8.cuh).
#include "capi_internal.h"
#include "hstu_attn_fwd_fp8.cuh"

namespace hstu {

template <int D>
static int launch_fwd_fp8_inst(const HstuAttnParams& p, const HstuFp8Descale& ds, hipStream_t st) {
  const int q_rows = p.delta_q > 0 ? p.delta_q : p.max_seq_len;
  const int nqb = (q_rows + kFwdRowsPerBlock - 1) / kFwdRowsPerBlock;
  const int groups = (p.batch * p.heads + 7) / 8;
  hipLaunchKernelGGL(hstu_attn_fwd_fp8_kernel<D>, dim3(groups * 8 * nqb), dim3(kFwdThreads), Fp8FwdCfg<D>::SMEM, st, p, ds, nqb);
  return check_launch("hstu_attn_fwd_fp8");
}

int launch_attn_fwd_fp8(const HstuAttnParams& p, const HstuFp8Descale& ds, hipStream_t st) {
  switch (fp8_head_dim(p.dqk)) {
    case 64: return launch_fwd_fp8_inst<64>(p, ds, st);
    case 128: return launch_fwd_fp8_inst<128>(p, ds, st);
    default: return set_error(HSTU_EUNSUPPORTED, "hstu_attn_fwd: fp8 head dim %d not instantiated", p.dqk);
  }
}

template <typename T>
static int launch_quantize_fp8_dtype(const void* x, int64_t rs, int64_t hs, void* x8, float* descale, const void* offsets, int batch,
                                     int heads, int dim, int index_dtype, hipStream_t st) {
  const bool vec = dim % 8 == 0 && ((rs | hs) * (int64_t)sizeof(T)) % 16 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)x8 & 7) == 0;
  auto kern = vec ? hstu_jagged_quantize_fp8_kernel<T, true> : hstu_jagged_quantize_fp8_kernel<T, false>;
  hipLaunchKernelGGL(kern, dim3(batch * heads), dim3(kQuantThreads), 0, st, (const char*)x, rs, hs, (uint8_t*)x8, descale, offsets,
                     index_dtype, heads, dim);
  return check_launch("hstu_jagged_quantize_fp8");
}

int launch_jagged_quantize_fp8(const void* x, int64_t rs, int64_t hs, void* x8, float* descale, const void* offsets, int batch, int heads,
                               int dim, int dtype, int index_dtype, hipStream_t st) {
  switch (dtype) {
    case HSTU_DTYPE_BF16: return launch_quantize_fp8_dtype<bf16_t>(x, rs, hs, x8, descale, offsets, batch, heads, dim, index_dtype, st);
    case HSTU_DTYPE_F16: return launch_quantize_fp8_dtype<f16_t>(x, rs, hs, x8, descale, offsets, batch, heads, dim, index_dtype, st);
    default: return launch_quantize_fp8_dtype<float>(x, rs, hs, x8, descale, offsets, batch, heads, dim, index_dtype, st);
  }
}

}  // namespace hstu
