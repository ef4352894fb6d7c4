// C entry points of the row-wise e4m3 UVQK projection (hstu_ln_linear_fp8.cuh).
#include <stdlib.h>

#include "hstu_ln_linear_fp8.cuh"

using namespace hstu;

namespace {
void l8_fill_shape(LnLinearFp8Args& g, int64_t rows, int32_t n) {
  g.rows = rows;
  g.n = n;
  g.n_tiles = n / 32;
  g.units = ((rows + kL8BlockRows - 1) / kL8BlockRows) * g.n_tiles;
}
}  // namespace

extern "C" {

int hstu_ln_linear_fp8_supported(int64_t rows, int32_t k, int32_t n, int dtype) {
  (void)rows;
  return (dtype == HSTU_DTYPE_BF16 || dtype == HSTU_DTYPE_F16) && k == kL8K && n > 0 && n % 32 == 0 && n <= kL8MaxN;
}

int hstu_quantize_rows_fp8(const void* src, int64_t ld, int64_t rows, int32_t k, int dtype, void* dst_q, float* scale, void* stream) {
  if (rows == 0) return HSTU_OK;
  if (!src || !dst_q || !scale) return set_error(HSTU_EINVAL, "quantize_rows_fp8: NULL tensor");
  if (!is_float_dtype(dtype)) return set_error(HSTU_EINVAL, "quantize_rows_fp8: src must be bf16, fp16 or fp32");
  if (k <= 0 || k % 16 != 0 || k > kQ8MaxK)
    return set_error(HSTU_EUNSUPPORTED, "quantize_rows_fp8: k must be a multiple of 16 up to %d (got %d)", kQ8MaxK, k);
  if (rows < 0 || ld < k) return set_error(HSTU_EINVAL, "quantize_rows_fp8: bad rows / leading dimension");
  if ((ld * dtype_bytes(dtype)) % 16 != 0 || (((uintptr_t)src | (uintptr_t)dst_q) & 15) != 0)
    return set_error(HSTU_EINVAL, "quantize_rows_fp8: src and dst_q must be 16-byte aligned, and so must the rows of src");
  const int per = kQ8Threads / 64;
  const int64_t blocks = (rows + per - 1) / per;
  if (blocks > 0x7fffffffLL) return set_error(HSTU_EUNSUPPORTED, "quantize_rows_fp8: too many rows");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(kQ8Threads);
  if (dtype == HSTU_DTYPE_BF16)
    hipLaunchKernelGGL(hstu_quantize_rows_fp8_kernel<bf16_t>, grid, block, 0, st, (const char*)src, ld, rows, k, (uint8_t*)dst_q, scale);
  else if (dtype == HSTU_DTYPE_F16)
    hipLaunchKernelGGL(hstu_quantize_rows_fp8_kernel<f16_t>, grid, block, 0, st, (const char*)src, ld, rows, k, (uint8_t*)dst_q, scale);
  else
    hipLaunchKernelGGL(hstu_quantize_rows_fp8_kernel<float>, grid, block, 0, st, (const char*)src, ld, rows, k, (uint8_t*)dst_q, scale);
  return check_launch("quantize_rows_fp8");
}

int hstu_ln_linear_fp8_fwd(const void* x, int64_t ldx, const void* ln_weight, const void* ln_bias, float eps, const void* wq,
                           const float* w_scale, const void* bias, void* y, int64_t ldy, void* xq, float* x_scale, float* mean,
                           float* rstd, int64_t rows, int32_t k, int32_t n, int dtype, void* stream) {
  if (rows == 0) return HSTU_OK;
  if (!x || !ln_weight || !ln_bias || !wq || !w_scale || !y) return set_error(HSTU_EINVAL, "ln_linear_fp8_fwd: NULL tensor");
  if (!hstu_ln_linear_fp8_supported(rows, k, n, dtype))
    return set_error(HSTU_EUNSUPPORTED, "ln_linear_fp8_fwd: needs bf16 / fp16, k == %d, n a multiple of 32 up to %d (got k %d, n %d, dtype %d)",
                     kL8K, kL8MaxN, k, n, dtype);
  if (rows < 0 || ldx < k || ldy < n) return set_error(HSTU_EINVAL, "ln_linear_fp8_fwd: bad rows / leading dimension");
  if ((ldx | ldy) % 8 != 0 || ((((uintptr_t)x | (uintptr_t)wq | (uintptr_t)y | (uintptr_t)xq)) & 15) != 0)
    return set_error(HSTU_EINVAL, "ln_linear_fp8_fwd: x, wq, y and xq must be 16-byte aligned with leading dimensions that are multiples of 8");
  LnLinearFp8Args g;
  g.x = x; g.ln_w = ln_weight; g.ln_b = ln_bias; g.x_scale_in = nullptr;
  g.wq = wq; g.w_scale = w_scale; g.bias = bias;
  g.y = y; g.xq = xq; g.x_scale = x_scale; g.mean = mean; g.rstd = rstd;
  g.ldx = ldx; g.ldy = ldy; g.eps = eps;
  l8_fill_shape(g, rows, n);
  hipStream_t st = (hipStream_t)stream;
  return dtype == HSTU_DTYPE_BF16 ? launch_ln_linear_fp8<bf16_t>(g, st) : launch_ln_linear_fp8<f16_t>(g, st);
}

// the same kernel without the LayerNorm prologue: the rows arrive as e4m3 codes with their scales
int hstu_linear_fp8_rowwise(const void* xq, const float* x_scale, const void* wq, const float* w_scale, const void* bias, void* y,
                            int64_t ldy, int64_t rows, int32_t k, int32_t n, int out_dtype, void* stream) {
  if (rows == 0) return HSTU_OK;
  if (!xq || !x_scale || !wq || !w_scale || !y) return set_error(HSTU_EINVAL, "linear_fp8_rowwise: NULL tensor");
  if (!hstu_ln_linear_fp8_supported(rows, k, n, out_dtype))
    return set_error(HSTU_EUNSUPPORTED, "linear_fp8_rowwise: needs bf16 / fp16 output, k == %d, n a multiple of 32 up to %d (got k %d, n %d, dtype %d)",
                     kL8K, kL8MaxN, k, n, out_dtype);
  if (rows < 0 || ldy < n) return set_error(HSTU_EINVAL, "linear_fp8_rowwise: bad rows / leading dimension");
  if (ldy % 8 != 0 || ((((uintptr_t)xq | (uintptr_t)wq | (uintptr_t)y)) & 15) != 0)
    return set_error(HSTU_EINVAL, "linear_fp8_rowwise: xq, wq and y must be 16-byte aligned with a leading dimension that is a multiple of 8");
  LnLinearFp8Args g;
  g.x = xq; g.ln_w = nullptr; g.ln_b = nullptr; g.x_scale_in = x_scale;
  g.wq = wq; g.w_scale = w_scale; g.bias = bias;
  g.y = y; g.xq = nullptr; g.x_scale = nullptr; g.mean = nullptr; g.rstd = nullptr;
  g.ldx = kL8K; g.ldy = ldy; g.eps = 0.f;
  l8_fill_shape(g, rows, n);
  hipStream_t st = (hipStream_t)stream;
  return out_dtype == HSTU_DTYPE_BF16 ? launch_ln_linear_fp8<bf16_t>(g, st) : launch_ln_linear_fp8<f16_t>(g, st);
}

}  // extern "C"
