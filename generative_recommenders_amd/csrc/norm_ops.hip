// Row-wise normalisation kernels around the HSTU projections (gfx950, HBM-bound).
//
// One wavefront owns one row at a time (grid-stride over rows): each lane loads its
// 16-byte pieces of the row once, keeps them in registers, reduces with wave shuffles,
// and writes once.  Weight gradients are accumulated per lane across all the rows a
// wave visits (lanes own fixed columns), reduced across the workgroup's waves through
// LDS and written as one fp32 partial per workgroup; a second small kernel sums the
// partials.  All math is fp32, outputs are cast to the I/O dtype, like the reference:
//   ops/pytorch/pt_layer_norm.py:24-38, ops/pytorch/pt_hstu_linear.py:23-65;
// kernels replaced: ops/triton/triton_layer_norm.py:77-309, :525-749 (RMS norm),
// ops/triton/triton_hstu_linear.py:48-337 (LN * u), :570-1036 (GroupNorm * u).
// The pieces and the wave sum are row_pass.cuh's, the grid rule capi_internal.h's (resident_row_blocks): shared with the
// later row-pass ops (multitask_ops.hip, time_ln_ops.hip, loss_ops.hip).
#include "row_pass.cuh"
#include "drop_hash.cuh"
#include "capi_internal.h"
#include "norm_dispatch.h"

namespace hstu {
// narrow / wide instances of every kernel and launcher (norm_kernels.inc)
namespace nw1 {
#define NORM_WIDE 1
#include "norm_kernels.inc"
#undef NORM_WIDE
}  // namespace nw1
namespace nw4 {
#define NORM_WIDE 4
#include "norm_kernels.inc"
#undef NORM_WIDE
}  // namespace nw4
// Every entry point below asks norm_dispatch.h ONCE for the class of its call -- piece width from all the facts its
// kernels depend on, then the narrow instance for rows of up to 1024 elements at the vector width (512 at the scalar
// width) and the wide one above, refused past 4096 (2048) -- and passes that class on to the instance's launcher.
using nw1::kMaxNormBlocks;
using nw1::silu_launch;
using norm_dispatch::RowClass;
static int accept_row(const RowClass& k, int dim, const char* who) {
  if (dim <= 0) return set_error(HSTU_EINVAL, "%s: dim must be positive", who);
  if (norm_dispatch::refused(k, dim))
    return set_error(HSTU_EUNSUPPORTED, "%s: dim %d exceeds the %d supported with this alignment", who, dim, k.limit);
  return HSTU_OK;
}
}  // namespace hstu

using namespace hstu;

#define DISPATCH_DTYPE(dtype, CALL_BF16, CALL_F16, CALL_F32)                          \
  switch (dtype) {                                                                    \
    case HSTU_DTYPE_BF16: return CALL_BF16;                                           \
    case HSTU_DTYPE_F16: return CALL_F16;                                             \
    case HSTU_DTYPE_F32: return CALL_F32;                                             \
    default: return set_error(HSTU_EINVAL, "dtype must be bf16, fp16 or fp32");       \
  }

// (cls.wide ? nw4::CALL : nw1::CALL): the row kernels' narrow or wide instance
#define NW(cls, ...) ((cls).wide ? nw4::__VA_ARGS__ : nw1::__VA_ARGS__)

extern "C" {

size_t hstu_norm_bwd_workspace_bytes(int64_t rows, int32_t dim) {
  (void)rows;
  return (size_t)kMaxNormBlocks * 2 * (size_t)dim * sizeof(float);
}

int hstu_layer_norm_fwd(const void* x, const void* weight, const void* bias, void* y, float* mean, float* rstd,
                        int64_t rows, int32_t dim, float eps, int dtype, void* stream) {
  if (rows == 0) return HSTU_OK;
  if (!x || !weight || !bias || !y) return set_error(HSTU_EINVAL, "layer_norm_fwd: NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  const RowClass k = norm_dispatch::ln_fwd_class(dim, dtype_bytes(dtype), x, weight, bias, y);
  if (int e = accept_row(k, dim, "layer_norm_fwd")) return e;
  DISPATCH_DTYPE(dtype, NW(k, ln_fwd<bf16_t>(k, x, weight, bias, y, mean, rstd, rows, dim, eps, st)),
                 NW(k, ln_fwd<f16_t>(k, x, weight, bias, y, mean, rstd, rows, dim, eps, st)),
                 NW(k, ln_fwd<float>(k, x, weight, bias, y, mean, rstd, rows, dim, eps, st)));
}

int hstu_layer_norm_bwd(const void* dy, const void* x, const void* weight, const float* mean, const float* rstd,
                        void* dx, float* dweight, float* dbias, float* partial_ws, int64_t rows, int32_t dim, int dtype,
                        void* stream) {
  return hstu_layer_norm_bwd_residual(dy, x, weight, mean, rstd, nullptr, dx, dweight, dbias, partial_ws, rows, dim, dtype, stream);
}

int hstu_layer_norm_bwd_residual(const void* dy, const void* x, const void* weight, const float* mean, const float* rstd,
                                 const void* dresidual, void* dx, float* dweight, float* dbias, float* partial_ws,
                                 int64_t rows, int32_t dim, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const void* dres = dresidual;
  if (!dweight || !dbias) return set_error(HSTU_EINVAL, "layer_norm_bwd: dweight/dbias are required");
  if (rows == 0) {
    (void)hipMemsetAsync(dweight, 0, dim * sizeof(float), st);
    (void)hipMemsetAsync(dbias, 0, dim * sizeof(float), st);
    return HSTU_OK;
  }
  if (!dy || !x || !weight || !mean || !rstd || !dx || !partial_ws) return set_error(HSTU_EINVAL, "layer_norm_bwd: NULL tensor");
  const RowClass k = norm_dispatch::ln_bwd_class(dim, dtype_bytes(dtype), dy, x, weight, nullptr, dres, dx);
  if (int e = accept_row(k, dim, "layer_norm_bwd")) return e;
  DISPATCH_DTYPE(dtype, NW(k, ln_bwd<bf16_t>(k, dy, x, weight, mean, rstd, dx, dweight, dbias, partial_ws, rows, dim, dres, st)),
                 NW(k, ln_bwd<f16_t>(k, dy, x, weight, mean, rstd, dx, dweight, dbias, partial_ws, rows, dim, dres, st)),
                 NW(k, ln_bwd<float>(k, dy, x, weight, mean, rstd, dx, dweight, dbias, partial_ws, rows, dim, dres, st)));
}

// y = x * sigmoid(LayerNorm(x)): the gate in front of the preprocessors' and DlrmHSTU's MLPs (SwishLayerNorm)
int hstu_swish_layer_norm_fwd(const void* x, const void* weight, const void* bias, void* y, float* mean, float* rstd,
                              int64_t rows, int32_t dim, float eps, int dtype, void* stream) {
  if (rows == 0) return HSTU_OK;
  if (!x || !weight || !bias || !y) return set_error(HSTU_EINVAL, "swish_layer_norm_fwd: NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  const RowClass k = norm_dispatch::ln_fwd_class(dim, dtype_bytes(dtype), x, weight, bias, y);
  if (int e = accept_row(k, dim, "swish_layer_norm_fwd")) return e;
  DISPATCH_DTYPE(dtype, NW(k, ln_fwd<bf16_t, true>(k, x, weight, bias, y, mean, rstd, rows, dim, eps, st)),
                 NW(k, ln_fwd<f16_t, true>(k, x, weight, bias, y, mean, rstd, rows, dim, eps, st)),
                 NW(k, ln_fwd<float, true>(k, x, weight, bias, y, mean, rstd, rows, dim, eps, st)));
}

int hstu_swish_layer_norm_bwd(const void* dy, const void* x, const void* weight, const void* bias, const float* mean,
                              const float* rstd, void* dx, float* dweight, float* dbias, float* partial_ws, int64_t rows,
                              int32_t dim, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!dweight || !dbias) return set_error(HSTU_EINVAL, "swish_layer_norm_bwd: dweight/dbias are required");
  if (rows == 0) {
    (void)hipMemsetAsync(dweight, 0, dim * sizeof(float), st);
    (void)hipMemsetAsync(dbias, 0, dim * sizeof(float), st);
    return HSTU_OK;
  }
  if (!dy || !x || !weight || !bias || !mean || !rstd || !dx || !partial_ws) return set_error(HSTU_EINVAL, "swish_layer_norm_bwd: NULL tensor");
  const RowClass k = norm_dispatch::ln_bwd_class(dim, dtype_bytes(dtype), dy, x, weight, bias, nullptr, dx);
  if (int e = accept_row(k, dim, "swish_layer_norm_bwd")) return e;
  DISPATCH_DTYPE(dtype, NW(k, ln_bwd<bf16_t, true>(k, dy, x, weight, mean, rstd, dx, dweight, dbias, partial_ws, rows, dim, nullptr, st, bias)),
                 NW(k, ln_bwd<f16_t, true>(k, dy, x, weight, mean, rstd, dx, dweight, dbias, partial_ws, rows, dim, nullptr, st, bias)),
                 NW(k, ln_bwd<float, true>(k, dy, x, weight, mean, rstd, dx, dweight, dbias, partial_ws, rows, dim, nullptr, st, bias)));
}

// y = x rstd weight, rstd = 1 / sqrt(mean(x^2) + eps): RMSNorm (rms kernels of norm_kernels.inc)
int hstu_rms_norm_fwd(const void* x, const void* weight, void* y, float* rstd, int64_t rows, int32_t dim, float eps, int dtype,
                      void* stream) {
  if (dim <= 0) return set_error(HSTU_EINVAL, "rms_norm_fwd: dim must be positive");
  if (rows == 0) return HSTU_OK;
  if (!x || !weight || !y) return set_error(HSTU_EINVAL, "rms_norm_fwd: NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  const RowClass k = norm_dispatch::rms_fwd_class(dim, dtype_bytes(dtype), x, weight, y);
  if (int e = accept_row(k, dim, "rms_norm_fwd")) return e;
  DISPATCH_DTYPE(dtype, NW(k, rms_fwd<bf16_t>(k, x, weight, y, rstd, rows, dim, eps, st)),
                 NW(k, rms_fwd<f16_t>(k, x, weight, y, rstd, rows, dim, eps, st)),
                 NW(k, rms_fwd<float>(k, x, weight, y, rstd, rows, dim, eps, st)));
}

int hstu_rms_norm_bwd(const void* dy, const void* x, const void* weight, const float* rstd, void* dx, float* dweight,
                      float* partial_ws, int64_t rows, int32_t dim, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!dweight) return set_error(HSTU_EINVAL, "rms_norm_bwd: dweight is required");
  if (dim <= 0) return set_error(HSTU_EINVAL, "rms_norm_bwd: dim must be positive");
  if (rows == 0) {
    (void)hipMemsetAsync(dweight, 0, dim * sizeof(float), st);
    return HSTU_OK;
  }
  if (!dy || !x || !weight || !rstd || !dx || !partial_ws) return set_error(HSTU_EINVAL, "rms_norm_bwd: NULL tensor");
  const RowClass k = norm_dispatch::rms_bwd_class(dim, dtype_bytes(dtype), dy, x, weight, dx);
  if (int e = accept_row(k, dim, "rms_norm_bwd")) return e;
  DISPATCH_DTYPE(dtype, NW(k, rms_bwd<bf16_t>(k, dy, x, weight, rstd, dx, dweight, partial_ws, rows, dim, st)),
                 NW(k, rms_bwd<f16_t>(k, dy, x, weight, rstd, dx, dweight, partial_ws, rows, dim, st)),
                 NW(k, rms_bwd<float>(k, dy, x, weight, rstd, dx, dweight, partial_ws, rows, dim, st)));
}

static int drop_ratio_ok(float r, const char* who) {
  if (!(r >= 0.f && r < 1.f)) return set_error(HSTU_EINVAL, "%s: dropout_ratio must be in [0, 1) (got %g)", who, (double)r);
  return HSTU_OK;
}

int hstu_norm_mul_dropout_fwd(const void* attn, const void* u, const void* weight, const void* bias, void* y, float* mean,
                              float* rstd, int64_t rows, int32_t heads, int32_t head_dim, float eps, int group_norm,
                              int concat_ux, float dropout_ratio, uint64_t seed, int dtype, void* stream) {
  return hstu_norm_mul_silu_fwd(attn, u, (int64_t)heads * head_dim, 0, weight, bias, y, mean, rstd, rows, heads, head_dim, eps,
                                group_norm, concat_ux, dropout_ratio, seed, dtype, stream);
}

int hstu_norm_mul_silu_fwd(const void* attn, const void* u, int64_t u_row_stride, int u_is_preactivation, const void* weight,
                           const void* bias, void* y, float* mean, float* rstd, int64_t rows, int32_t heads,
                           int32_t head_dim, float eps, int group_norm, int concat_ux, float dropout_ratio, uint64_t seed,
                           int dtype, void* stream) {
  if (int e = drop_ratio_ok(dropout_ratio, "norm_mul_dropout_fwd")) return e;
  if (u_row_stride < (int64_t)heads * head_dim) return set_error(HSTU_EINVAL, "norm_mul_fwd: u_row_stride is smaller than a row");
  const bool silu = u_is_preactivation != 0;
  if (rows == 0) return HSTU_OK;
  if (!attn || !u || !weight || !bias || !y) return set_error(HSTU_EINVAL, "norm_mul_fwd: NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  const RowClass k = norm_dispatch::nm_fwd_class(heads, head_dim, dtype_bytes(dtype), group_norm != 0, attn, u, u_row_stride, weight, bias, y);
  if (int e = accept_row(k, heads * head_dim, "norm_mul_fwd")) return e;
#define NM_FWD(T) (k.wide ? nw4::nm_fwd<T>(k, attn, u, weight, bias, y, mean, rstd, rows, heads, head_dim, eps, group_norm, concat_ux, nw4::make_drop_ctx(dropout_ratio, seed), u_row_stride, silu, st) \
                      : nw1::nm_fwd<T>(k, attn, u, weight, bias, y, mean, rstd, rows, heads, head_dim, eps, group_norm, concat_ux, nw1::make_drop_ctx(dropout_ratio, seed), u_row_stride, silu, st))
  DISPATCH_DTYPE(dtype, NM_FWD(bf16_t), NM_FWD(f16_t), NM_FWD(float));
#undef NM_FWD
}

int hstu_norm_mul_fwd(const void* attn, const void* u, const void* weight, const void* bias, void* y, float* mean,
                      float* rstd, int64_t rows, int32_t heads, int32_t head_dim, float eps, int group_norm,
                      int concat_ux, int dtype, void* stream) {
  return hstu_norm_mul_dropout_fwd(attn, u, weight, bias, y, mean, rstd, rows, heads, head_dim, eps, group_norm, concat_ux,
                                   0.f, 0, dtype, stream);
}

int hstu_norm_mul_bwd(const void* dy, const void* attn, const void* u, const void* weight, const void* bias,
                      const float* mean, const float* rstd, void* dattn, void* du, float* dweight, float* dbias,
                      float* partial_ws, int64_t rows, int32_t heads, int32_t head_dim, int group_norm, int concat_ux,
                      int dtype, void* stream) {
  return hstu_norm_mul_dropout_bwd(dy, attn, u, weight, bias, mean, rstd, dattn, du, dweight, dbias, partial_ws, rows, heads,
                                   head_dim, group_norm, concat_ux, 0.f, 0, dtype, stream);
}

int hstu_norm_mul_dropout_bwd(const void* dy, const void* attn, const void* u, const void* weight, const void* bias,
                              const float* mean, const float* rstd, void* dattn, void* du, float* dweight, float* dbias,
                              float* partial_ws, int64_t rows, int32_t heads, int32_t head_dim, int group_norm,
                              int concat_ux, float dropout_ratio, uint64_t seed, int dtype, void* stream) {
  const int64_t dim = (int64_t)heads * head_dim;
  return hstu_norm_mul_silu_bwd(dy, attn, u, dim, 0, weight, bias, mean, rstd, dattn, du, dim, dweight, dbias, partial_ws, rows,
                                heads, head_dim, group_norm, concat_ux, dropout_ratio, seed, dtype, stream);
}

int hstu_norm_mul_silu_bwd(const void* dy, const void* attn, const void* u, int64_t u_row_stride, int u_is_preactivation,
                           const void* weight, const void* bias, const float* mean, const float* rstd, void* dattn, void* du,
                           int64_t du_row_stride, float* dweight, float* dbias, float* partial_ws, int64_t rows,
                           int32_t heads, int32_t head_dim, int group_norm, int concat_ux, float dropout_ratio,
                           uint64_t seed, int dtype, void* stream) {
  if (int e = drop_ratio_ok(dropout_ratio, "norm_mul_dropout_bwd")) return e;
  if (u_row_stride < (int64_t)heads * head_dim || du_row_stride < (int64_t)heads * head_dim)
    return set_error(HSTU_EINVAL, "norm_mul_bwd: a row stride is smaller than a row");
  const bool silu = u_is_preactivation != 0;
  hipStream_t st = (hipStream_t)stream;
  const int width = group_norm ? heads : heads * head_dim;
  if (!dweight || !dbias) return set_error(HSTU_EINVAL, "norm_mul_bwd: dweight/dbias are required");
  if (rows == 0) {
    (void)hipMemsetAsync(dweight, 0, width * sizeof(float), st);
    (void)hipMemsetAsync(dbias, 0, width * sizeof(float), st);
    return HSTU_OK;
  }
  if (!dy || !attn || !u || !weight || !bias || !mean || !rstd || !dattn || !du || !partial_ws)
    return set_error(HSTU_EINVAL, "norm_mul_bwd: NULL tensor");
  const RowClass k = norm_dispatch::nm_bwd_class(heads, head_dim, dtype_bytes(dtype), group_norm != 0, dy, attn, u, u_row_stride, weight, bias,
                                                 dattn, du, du_row_stride);
  if (int e = accept_row(k, heads * head_dim, "norm_mul_bwd")) return e;
#define NM_BWD(T) (k.wide ? nw4::nm_bwd<T>(k, dy, attn, u, weight, bias, mean, rstd, dattn, du, dweight, dbias, partial_ws, rows, heads, head_dim, group_norm, concat_ux, nw4::make_drop_ctx(dropout_ratio, seed), u_row_stride, du_row_stride, silu, st) \
                      : nw1::nm_bwd<T>(k, dy, attn, u, weight, bias, mean, rstd, dattn, du, dweight, dbias, partial_ws, rows, heads, head_dim, group_norm, concat_ux, nw1::make_drop_ctx(dropout_ratio, seed), u_row_stride, du_row_stride, silu, st))
  DISPATCH_DTYPE(dtype, NM_BWD(bf16_t), NM_BWD(f16_t), NM_BWD(float));
#undef NM_BWD
}

int hstu_silu_fwd(const void* in, void* out, int64_t rows, int32_t cols, int64_t in_row_stride, int64_t out_row_stride,
                  int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool vk = norm_dispatch::silu_vector(dtype_bytes(dtype), cols, nullptr, in, out, 0, in_row_stride, out_row_stride);
  DISPATCH_DTYPE(dtype, (silu_launch<bf16_t, false>(vk, nullptr, in, out, rows, cols, 0, in_row_stride, out_row_stride, st)),
                 (silu_launch<f16_t, false>(vk, nullptr, in, out, rows, cols, 0, in_row_stride, out_row_stride, st)),
                 (silu_launch<float, false>(vk, nullptr, in, out, rows, cols, 0, in_row_stride, out_row_stride, st)));
}

int hstu_silu_bwd(const void* dout, const void* in, void* din, int64_t rows, int32_t cols, int64_t dout_row_stride,
                  int64_t in_row_stride, int64_t din_row_stride, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool vk = norm_dispatch::silu_vector(dtype_bytes(dtype), cols, dout, in, din, dout_row_stride, in_row_stride, din_row_stride);
  DISPATCH_DTYPE(dtype, (silu_launch<bf16_t, true>(vk, dout, in, din, rows, cols, dout_row_stride, in_row_stride, din_row_stride, st)),
                 (silu_launch<f16_t, true>(vk, dout, in, din, rows, cols, dout_row_stride, in_row_stride, din_row_stride, st)),
                 (silu_launch<float, true>(vk, dout, in, din, rows, cols, dout_row_stride, in_row_stride, din_row_stride, st)));
}


int hstu_l2_norm_fwd(const void* x, void* y, int64_t rows, int32_t dim, float eps, int dtype, void* stream) {
  if (rows > 0 && (!x || !y)) return set_error(HSTU_EINVAL, "hstu_l2_norm_fwd: x and y must be non-NULL");
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0) return HSTU_OK;
  const RowClass k = norm_dispatch::l2_class(dim, dtype_bytes(dtype), x, nullptr, y);
  if (int e = accept_row(k, dim, "l2_norm")) return e;
  DISPATCH_DTYPE(dtype, NW(k, l2_launch<bf16_t, false>(k, x, nullptr, y, rows, dim, eps, st)),
                 NW(k, l2_launch<f16_t, false>(k, x, nullptr, y, rows, dim, eps, st)),
                 NW(k, l2_launch<float, false>(k, x, nullptr, y, rows, dim, eps, st)));
}

int hstu_l2_norm_bwd(const void* dy, const void* x, void* dx, int64_t rows, int32_t dim, float eps, int dtype, void* stream) {
  if (rows > 0 && (!x || !dy || !dx)) return set_error(HSTU_EINVAL, "hstu_l2_norm_bwd: dy, x and dx must be non-NULL");
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0) return HSTU_OK;
  const RowClass k = norm_dispatch::l2_class(dim, dtype_bytes(dtype), x, dy, dx);
  if (int e = accept_row(k, dim, "l2_norm")) return e;
  DISPATCH_DTYPE(dtype, NW(k, l2_launch<bf16_t, true>(k, x, dy, dx, rows, dim, eps, st)),
                 NW(k, l2_launch<f16_t, true>(k, x, dy, dx, rows, dim, eps, st)),
                 NW(k, l2_launch<float, true>(k, x, dy, dx, rows, dim, eps, st)));
}

}  // extern "C"
