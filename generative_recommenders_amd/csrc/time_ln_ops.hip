// TimestampLayerNormPostprocessor behind its GEMM (gfx950, HBM-bound): with the combiner weight split as W = [Wx | Wt],
//   z0 = x Wx^T                                        (a GEMM with an aligned contraction length; not in this file)
//   z  = z0 + b + sum_j tf_j(t) Wt[j, :]               (2F time features of the row's timestamp: a rank-2F update)
//   y  = LayerNorm(z) ln_w + ln_b
// in one row pass, and the backward of it.  Replaces the concat to a (D + 2F)-wide row, the Linear(D + 2F, D) and the
// LayerNorm pass of modules/postprocessors.py:105-176 (the postprocessor DlrmHSTU builds, modules/dlrm_hstu.py:182-191).
//
// One wavefront owns one row at a time (grid-stride over rows), lanes own fixed columns.  Lane j < 2F computes feature j of
// the row (fmod, two IEEE divides, one sin or cos per ROW, not per element); the others read it with v_readlane.  Rows of
// one chunk (64 16-byte pieces: 512 bf16, 256 fp32) keep b, Wt, ln_w, ln_b -- and in the backward the per-lane partials of
// the 3 + 2F column sums -- in registers: z0 (and dy) are read once, y (dz) written once.  Wider rows hold the forward's row in
// registers (the narrow / wide instance of norm_dispatch.h) and read the parameters through the cache; their backward runs
// one workgroup column per chunk, each sweeping the whole row for the norm's two row sums (a row is read once per chunk).
// Every sum over rows is a per-lane sum in row order, a fixed-order sum over the workgroup's waves through LDS, one partial
// per workgroup in the workspace and a fixed-order finish kernel: no float atomics, bit-identical run to run.
// Pieces, wave sums and the sum over the waves are row_pass.cuh's; the grid rule and the backward's finish kernel
// (launch_partial_col_sums, aux_ops.hip) are capi_internal.h's.
#include "row_pass.cuh"
#include "capi_internal.h"
#include "norm_dispatch.h"

namespace hstu {
namespace {

constexpr int kTlThreads = 256;
constexpr int kTlWaves = kTlThreads / 64;
constexpr int kTlMaxBlocks = HSTU_TIME_LN_MAX_BLOCKS;
constexpr int kTlMaxFeat = 2 * HSTU_TIME_LN_MAX_PERIODS;

// ------------------------------------------------------------------ time features
// torch.div(a, b, rounding_mode="floor") on fp32 (c10::div_floor_floating): fmod-based, NOT floorf(a / b)
HSTU_DEV float floor_div_f32(float a, float b) {
  if (b == 0.f) return a / b;
  const float mod = fmodf(a, b);
  float div = (a - mod) / b;
  if (mod != 0.f && ((b < 0.f) != (mod < 0.f))) div -= 1.0f;
  if (div == 0.f) return copysignf(0.f, a / b);
  float fl = floorf(div);
  if (div - fl > 0.5f) fl += 1.0f;
  return fl;
}

// torch.remainder on fp32: the sign of the divisor
HSTU_DEV float remainder_f32(float a, float b) {
  float mod = fmodf(a, b);
  if (mod != 0.f && ((b < 0.f) != (mod < 0.f))) mod += b;
  return mod;
}

// feature j of timestamp t: [cos, sin] of period j >> 1, interleaved.  The reference's fp32 arithmetic in its order
// (postprocessors.py:133-165): the constant is 3.14, the timestamp is rounded to fp32 first.
HSTU_DEV float time_feature(int64_t t, const float* period_units, const float* units_per_period, int j) {
  const float period = period_units[j >> 1], upp = units_per_period[j >> 1];
  const float units = floor_div_f32((float)t, period);
  const float angle = ((remainder_f32(units, upp) / upp) * 2.0f) * 3.14f;
  return (j & 1) ? sinf(angle) : cosf(angle);
}

__global__ __launch_bounds__(256) void time_features_kernel(const int64_t* t, const float* period_units,
                                                            const float* units_per_period, int nf, float* out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / nf;
    out[i] = time_feature(t[row], period_units, units_per_period, (int)(i - row * nf));
  }
}

struct TlFwdArgs {
  const void* z0; const int64_t* t; const float* period_units; const float* units_per_period;
  const float* b; const float* wt; const float* ln_w; const float* ln_b; float eps;
  void* y; float* mean; float* rstd;
  int64_t rows; int dim; int nf;
};

struct TlBwdArgs {
  const void* dy; const void* z0; const int64_t* t; const float* period_units; const float* units_per_period;
  const float* b; const float* wt; const float* ln_w; const float* mean; const float* rstd;
  void* dz; float* partial;
  int64_t rows; int dim; int nf;
};

// the row's 2F features in every lane: lane j computes feature j
template <int NF>
HSTU_DEV void row_features(float (&tf)[NF], int64_t t, const float* period_units, const float* units_per_period, int nf, int lane) {
  const float f = lane < nf ? time_feature(t, period_units, units_per_period, lane) : 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) tf[j] = lane_value(f, j);
}

// Wt[j][c .. c + VEC) of every feature (zeros past nf and for a lane past the row)
template <int VEC, int NF>
HSTU_DEV void load_wt(float (&wv)[NF][VEC], const float* wt, int dim, int c, int nf, bool ok) {
#pragma unroll
  for (int j = 0; j < NF; ++j) load_param<VEC>(wv[j], wt + (int64_t)j * dim + c, ok && j < nf);
}

// z = z0 + b + sum_j tf_j Wt[j]
template <int VEC, int NF>
HSTU_DEV void add_update(float (&z)[VEC], const float (&bv)[VEC], const float (&wv)[NF][VEC], const float (&tf)[NF], int nf) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    float u = bv[i];
#pragma unroll
    for (int j = 0; j < NF; ++j)
      if (j < nf) u += tf[j] * wv[j][i];
    z[i] += u;
  }
}

// the same with the parameters read through the cache, one piece at a time (rows of more than one chunk)
template <int VEC, int NF>
HSTU_DEV void add_update_mem(float (&z)[VEC], const float* b, const float* wt, int dim, int c, const float (&tf)[NF], int nf, bool ok) {
  float u[VEC];
  load_param<VEC>(u, b + c, ok);
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    if (j < nf) {
      float wv[VEC];
      load_param<VEC>(wv, wt + (int64_t)j * dim + c, ok);
#pragma unroll
      for (int i = 0; i < VEC; ++i) u[i] += tf[j] * wv[i];
    }
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) z[i] += u[i];
}

// ------------------------------------------------------------------ forward
template <typename T, int VEC, int MC, int NF>
__global__ __launch_bounds__(kTlThreads) void time_ln_fwd_kernel(const TlFwdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dim = a.dim, nf = a.nf;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  const T* z0 = (const T*)a.z0;
  [[maybe_unused]] float br[VEC], wr[MC == 1 ? NF : 1][VEC], gr[VEC], hr[VEC];
  if constexpr (MC == 1) {
    const int c = lane * VEC;
    load_param<VEC>(br, a.b + c, c < dim);
    load_wt<VEC, NF>(wr, a.wt, dim, c, nf, c < dim);
    load_param<VEC>(gr, a.ln_w + c, c < dim);
    load_param<VEC>(hr, a.ln_b + c, c < dim);
  }
  for (int64_t row = (int64_t)blockIdx.x * kTlWaves + wave; row < a.rows; row += (int64_t)gridDim.x * kTlWaves) {
    float tf[NF];
    row_features<NF>(tf, a.t[row], a.period_units, a.units_per_period, nf, lane);
    float zv[MC][VEC];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      const bool ok = k < nch && c < dim;
      load_piece<T, VEC>(zv[k], z0 + row * dim + c, ok);
      if (k < nch) {   // wave-uniform; lanes past dim hold zeros and add zeros
        if constexpr (MC == 1) {
          add_update<VEC, NF>(zv[k], br, wr, tf, nf);
        } else {
          add_update_mem<VEC, NF>(zv[k], a.b, a.wt, dim, c, tf, nf, ok);
        }
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) s += zv[k][i];
    }
    const float mean = wave_sum(s) / dim;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch && c < dim) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { const float d = zv[k][i] - mean; q += d * d; }
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / dim + a.eps);
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch && c < dim) {
        float o[VEC];
        if constexpr (MC == 1) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) o[i] = (zv[k][i] - mean) * rstd * gr[i] + hr[i];
        } else {
          float gv[VEC], hv[VEC];
          load_param<VEC>(gv, a.ln_w + c, true);
          load_param<VEC>(hv, a.ln_b + c, true);
#pragma unroll
          for (int i = 0; i < VEC; ++i) o[i] = (zv[k][i] - mean) * rstd * gv[i] + hv[i];
        }
        store_piece<T, VEC, true>(o, (T*)a.y + row * dim + c);
      }
    }
    if (lane == 0) {
      if (a.mean) a.mean[row] = mean;
      if (a.rstd) a.rstd[row] = rstd;
    }
  }
}

// ------------------------------------------------------------------ backward
// one piece of a row: xhat of the recomputed z and the gradient entering it, dxh = dy ln_w (zeros in a lane past the row)
template <int VEC, int NF>
HSTU_DEV void piece_terms(float (&z)[VEC], const float (&dyv)[VEC], const float (&bv)[VEC], const float (&wv)[NF][VEC],
                          const float (&gv)[VEC], const float (&tf)[NF], int nf, float mean, float rstd, bool ok,
                          float (&xhat)[VEC], float (&dxh)[VEC]) {
  add_update<VEC, NF>(z, bv, wv, tf, nf);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    xhat[i] = ok ? (z[i] - mean) * rstd : 0.f;
    dxh[i] = dyv[i] * gv[i];
  }
}

// Workgroup (bx, by): chunk by (columns [by 64 VEC, +64 VEC)) of the rows bx, bx + gridDim.x, ...  Its lanes keep that
// chunk's parameters and the per-lane partials of the 3 + 2F column sums in registers; the other chunks of a row are swept
// only for the two row sums of the norm's backward.
// partial row of a workgroup row bx: [d ln_w (dim) | d ln_b (dim) | d b (dim) | d Wt (nf, dim)]
template <typename T, int VEC, int NF>
__global__ __launch_bounds__(kTlThreads) void time_ln_bwd_kernel(const TlBwdArgs a) {
  __shared__ float lds[kTlWaves * 64 * VEC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dim = a.dim, nf = a.nf;
  const int nch = (int)gridDim.y, own = (int)blockIdx.y;
  const int c0 = own * 64 * VEC;
  const int c = c0 + lane * VEC;
  const bool ok = c < dim;
  const T* dy = (const T*)a.dy;
  const T* z0 = (const T*)a.z0;
  float br[VEC], wr[NF][VEC], gr[VEC], dg[VEC], dh[VEC], db[VEC], dw[NF][VEC];
  load_param<VEC>(br, a.b + c, ok);
  load_wt<VEC, NF>(wr, a.wt, dim, c, nf, ok);
  load_param<VEC>(gr, a.ln_w + c, ok);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    dg[i] = 0.f;
    dh[i] = 0.f;
    db[i] = 0.f;
#pragma unroll
    for (int j = 0; j < NF; ++j) dw[j][i] = 0.f;
  }
  for (int64_t row = (int64_t)blockIdx.x * kTlWaves + wave; row < a.rows; row += (int64_t)gridDim.x * kTlWaves) {
    float tf[NF];
    row_features<NF>(tf, a.t[row], a.period_units, a.units_per_period, nf, lane);
    const float mean = a.mean[row], rstd = a.rstd[row];
    float zv[VEC], dyv[VEC], xhat[VEC], dxh[VEC];
    load_piece<T, VEC>(zv, z0 + row * dim + c, ok);
    load_piece<T, VEC>(dyv, dy + row * dim + c, ok);
    piece_terms<VEC, NF>(zv, dyv, br, wr, gr, tf, nf, mean, rstd, ok, xhat, dxh);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) { s1 += dxh[i] * xhat[i]; s2 += dxh[i]; }
    for (int k = 0; k < nch; ++k) {
      if (k == own) continue;   // wave-uniform
      const int ck = (k * 64 + lane) * VEC;
      const bool okk = ck < dim;
      float z2[VEC], dy2[VEC], g2[VEC];
      load_piece<T, VEC>(z2, z0 + row * dim + ck, okk);
      load_piece<T, VEC>(dy2, dy + row * dim + ck, okk);
      load_param<VEC>(g2, a.ln_w + ck, okk);
      add_update_mem<VEC, NF>(z2, a.b, a.wt, dim, ck, tf, nf, okk);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float g = dy2[i] * g2[i];   // zero in a lane past the row
        s1 += g * (z2[i] - mean) * rstd;
        s2 += g;
      }
    }
    const float c1 = wave_sum(s1) / dim, c2 = wave_sum(s2) / dim;
    if (ok) {
      float o[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        o[i] = rstd * (dxh[i] - c2 - xhat[i] * c1);
        dg[i] += dyv[i] * xhat[i];
        dh[i] += dyv[i];
        db[i] += o[i];
#pragma unroll
        for (int j = 0; j < NF; ++j)
          if (j < nf) dw[j][i] += tf[j] * o[i];
      }
      store_piece<T, VEC, true>(o, (T*)a.dz + row * dim + c);
    }
  }
  float* prow = a.partial + (int64_t)blockIdx.x * (3 + nf) * dim;
  block_sum_cols<VEC, kTlWaves>(dg, lds, prow, c0, dim);
  block_sum_cols<VEC, kTlWaves>(dh, lds, prow + dim, c0, dim);
  block_sum_cols<VEC, kTlWaves>(db, lds, prow + 2 * (int64_t)dim, c0, dim);
#pragma unroll
  for (int j = 0; j < NF; ++j)
    if (j < nf) block_sum_cols<VEC, kTlWaves>(dw[j], lds, prow + (int64_t)(3 + j) * dim, c0, dim);
}

// ------------------------------------------------------------------ host side
// (grids: the resident one, at most kTlMaxBlocks; the backward's is divided among its workgroup columns)
template <typename T, int VEC, int MC, int NF>
static int fwd_go(const TlFwdArgs& a, hipStream_t st) {
  auto kernel = time_ln_fwd_kernel<T, VEC, MC, NF>;
  hipLaunchKernelGGL(kernel, dim3(resident_row_blocks(kernel, kTlThreads, 0, a.rows, kTlWaves, kTlMaxBlocks)), dim3(kTlThreads), 0, st, a);
  return check_launch("hstu_time_ln_fwd");
}

// one chunk: parameters in registers (4 features: the DLRM pair of periods; else 8); narrow / wide: the row in registers
template <typename T>
static int fwd_pick(const TlFwdArgs& a, const norm_dispatch::RowClass& k, hipStream_t st) {
  constexpr int VV = 16 / (int)sizeof(T);
  if (k.one_chunk) return a.nf <= 4 ? fwd_go<T, VV, 1, 4>(a, st) : fwd_go<T, VV, 1, kTlMaxFeat>(a, st);
  if (k.vec > 1) {
    return k.wide ? fwd_go<T, VV, norm_dispatch::pieces_per_lane(VV, true), kTlMaxFeat>(a, st)
                  : fwd_go<T, VV, norm_dispatch::pieces_per_lane(VV, false), kTlMaxFeat>(a, st);
  }
  return k.wide ? fwd_go<T, 1, norm_dispatch::pieces_per_lane(1, true), kTlMaxFeat>(a, st)
                : fwd_go<T, 1, norm_dispatch::pieces_per_lane(1, false), kTlMaxFeat>(a, st);
}

template <typename T, int VEC, int NF>
static int bwd_go(const TlBwdArgs& a, float* dln_w, float* dln_b, float* db, float* dwt, hipStream_t st) {
  const char* who = "hstu_time_ln_bwd";
  auto kernel = time_ln_bwd_kernel<T, VEC, NF>;
  const int nch = (a.dim + 64 * VEC - 1) / (64 * VEC);
  const int nb = resident_row_blocks(kernel, kTlThreads, 0, a.rows, kTlWaves, kTlMaxBlocks, nch);
  hipLaunchKernelGGL(kernel, dim3(nb, nch), dim3(kTlThreads), 0, st, a);
  if (int e = check_launch(who)) return e;
  const int64_t pstride = (int64_t)(3 + a.nf) * a.dim;
  return launch_partial_col_sums(a.partial, nb, pstride, {{dln_w, a.dim}, {dln_b, a.dim}, {db, a.dim}, {dwt, (int64_t)a.nf * a.dim}}, who, st);
}

// the backward's lanes hold one chunk whatever the row's width: only the piece width of the class picks its instance
template <typename T>
static int bwd_pick(const TlBwdArgs& a, const norm_dispatch::RowClass& k, float* dln_w, float* dln_b, float* db, float* dwt,
                    hipStream_t st) {
  constexpr int VV = 16 / (int)sizeof(T);
  if (k.vec > 1) return a.nf <= 4 ? bwd_go<T, VV, 4>(a, dln_w, dln_b, db, dwt, st) : bwd_go<T, VV, kTlMaxFeat>(a, dln_w, dln_b, db, dwt, st);
  return a.nf <= 4 ? bwd_go<T, 1, 4>(a, dln_w, dln_b, db, dwt, st) : bwd_go<T, 1, kTlMaxFeat>(a, dln_w, dln_b, db, dwt, st);
}

// max_periods: what the row pass holds in registers (HSTU_TIME_LN_MAX_PERIODS); the feature kernel alone takes any number
static int check_common(const char* who, int num_periods, int max_periods, int dim, int64_t rows, int dtype) {
  if (!is_float_dtype(dtype)) return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32 (got code %d)", who, dtype);
  if (num_periods < 1 || num_periods > max_periods)
    return set_error(HSTU_EINVAL, "%s: num_periods must be in [1, %d] (got %d)", who, max_periods, num_periods);
  if (rows < 0) return set_error(HSTU_EINVAL, "%s: negative rows", who);
  if (dim <= 0) return set_error(HSTU_EINVAL, "%s: dim must be positive (got %d)", who, dim);
  return HSTU_OK;
}

static int accept_class(const char* who, const norm_dispatch::RowClass& k, int dim) {
  if (norm_dispatch::refused(k, dim))
    return set_error(HSTU_EUNSUPPORTED, "%s: dim %d exceeds the %d supported with this alignment", who, dim, k.limit);
  return HSTU_OK;
}

}  // namespace
}  // namespace hstu

using namespace hstu;

extern "C" {

int hstu_time_features(const int64_t* timestamps, const float* period_units, const float* units_per_period, int32_t num_periods,
                       float* out, int64_t rows, void* stream) {
  const char* who = "hstu_time_features";
  if (int e = check_common(who, num_periods, HSTU_TIME_FEATURES_MAX_PERIODS, 1, rows, HSTU_DTYPE_F32)) return e;
  if (!period_units || !units_per_period) return set_error(HSTU_EINVAL, "%s: period_units and units_per_period must be non-NULL", who);
  if (rows == 0) return HSTU_OK;
  if (!timestamps || !out) return set_error(HSTU_EINVAL, "%s: timestamps and out must be non-NULL", who);
  if (((uintptr_t)timestamps & 7) || (((uintptr_t)out | (uintptr_t)period_units | (uintptr_t)units_per_period) & 3))
    return set_error(HSTU_EINVAL, "%s: a tensor is not aligned to its element size", who);
  const int64_t n = rows * 2 * num_periods;
  int64_t blocks = (n + 255) / 256;
  if (blocks > (int64_t)cu_count() * 8) blocks = (int64_t)cu_count() * 8;
  hipLaunchKernelGGL(time_features_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, timestamps, period_units,
                     units_per_period, 2 * num_periods, out, n);
  return check_launch(who);
}

size_t hstu_time_ln_workspace_bytes(int32_t dim, int32_t num_periods) {
  if (dim < 1 || num_periods < 1 || num_periods > HSTU_TIME_LN_MAX_PERIODS) return 0;
  return (size_t)kTlMaxBlocks * (size_t)(3 + 2 * num_periods) * (size_t)dim * sizeof(float);
}

int hstu_time_ln_fwd(const void* z0, const int64_t* timestamps, const float* period_units, const float* units_per_period,
                     int32_t num_periods, const float* b, const float* wt, const float* ln_weight, const float* ln_bias, float eps,
                     void* y, float* mean, float* rstd, int64_t rows, int32_t dim, int dtype, void* stream) {
  const char* who = "hstu_time_ln_fwd";
  if (int e = check_common(who, num_periods, HSTU_TIME_LN_MAX_PERIODS, dim, rows, dtype)) return e;
  if (!period_units || !units_per_period || !b || !wt || !ln_weight || !ln_bias)
    return set_error(HSTU_EINVAL, "%s: the periods, b, wt, ln_weight and ln_bias must be non-NULL", who);
  const int eb = dtype_bytes(dtype);
  if ((((uintptr_t)z0 | (uintptr_t)y) & (eb - 1)) || ((uintptr_t)timestamps & 7) ||
      (((uintptr_t)period_units | (uintptr_t)units_per_period | (uintptr_t)b | (uintptr_t)wt | (uintptr_t)ln_weight |
        (uintptr_t)ln_bias | (uintptr_t)mean | (uintptr_t)rstd) & 3))
    return set_error(HSTU_EINVAL, "%s: a tensor is not aligned to its element size", who);
  const norm_dispatch::RowClass k = norm_dispatch::time_ln_fwd_class(dim, eb, z0, b, wt, ln_weight, ln_bias, y);
  if (int e = accept_class(who, k, dim)) return e;
  if (rows == 0) return HSTU_OK;
  if (!z0 || !timestamps || !y) return set_error(HSTU_EINVAL, "%s: z0, timestamps and y must be non-NULL", who);
  const TlFwdArgs a{z0, timestamps, period_units, units_per_period, b, wt, ln_weight, ln_bias, eps, y, mean, rstd, rows, dim,
                    2 * num_periods};
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case HSTU_DTYPE_BF16: return fwd_pick<bf16_t>(a, k, st);
    case HSTU_DTYPE_F16: return fwd_pick<f16_t>(a, k, st);
    default: return fwd_pick<float>(a, k, st);
  }
}

int hstu_time_ln_bwd(const void* dy, const void* z0, const int64_t* timestamps, const float* period_units,
                     const float* units_per_period, int32_t num_periods, const float* b, const float* wt, const float* ln_weight,
                     const float* mean, const float* rstd, void* dz, float* dln_weight, float* dln_bias, float* db, float* dwt,
                     void* workspace, int64_t rows, int32_t dim, int dtype, void* stream) {
  const char* who = "hstu_time_ln_bwd";
  if (int e = check_common(who, num_periods, HSTU_TIME_LN_MAX_PERIODS, dim, rows, dtype)) return e;
  if (!period_units || !units_per_period || !b || !wt || !ln_weight)
    return set_error(HSTU_EINVAL, "%s: the periods, b, wt and ln_weight must be non-NULL", who);
  if (!dln_weight || !dln_bias || !db || !dwt) return set_error(HSTU_EINVAL, "%s: dln_weight, dln_bias, db and dwt are required", who);
  const int eb = dtype_bytes(dtype);
  if ((((uintptr_t)dy | (uintptr_t)z0 | (uintptr_t)dz) & (eb - 1)) || ((uintptr_t)timestamps & 7) || ((uintptr_t)workspace & 15) ||
      (((uintptr_t)period_units | (uintptr_t)units_per_period | (uintptr_t)b | (uintptr_t)wt | (uintptr_t)ln_weight |
        (uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)dln_weight | (uintptr_t)dln_bias | (uintptr_t)db | (uintptr_t)dwt) & 3))
    return set_error(HSTU_EINVAL, "%s: a tensor is not aligned to its element size (the workspace: 16 bytes)", who);
  const norm_dispatch::RowClass k = norm_dispatch::time_ln_bwd_class(dim, eb, dy, z0, b, wt, ln_weight, dz);
  if (int e = accept_class(who, k, dim)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0) {
    (void)hipMemsetAsync(dln_weight, 0, dim * sizeof(float), st);
    (void)hipMemsetAsync(dln_bias, 0, dim * sizeof(float), st);
    (void)hipMemsetAsync(db, 0, dim * sizeof(float), st);
    (void)hipMemsetAsync(dwt, 0, (size_t)2 * num_periods * dim * sizeof(float), st);
    return HSTU_OK;
  }
  if (!dy || !z0 || !timestamps || !mean || !rstd || !dz || !workspace)
    return set_error(HSTU_EINVAL, "%s: dy, z0, timestamps, mean, rstd, dz and the workspace must be non-NULL", who);
  const TlBwdArgs a{dy, z0, timestamps, period_units, units_per_period, b, wt, ln_weight, mean, rstd, dz, (float*)workspace,
                    rows, dim, 2 * num_periods};
  switch (dtype) {
    case HSTU_DTYPE_BF16: return bwd_pick<bf16_t>(a, k, dln_weight, dln_bias, db, dwt, st);
    case HSTU_DTYPE_F16: return bwd_pick<f16_t>(a, k, dln_weight, dln_bias, db, dwt, st);
    default: return bwd_pick<float>(a, k, dln_weight, dln_bias, db, dwt, st);
  }
}

}  // extern "C"
