// Multitask prediction head behind the first projection (gfx950, HBM-bound): per row of x (rows, dim)
//   y = x * sigmoid(LayerNorm(x) g + b)            (SwishLayerNorm, never written to memory)
//   logit[t] = <y, W[t]> + c[t],  pred[t] = sigmoid(logit[t]) for the binary tasks, logit[t] for the regression tasks
//   loss[t] = sum_rows weight * (BCE-with-logits | squared error) / max(sum_rows weight, 1) * loss_scale
// and the backward of all of it.  Replaces the tail of DefaultMultitaskModule (modules/multitask_module.py:70-104 predictions,
// :136-191 losses; the prediction module of modules/dlrm_hstu.py:139-149): SwishLayerNorm + Linear(hidden, T) + the (T, L) torch ops.
//
// One wavefront owns one row at a time (grid-stride over rows), lanes own fixed columns.  Rows of up to 64 16-byte pieces (512
// bf16) keep W, g, b -- and in the backward the per-lane partials of dW, dg, db -- in registers: x is read once, dx written
// once.  Wider rows hold W in LDS; their backward runs as two kernels (dx over whole rows; dW / dg / db per group of 64 pieces,
// which reads x a second time) so that no instance needs more than 64 accumulators per array.  The T values of a row live in
// lanes 0 .. T-1.  Every sum over rows is a per-lane sum in row order, a fixed-order sum over the workgroup's waves through LDS,
// one partial per workgroup in the workspace and a fixed-order finish kernel: no float atomics, bit-identical run to run.
// Pieces, wave sums and the sum over the waves are row_pass.cuh's; the grid rule and the backward's finish kernel
// (launch_partial_col_sums, aux_ops.hip) are capi_internal.h's.
#include "row_pass.cuh"
#include "capi_internal.h"

namespace hstu {
namespace {

constexpr int kMtThreads = 256;
constexpr int kMtWaves = HSTU_MULTITASK_ROWS_PER_BLOCK;
constexpr int kMtMaxBlocks = HSTU_MULTITASK_MAX_BLOCKS;
constexpr int kMtMaxTasks = HSTU_MULTITASK_MAX_TASKS;
constexpr int kMtLossCols = 2 * kMtMaxTasks;   // forward partial of a workgroup: [loss sums (8) | weight sums (8)]
static_assert(kMtThreads == 64 * kMtWaves, "one wave per row");

struct MtFwdArgs {
  const void* x; int64_t x_rs;
  const void* g; const void* b; float eps;
  const float* w; const float* c;
  const float* labels; const float* weights;
  float* logits; float* preds; float* mean; float* rstd;
  float* partial;
  int64_t rows; int dim; int tasks; int nbin;
};

struct MtBwdArgs {
  const float* grad_loss; const float* grad_pred;
  const void* x; int64_t x_rs;
  const void* g; const void* b;
  const float* w; const float* labels; const float* weights; const float* logits;
  const float* mean; const float* rstd; const float* wsum;
  void* dx; int64_t dx_rs;
  float* partial;
  int64_t rows; int dim; int tasks; int nbin; float loss_scale;
};

// the T values of a row are computed once, in lanes 0 .. T-1: IEEE exp / log1p / divide there (T <= 8 per row), the hardware
// exp2 / rcp only for the row's dim sigmoids of the gate
HSTU_DEV float precise_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// W[t][c .. c + VEC) of every task: from global memory (narrow rows: once per wave) or from the workgroup's LDS copy
template <int VEC, int NT>
HSTU_DEV void load_w(float (&wv)[NT][VEC], const float* w, int row_stride, int c, int tasks, bool ok) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < VEC; ++i) wv[t][i] = (ok && t < tasks) ? w[(int64_t)t * row_stride + c + i] : 0.f;
}

// the workgroup's copy of W in LDS: [tasks][dpad], zeros past dim
HSTU_DEV void stage_w(float* lds, const float* w, int tasks, int dim, int dpad) {
  for (int i = threadIdx.x; i < tasks * dpad; i += kMtThreads) {
    const int t = i / dpad, c = i - t * dpad;
    lds[i] = c < dim ? w[(int64_t)t * dim + c] : 0.f;
  }
  __syncthreads();
}

// ------------------------------------------------------------------ forward
template <typename T, int VEC, int MC, int NT>
__global__ __launch_bounds__(kMtThreads) void multitask_head_fwd_kernel(const MtFwdArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dim = a.dim, tasks = a.tasks;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  const int dpad = nch * 64 * VEC;
  const T* x = (const T*)a.x;
  const T* g = (const T*)a.g;
  const T* b = (const T*)a.b;
  [[maybe_unused]] float wr[MC == 1 ? NT : 1][VEC], gr[VEC], br[VEC];
  if constexpr (MC == 1) {
    const int c = lane * VEC;
    load_w<VEC, NT>(wr, a.w, dim, c, tasks, c < dim);
    load_piece<T, VEC>(gr, g + c, c < dim);
    load_piece<T, VEC>(br, b + c, c < dim);
  } else {
    stage_w(lds, a.w, tasks, dim, dpad);
  }
  const float cb = lane < tasks ? a.c[lane] : 0.f;
  float lacc = 0.f, wacc = 0.f;   // lane t: this wave's sums of weighted loss and of weight for task t
  for (int64_t row = (int64_t)blockIdx.x * kMtWaves + wave; row < a.rows; row += (int64_t)gridDim.x * kMtWaves) {
    float xv[MC][VEC];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      load_piece<T, VEC>(xv[k], x + row * a.x_rs + c, k < nch && c < dim);
#pragma unroll
      for (int i = 0; i < VEC; ++i) s += xv[k][i];
    }
    const float mean = wave_sum(s) / dim;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch && c < dim) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { const float d = xv[k][i] - mean; q += d * d; }
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / dim + a.eps);
    float part[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) part[t] = 0.f;
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      if (k < nch) {   // wave-uniform; lanes past dim hold zeros and add zeros
        const bool ok = c < dim;
        float y[VEC];
        if constexpr (MC == 1) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) y[i] = xv[k][i] * fast_sigmoid((xv[k][i] - mean) * rstd * gr[i] + br[i]);
        } else {
          float gv[VEC], bv[VEC];
          load_piece<T, VEC>(gv, g + c, ok);
          load_piece<T, VEC>(bv, b + c, ok);
#pragma unroll
          for (int i = 0; i < VEC; ++i) y[i] = xv[k][i] * fast_sigmoid((xv[k][i] - mean) * rstd * gv[i] + bv[i]);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (t < tasks) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              if constexpr (MC == 1) part[t] += y[i] * wr[t][i];
              else part[t] += y[i] * lds[t * dpad + c + i];
            }
          }
        }
      }
    }
    float z = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < tasks) {
        const float p = wave_sum(part[t]);
        if (lane == t) z = p;
      }
    }
    z += cb;
    if (lane < tasks) {
      const int64_t o = (int64_t)lane * a.rows + row;
      const bool binary = lane < a.nbin;
      if (a.logits) a.logits[o] = z;
      a.preds[o] = binary ? precise_sigmoid(z) : z;
      if (a.labels) {
        const float lab = a.labels[o];
        const float wt = a.weights ? a.weights[o] : 1.0f;
        const float d = z - lab;
        const float l = binary ? fmaxf(z, 0.f) - z * lab + log1pf(expf(-fabsf(z))) : d * d;
        lacc += l * wt;
        wacc += wt;
      }
    }
    if (lane == 0) {
      if (a.mean) a.mean[row] = mean;
      if (a.rstd) a.rstd[row] = rstd;
    }
  }
  if (a.labels) {   // kernel-uniform
    __syncthreads();   // every wave is done with the LDS copy of W
    if (lane < kMtMaxTasks) {
      lds[wave * kMtLossCols + lane] = lacc;
      lds[wave * kMtLossCols + kMtMaxTasks + lane] = wacc;
    }
    __syncthreads();
    if (threadIdx.x < kMtLossCols) {
      float s = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < kMtWaves; ++w2) s += lds[w2 * kMtLossCols + threadIdx.x];
      a.partial[(int64_t)blockIdx.x * kMtLossCols + threadIdx.x] = s;
    }
  }
}

// loss[t] = (sum of the workgroups' loss partials) / max(sum of their weight partials, 1) * loss_scale; one block per task,
// thread i adds partials i, i + 256, .. in order, then a fixed tree
__global__ __launch_bounds__(256) void multitask_head_loss_finish_kernel(const float* partial, int nparts, float loss_scale,
                                                                         float* loss, float* weight_sum) {
  __shared__ float red[2][256];
  const int t = blockIdx.x;
  float sl = 0.f, sw = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) {
    sl += partial[(int64_t)i * kMtLossCols + t];
    sw += partial[(int64_t)i * kMtLossCols + kMtMaxTasks + t];
  }
  red[0][threadIdx.x] = sl;
  red[1][threadIdx.x] = sw;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      red[0][threadIdx.x] += red[0][threadIdx.x + k];
      red[1][threadIdx.x] += red[1][threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    weight_sum[t] = red[1][0];
    loss[t] = red[0][0] / fmaxf(red[1][0], 1.0f) * loss_scale;
  }
}

// ------------------------------------------------------------------ backward
// lane t: d logit[t, row] = grad_loss[t] loss_scale weight / max(sum weight, 1) * d l/d z + grad_pred[t, row] * d pred/d z
// (`coef` = the row-independent factor of the first term, 0 without a loss gradient); returned per task in every lane
template <int NT>
HSTU_DEV float row_dlogit(const MtBwdArgs& a, int64_t row, int lane, float coef, float (&dlt)[NT]) {
  float dl = 0.f;
  if (lane < a.tasks) {
    const int64_t o = (int64_t)lane * a.rows + row;
    const bool binary = lane < a.nbin;
    const float z = a.logits[o];
    const float p = precise_sigmoid(z);
    if (a.grad_loss && a.labels) {
      const float lab = a.labels[o];
      const float wt = a.weights ? a.weights[o] : 1.0f;
      dl = coef * wt * (binary ? p - lab : 2.0f * (z - lab));
    }
    if (a.grad_pred) dl += a.grad_pred[o] * (binary ? p * (1.0f - p) : 1.0f);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) dlt[t] = lane_value(dl, t);
  return dl;
}

HSTU_DEV float loss_coef(const MtBwdArgs& a, int lane) {
  return (lane < a.tasks && a.grad_loss && a.labels) ? a.grad_loss[lane] * a.loss_scale / fmaxf(a.wsum[lane], 1.0f) : 0.f;
}

// one piece of a row: with s = sigmoid(z), z = xhat g + b and dy = sum_t dlogit[t] W[t], the gradient entering the norm is
// dz = dy x s (1 - s) and dy s reaches x directly (as in the SwishLayerNorm backward); y = x s is recomputed for dW
template <int VEC, int NT>
HSTU_DEV void piece_backward(const float (&xv)[VEC], const float (&gv)[VEC], const float (&bv)[VEC], const float (&wv)[NT][VEC],
                             const float (&dlt)[NT], int tasks, float mean, float rstd, bool ok, float (&xhat)[VEC],
                             float (&y)[VEC], float (&direct)[VEC], float (&dz)[VEC]) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    xhat[i] = ok ? (xv[i] - mean) * rstd : 0.f;
    const float sg = fast_sigmoid(xhat[i] * gv[i] + bv[i]);
    y[i] = xv[i] * sg;
    float dy = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < tasks) dy += dlt[t] * wv[t][i];
    direct[i] = dy * sg;
    dz[i] = direct[i] * xv[i] * (1.0f - sg);
  }
}

// Columns [blockIdx.y 64 VEC, +64 VEC) of every row: per-lane partials of dW, dg, db (and dc in column group 0) in
// registers.  DX (rows of one column group, gridDim.y == 1): the row sums of the norm's backward are complete inside the
// wave, so dx is written here too and x is read exactly once.
// partial row of a workgroup: [dW (tasks, dim) | dg (dim) | db (dim) | dc (8)]
// (two waves per SIMD asked for: at eight tasks the whole-row instance otherwise settles one register above the 256 of a second wave)
template <typename T, int VEC, int NT, bool DX>
__global__ __launch_bounds__(kMtThreads, 2) void multitask_head_bwd_kernel(const MtBwdArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dim = a.dim, tasks = a.tasks;
  const int c0 = blockIdx.y * 64 * VEC;
  const int c = c0 + lane * VEC;
  const bool ok = c < dim;
  const T* x = (const T*)a.x;
  float wr[NT][VEC], gr[VEC], br[VEC], dw[NT][VEC], dg[VEC], db[VEC];
  load_w<VEC, NT>(wr, a.w, dim, c, tasks, ok);
  load_piece<T, VEC>(gr, (const T*)a.g + c, ok);
  load_piece<T, VEC>(br, (const T*)a.b + c, ok);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    dg[i] = 0.f;
    db[i] = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) dw[t][i] = 0.f;
  }
  const float coef = loss_coef(a, lane);
  float dcacc = 0.f;   // lane t: sum over this wave's rows of d logit[t]
  for (int64_t row = (int64_t)blockIdx.x * kMtWaves + wave; row < a.rows; row += (int64_t)gridDim.x * kMtWaves) {
    float xv[VEC], dlt[NT];
    load_piece<T, VEC>(xv, x + row * a.x_rs + c, ok);
    const float mean = a.mean[row], rstd = a.rstd[row];
    dcacc += row_dlogit<NT>(a, row, lane, coef, dlt);
    float xhat[VEC], y[VEC], direct[VEC], dz[VEC];
    piece_backward<VEC, NT>(xv, gr, br, wr, dlt, tasks, mean, rstd, ok, xhat, y, direct, dz);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t < tasks) dw[t][i] += dlt[t] * y[i];
      dg[i] += dz[i] * xhat[i];
      db[i] += dz[i];
      if constexpr (DX) {
        dz[i] *= gr[i];          // the gradient entering xhat
        s1 += dz[i] * xhat[i];
        s2 += dz[i];
      }
    }
    if constexpr (DX) {
      const float c1 = wave_sum(s1) / dim, c2 = wave_sum(s2) / dim;
      if (ok) {
        float o[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) o[i] = rstd * (dz[i] - c2 - xhat[i] * c1) + direct[i];
        store_piece<T, VEC, true>(o, (T*)a.dx + row * a.dx_rs + c);
      }
    }
  }
  const int64_t pstride = (int64_t)(tasks + 2) * dim + kMtMaxTasks;
  float* prow = a.partial + (int64_t)blockIdx.x * pstride;
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < tasks) block_sum_cols<VEC, kMtWaves>(dw[t], lds, prow + (int64_t)t * dim, c0, dim);
  block_sum_cols<VEC, kMtWaves>(dg, lds, prow + (int64_t)tasks * dim, c0, dim);
  block_sum_cols<VEC, kMtWaves>(db, lds, prow + (int64_t)(tasks + 1) * dim, c0, dim);
  if (blockIdx.y == 0) {
    if (lane < kMtMaxTasks) lds[wave * kMtMaxTasks + lane] = dcacc;
    __syncthreads();
    if (threadIdx.x < kMtMaxTasks) {
      float s = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < kMtWaves; ++w2) s += lds[w2 * kMtMaxTasks + threadIdx.x];
      prow[(int64_t)(tasks + 2) * dim + threadIdx.x] = s;
    }
  }
}

// dx of rows wider than one column group: the whole row in registers, W in LDS.  The row is swept twice (the row sums of
// the norm's backward, then dx) and the per-piece terms are recomputed in the second sweep instead of held.
template <typename T, int VEC, int MC, int NT>
__global__ __launch_bounds__(kMtThreads) void multitask_head_bwd_dx_kernel(const MtBwdArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dim = a.dim, tasks = a.tasks;
  const int nch = (dim + 64 * VEC - 1) / (64 * VEC);
  const int dpad = nch * 64 * VEC;
  const T* x = (const T*)a.x;
  const T* g = (const T*)a.g;
  const T* b = (const T*)a.b;
  stage_w(lds, a.w, tasks, dim, dpad);
  const float coef = loss_coef(a, lane);
  for (int64_t row = (int64_t)blockIdx.x * kMtWaves + wave; row < a.rows; row += (int64_t)gridDim.x * kMtWaves) {
    float xv[MC][VEC], dlt[NT];
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int c = (k * 64 + lane) * VEC;
      load_piece<T, VEC>(xv[k], x + row * a.x_rs + c, k < nch && c < dim);
    }
    const float mean = a.mean[row], rstd = a.rstd[row];
    (void)row_dlogit<NT>(a, row, lane, coef, dlt);
    float s1 = 0.f, s2 = 0.f, c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int sweep = 0; sweep < 2; ++sweep) {
#pragma unroll
      for (int k = 0; k < MC; ++k) {
        const int c = (k * 64 + lane) * VEC;
        if (k < nch) {   // wave-uniform
          const bool ok = c < dim;
          float gv[VEC], bv[VEC], wv[NT][VEC], xhat[VEC], y[VEC], direct[VEC], dz[VEC];
          load_piece<T, VEC>(gv, g + c, ok);
          load_piece<T, VEC>(bv, b + c, ok);
          load_w<VEC, NT>(wv, lds, dpad, c, tasks, true);
          piece_backward<VEC, NT>(xv[k], gv, bv, wv, dlt, tasks, mean, rstd, ok, xhat, y, direct, dz);
          if (sweep == 0) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) { s1 += dz[i] * gv[i] * xhat[i]; s2 += dz[i] * gv[i]; }
          } else if (ok) {
            float o[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) o[i] = rstd * (dz[i] * gv[i] - c2 - xhat[i] * c1) + direct[i];
            store_piece<T, VEC, true>(o, (T*)a.dx + row * a.dx_rs + c);
          }
        }
      }
      if (sweep == 0) { c1 = wave_sum(s1) / dim; c2 = wave_sum(s2) / dim; }
    }
  }
}

// ------------------------------------------------------------------ host side
// the kernel's LDS reserved, and its resident grid (at most kMtMaxBlocks)
template <typename K>
static int mt_launch_blocks(K kernel, size_t lds, int64_t rows, const char* who, int* nb) {
  if (int e = reserve_lds((const void*)kernel, (int)lds, who)) return e;
  *nb = resident_row_blocks(kernel, kMtThreads, lds, rows, kMtWaves, kMtMaxBlocks);
  return HSTU_OK;
}

template <typename T, int VEC, int MC, int NT>
static int fwd_go(MtFwdArgs a, float loss_scale, float* loss, float* weight_sum, hipStream_t st) {
  const char* who = "hstu_multitask_head_fwd";
  const int nch = (a.dim + 64 * VEC - 1) / (64 * VEC);
  size_t lds = (size_t)kMtWaves * kMtLossCols * sizeof(float);
  if (MC > 1 && (size_t)a.tasks * nch * 64 * VEC * sizeof(float) > lds) lds = (size_t)a.tasks * nch * 64 * VEC * sizeof(float);
  auto kernel = multitask_head_fwd_kernel<T, VEC, MC, NT>;
  int nb = 0;
  if (int e = mt_launch_blocks(kernel, lds, a.rows, who, &nb)) return e;
  hipLaunchKernelGGL(kernel, dim3(nb), dim3(kMtThreads), lds, st, a);
  if (int e = check_launch(who)) return e;
  if (!a.labels) return HSTU_OK;
  hipLaunchKernelGGL(multitask_head_loss_finish_kernel, dim3(a.tasks), dim3(256), 0, st, a.partial, nb, loss_scale, loss, weight_sum);
  return check_launch(who);
}

template <typename T, int VEC, int MC, int NT>
static int bwd_go(MtBwdArgs a, float* dw, float* dc, float* dg, float* db, hipStream_t st) {
  const char* who = "hstu_multitask_head_bwd";
  const int nch = (a.dim + 64 * VEC - 1) / (64 * VEC);
  const size_t lds_acc = (size_t)kMtWaves * 64 * VEC * sizeof(float);
  int nb = 0;
  if constexpr (MC == 1) {
    auto kernel = multitask_head_bwd_kernel<T, VEC, NT, true>;
    if (int e = mt_launch_blocks(kernel, lds_acc, a.rows, who, &nb)) return e;
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(kMtThreads), lds_acc, st, a);
  } else {
    auto dx_kernel = multitask_head_bwd_dx_kernel<T, VEC, MC, NT>;
    const size_t lds_w = (size_t)a.tasks * nch * 64 * VEC * sizeof(float);
    int nb_dx = 0;
    if (int e = mt_launch_blocks(dx_kernel, lds_w, a.rows, who, &nb_dx)) return e;
    hipLaunchKernelGGL(dx_kernel, dim3(nb_dx), dim3(kMtThreads), lds_w, st, a);
    if (int e = check_launch(who)) return e;
    auto kernel = multitask_head_bwd_kernel<T, VEC, NT, false>;
    if (int e = mt_launch_blocks(kernel, lds_acc, a.rows, who, &nb)) return e;
    hipLaunchKernelGGL(kernel, dim3(nb, nch), dim3(kMtThreads), lds_acc, st, a);
  }
  if (int e = check_launch(who)) return e;
  const int64_t pstride = (int64_t)(a.tasks + 2) * a.dim + kMtMaxTasks;
  return launch_partial_col_sums(a.partial, nb, pstride, {{dw, (int64_t)a.tasks * a.dim}, {dg, a.dim}, {db, a.dim}, {dc, a.tasks}}, who, st);
}

// rows of 16-byte pieces (vec) or of single elements; one column group or the widest row; one task or up to eight
#define MT_PICK(GO, T, ...)                                                                                                   \
  do {                                                                                                                        \
    constexpr int VV = sizeof(T) == 2 ? 8 : 4;                                                                                \
    constexpr int WIDE_V = kMultitaskMaxDimVec / (64 * VV), WIDE_1 = kMultitaskMaxDimScalar / 64;                            \
    const bool one = a.tasks == 1;                                                                                            \
    if (vec && a.dim <= 64 * VV) return one ? GO<T, VV, 1, 1>(__VA_ARGS__) : GO<T, VV, 1, kMtMaxTasks>(__VA_ARGS__);          \
    if (vec) return one ? GO<T, VV, WIDE_V, 1>(__VA_ARGS__) : GO<T, VV, WIDE_V, kMtMaxTasks>(__VA_ARGS__);                    \
    if (a.dim <= 64) return one ? GO<T, 1, 1, 1>(__VA_ARGS__) : GO<T, 1, 1, kMtMaxTasks>(__VA_ARGS__);                        \
    return one ? GO<T, 1, WIDE_1, 1>(__VA_ARGS__) : GO<T, 1, WIDE_1, kMtMaxTasks>(__VA_ARGS__);                               \
  } while (0)

template <typename T> static int fwd_pick(const MtFwdArgs& a, bool vec, float loss_scale, float* loss, float* weight_sum, hipStream_t st) {
  MT_PICK(fwd_go, T, a, loss_scale, loss, weight_sum, st);
}
template <typename T> static int bwd_pick(const MtBwdArgs& a, bool vec, float* dw, float* dc, float* dg, float* db, hipStream_t st) {
  MT_PICK(bwd_go, T, a, dw, dc, dg, db, st);
}
#undef MT_PICK

}  // namespace

size_t multitask_head_workspace_bytes(int dim, int tasks) {
  if (dim < 1 || tasks < 1) return 0;
  const size_t fwd = (size_t)kMtMaxBlocks * kMtLossCols * sizeof(float);
  const size_t bwd = (size_t)kMtMaxBlocks * ((size_t)(tasks + 2) * dim + kMtMaxTasks) * sizeof(float);
  return fwd > bwd ? fwd : bwd;
}

int launch_multitask_head_fwd(const void* x, int64_t x_rs, const void* ln_w, const void* ln_b, float eps, const float* w,
                              const float* c, const float* labels, const float* weights, float* logits, float* preds,
                              float* mean, float* rstd, float* loss, float* weight_sum, void* workspace, int64_t rows, int dim,
                              int tasks, int nbin, float loss_scale, int dtype, bool vec, hipStream_t st) {
  const MtFwdArgs a{x, x_rs, ln_w, ln_b, eps, w, c, labels, weights, logits, preds, mean, rstd, (float*)workspace, rows, dim, tasks, nbin};
  switch (dtype) {
    case HSTU_DTYPE_BF16: return fwd_pick<bf16_t>(a, vec, loss_scale, loss, weight_sum, st);
    case HSTU_DTYPE_F16: return fwd_pick<f16_t>(a, vec, loss_scale, loss, weight_sum, st);
    default: return fwd_pick<float>(a, vec, loss_scale, loss, weight_sum, st);
  }
}

int launch_multitask_head_bwd(const float* grad_loss, const float* grad_pred, const void* x, int64_t x_rs, const void* ln_w,
                              const void* ln_b, const float* w, const float* labels, const float* weights, const float* logits,
                              const float* mean, const float* rstd, const float* weight_sum, void* dx, int64_t dx_rs, float* dw,
                              float* dc, float* dln_w, float* dln_b, void* workspace, int64_t rows, int dim, int tasks, int nbin,
                              float loss_scale, int dtype, bool vec, hipStream_t st) {
  const MtBwdArgs a{grad_loss, grad_pred, x, x_rs, ln_w, ln_b, w, labels, weights, logits, mean, rstd, weight_sum, dx, dx_rs,
                    (float*)workspace, rows, dim, tasks, nbin, loss_scale};
  switch (dtype) {
    case HSTU_DTYPE_BF16: return bwd_pick<bf16_t>(a, vec, dw, dc, dln_w, dln_b, st);
    case HSTU_DTYPE_F16: return bwd_pick<f16_t>(a, vec, dw, dc, dln_w, dln_b, st);
    default: return bwd_pick<float>(a, vec, dw, dc, dln_w, dln_b, st);
  }
}
}  // namespace hstu
