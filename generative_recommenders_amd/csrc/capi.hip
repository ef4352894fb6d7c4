// C ABI entry points of libhstu_hip.so (see include/hstu_hip.h): argument validation in the
// spirit of the reference's TORCH_CHECKs (ops/cpp/hstu_attention/flash_common.cpp:339-456),
// then dtype dispatch to the per-dtype launchers.
#include <stdarg.h>
#include <stdio.h>

#include <initializer_list>

#include "capi_internal.h"

namespace hstu {

static thread_local char g_err[512] = "";

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(HSTU_ELAUNCH, "%s: HIP launch failed: %s", what, hipGetErrorString(e));
  return HSTU_OK;
}

static int validate_attn(const HstuAttnParams& p, const char* who) {
  if (!p.q || !p.k || !p.v || !p.seq_offsets) return set_error(HSTU_EINVAL, "%s: q, k, v and seq_offsets must be non-NULL", who);
  if (p.batch < 0 || p.heads <= 0) return set_error(HSTU_EINVAL, "%s: bad batch/heads", who);
  if (p.max_seq_len <= 0) return set_error(HSTU_EINVAL, "%s: max_seq_len must be larger than 0", who);
  if (!is_float_dtype(p.dtype))
    return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32", who);
  const int eb = dtype_bytes(p.dtype);
  const int epu = 16 / eb;
  if (p.dqk <= 0 || p.dv <= 0 || p.dqk % epu || p.dv % epu)
    return set_error(HSTU_EINVAL, "%s: head dims (%d, %d) must be positive multiples of %d", who, p.dqk, p.dv, epu);
  if (!pad_head_dim(p.dqk) || !pad_head_dim(p.dv))
    return set_error(HSTU_EUNSUPPORTED, "%s: head dims (%d, %d) above 128 are not instantiated", who, p.dqk, p.dv);
  const int64_t strides[] = {p.q_row_stride, p.q_head_stride, p.k_row_stride, p.k_head_stride, p.v_row_stride, p.v_head_stride};
  for (int64_t s : strides)
    if ((s * eb) % 16) return set_error(HSTU_EINVAL, "%s: every (row, head) vector must be 16-byte aligned (stride %lld elements)", who, (long long)s);
  if (((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v) & 15) return set_error(HSTU_EINVAL, "%s: q/k/v base pointers must be 16-byte aligned", who);
  if (p.max_attn_len < 0 || p.contextual_seq_len < 0 || p.min_full_attn_seq_len < 0)
    return set_error(HSTU_EINVAL, "%s: negative mask parameter", who);
  if (p.delta_q < 0) return set_error(HSTU_EINVAL, "%s: negative delta_q", who);
  if (p.pos_w) {
    if ((p.ts_w == nullptr) != (p.timestamps == nullptr)) return set_error(HSTU_EINVAL, "%s: ts_w and timestamps must be given together", who);
    if (p.ts_w && (p.num_buckets <= 0 || !(p.bucket_div > 0.f) || p.ts_row_stride < p.max_seq_len))
      return set_error(HSTU_EINVAL, "%s: bad bucket parameters / timestamp stride", who);
  }
  return HSTU_OK;
}

// e4m3 forward: the same checks with 1-byte q / k / v and a bf16 output, and the narrower shape rule of the fp8 kernel
static int validate_attn_fp8(const HstuAttnParams& p, const char* who) {
  if (!p.q || !p.k || !p.v || !p.seq_offsets) return set_error(HSTU_EINVAL, "%s: q, k, v and seq_offsets must be non-NULL", who);
  if (p.batch < 0 || p.heads <= 0) return set_error(HSTU_EINVAL, "%s: bad batch/heads", who);
  if (p.max_seq_len <= 0) return set_error(HSTU_EINVAL, "%s: max_seq_len must be larger than 0", who);
  if (p.dqk != p.dv) return set_error(HSTU_EUNSUPPORTED, "%s: fp8 attention needs dqk == dv (got %d, %d)", who, p.dqk, p.dv);
  if (p.dqk <= 0 || p.dqk % 16) return set_error(HSTU_EINVAL, "%s: fp8 head dims must be positive multiples of 16 (got %d)", who, p.dqk);
  if (!fp8_head_dim(p.dqk)) return set_error(HSTU_EUNSUPPORTED, "%s: fp8 head dim %d above 128 is not instantiated", who, p.dqk);
  if (p.pos_w) return set_error(HSTU_EUNSUPPORTED, "%s: fp8 attention with the relative (research-path) bias is not supported", who);
  const int64_t strides[] = {p.q_row_stride, p.q_head_stride, p.k_row_stride, p.k_head_stride, p.v_row_stride, p.v_head_stride};
  for (int64_t s : strides)
    if (s % 16) return set_error(HSTU_EINVAL, "%s: every fp8 (row, head) vector must be 16-byte aligned (stride %lld elements)", who, (long long)s);
  if (((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v) & 15) return set_error(HSTU_EINVAL, "%s: q/k/v base pointers must be 16-byte aligned", who);
  if (p.max_attn_len < 0 || p.contextual_seq_len < 0 || p.min_full_attn_seq_len < 0)
    return set_error(HSTU_EINVAL, "%s: negative mask parameter", who);
  if (p.delta_q < 0) return set_error(HSTU_EINVAL, "%s: negative delta_q", who);
  return HSTU_OK;
}

static int attn_fwd_fp8(const HstuAttnParams* p, const HstuFp8Descale& ds, void* stream) {
  if (int e = validate_attn_fp8(*p, "hstu_attn_fwd")) return e;
  if (!p->out) return set_error(HSTU_EINVAL, "hstu_attn_fwd: out is NULL");
  if (((p->o_row_stride | p->o_head_stride) * 2) % 16 || ((uintptr_t)p->out & 15))
    return set_error(HSTU_EINVAL, "hstu_attn_fwd: out rows must be 16-byte aligned");
  if (p->batch == 0) return HSTU_OK;
  return launch_attn_fwd_fp8(*p, ds, (hipStream_t)stream);
}

}  // namespace hstu

using namespace hstu;

extern "C" {

int hstu_abi_version(void) { return HSTU_ABI_VERSION; }
const char* hstu_last_error(void) { return g_err; }

int hstu_attn_fwd(const HstuAttnParams* p, void* stream) {
  if (!p) return set_error(HSTU_EINVAL, "hstu_attn_fwd: NULL params");
  if (p->dtype == HSTU_DTYPE_FP8_E4M3) return attn_fwd_fp8(p, HstuFp8Descale{}, stream);   // every descale 1
  if (int e = validate_attn(*p, "hstu_attn_fwd")) return e;
  if (!p->out) return set_error(HSTU_EINVAL, "hstu_attn_fwd: out is NULL");
  if (((p->o_row_stride | p->o_head_stride) * dtype_bytes(p->dtype)) % 16 || ((uintptr_t)p->out & 15))
    return set_error(HSTU_EINVAL, "hstu_attn_fwd: out rows must be 16-byte aligned");
  if (p->batch == 0) return HSTU_OK;   // empty batch: nothing to launch (flash_common.cpp:548-551)
  const AttnPlan pl = plan_attn_fwd(*p);
  if (pl.err) return set_error(pl.err, "%s", pl.msg);
  hipStream_t st = (hipStream_t)stream;
  switch (p->dtype) {
    case HSTU_DTYPE_BF16: return launch_attn_fwd<bf16_t>(pl, *p, st);
    case HSTU_DTYPE_F16: return launch_attn_fwd<f16_t>(pl, *p, st);
    default: return launch_attn_fwd<float>(pl, *p, st);
  }
}

int hstu_attn_fwd_fp8(const HstuAttnParams* p, const HstuFp8Descale* descale, void* stream) {
  if (!p) return set_error(HSTU_EINVAL, "hstu_attn_fwd_fp8: NULL params");
  if (p->dtype != HSTU_DTYPE_FP8_E4M3) return set_error(HSTU_EINVAL, "hstu_attn_fwd_fp8: dtype must be HSTU_DTYPE_FP8_E4M3 (fp8 e4m3 q, k, v)");
  return attn_fwd_fp8(p, descale ? *descale : HstuFp8Descale{}, stream);
}

int hstu_attn_fwd_kernel_name(const HstuAttnParams* p, char* buf, size_t len) {
  if (!p) return set_error(HSTU_EINVAL, "hstu_attn_fwd_kernel_name: NULL params");
  if (p->dtype == HSTU_DTYPE_FP8_E4M3) {
    if (!buf || len == 0) return HSTU_EINVAL;
    buf[0] = 0;
    if (p->dqk != p->dv || !fp8_head_dim(p->dqk) || p->pos_w)
      return set_error(HSTU_EUNSUPPORTED, "fp8 attention is instantiated for dqk == dv, multiples of 16 up to 128, without bias (got %d, %d)",
                       p->dqk, p->dv);
    snprintf(buf, len, "hstu_attn_fwd_fp8_kernel<fp8,%d,%d>", fp8_head_dim(p->dqk), fp8_head_dim(p->dv));
    return HSTU_OK;
  }
  return attn_kernel_name(plan_attn_fwd(*p), buf, len);
}

int hstu_attn_bwd_kernel_name(const HstuAttnBwdParams* p, char* buf, size_t len) {
  if (!p) return set_error(HSTU_EINVAL, "hstu_attn_bwd_kernel_name: NULL params");
  if (p->fwd.dtype == HSTU_DTYPE_FP8_E4M3) {
    if (buf && len) buf[0] = 0;
    return set_error(HSTU_EUNSUPPORTED, "hstu_attn_bwd: fp8 (e4m3) attention is forward-only");
  }
  return attn_kernel_name(plan_attn_bwd(*p), buf, len);
}

size_t hstu_attn_bwd_workspace_bytes(const HstuAttnBwdParams* p) {
  if (!p || p->fwd.dtype == HSTU_DTYPE_FP8_E4M3) return 0;
  return plan_attn_bwd(*p).ws_bytes;
}

int hstu_attn_bwd(const HstuAttnBwdParams* p, void* stream) {
  if (!p) return set_error(HSTU_EINVAL, "hstu_attn_bwd: NULL params");
  if (p->fwd.dtype == HSTU_DTYPE_FP8_E4M3) return set_error(HSTU_EUNSUPPORTED, "hstu_attn_bwd: fp8 (e4m3) attention is forward-only");
  if (int e = validate_attn(p->fwd, "hstu_attn_bwd")) return e;
  if (p->fwd.delta_q != 0) return set_error(HSTU_EUNSUPPORTED, "hstu_attn_bwd: delta_q attention is forward-only (as in the reference)");
  if (!p->dout || !p->dq || !p->dk || !p->dv) return set_error(HSTU_EINVAL, "hstu_attn_bwd: dout, dq, dk, dv must be non-NULL");
  const int eb = dtype_bytes(p->fwd.dtype);
  const int64_t strides[] = {p->do_row_stride, p->do_head_stride, p->dq_row_stride, p->dq_head_stride,
                             p->dk_row_stride, p->dk_head_stride, p->dv_row_stride, p->dv_head_stride};
  for (int64_t s : strides)
    if ((s * eb) % 16) return set_error(HSTU_EINVAL, "hstu_attn_bwd: gradient rows must be 16-byte aligned (stride %lld elements)", (long long)s);
  if (((uintptr_t)p->dout | (uintptr_t)p->dq | (uintptr_t)p->dk | (uintptr_t)p->dv) & 15)
    return set_error(HSTU_EINVAL, "hstu_attn_bwd: gradient base pointers must be 16-byte aligned");
  if (p->fwd.pos_w && (!p->dpos_w || (p->fwd.ts_w && !p->dts_w)))
    return set_error(HSTU_EINVAL, "hstu_attn_bwd: dpos_w / dts_w outputs are required with a relative bias");
  // ahead of every dispatch decision (solo_bias, fold_bias and the general bias kernel all add their table gradients with
  // float atomics into LDS histograms): refused rather than silently not honoured
  if (p->fwd.pos_w && p->deterministic)
    return set_error(HSTU_EUNSUPPORTED, "hstu_attn_bwd: deterministic = 1 is not available with the relative bias (the table gradients are "
                                        "histograms of float atomics)");
  if (p->fwd.batch == 0 || p->total_rows == 0) return HSTU_OK;
  const AttnPlan pl = plan_attn_bwd(*p);
  if (pl.ws_bytes > 0 && !p->workspace) return set_error(HSTU_EINVAL, "hstu_attn_bwd: this shape needs %zu bytes of workspace", pl.ws_bytes);
  if (pl.err) return set_error(pl.err, "%s", pl.msg);
  hipStream_t st = (hipStream_t)stream;
  switch (p->fwd.dtype) {
    case HSTU_DTYPE_BF16: return launch_attn_bwd<bf16_t>(pl, *p, st);
    case HSTU_DTYPE_F16: return launch_attn_bwd<f16_t>(pl, *p, st);
    default: return launch_attn_bwd<float>(pl, *p, st);
  }
}

int hstu_jagged_quantize_fp8(const void* x, int64_t x_row_stride, int64_t x_head_stride, void* x8, float* descale,
                             const void* seq_offsets, int32_t batch, int32_t heads, int32_t dim, int dtype, int index_dtype,
                             void* stream) {
  if (!x || !x8 || !descale || !seq_offsets) return set_error(HSTU_EINVAL, "hstu_jagged_quantize_fp8: x, x8, descale and seq_offsets must be non-NULL");
  if (batch < 0 || heads <= 0 || dim <= 0) return set_error(HSTU_EINVAL, "hstu_jagged_quantize_fp8: bad batch / heads / dim");
  if (!is_float_dtype(dtype))
    return set_error(HSTU_EINVAL, "hstu_jagged_quantize_fp8: x must be bf16, fp16 or fp32");
  if (index_dtype != HSTU_INDEX_I32 && index_dtype != HSTU_INDEX_I64) return set_error(HSTU_EINVAL, "hstu_jagged_quantize_fp8: bad index dtype");
  if (batch == 0) return HSTU_OK;
  return launch_jagged_quantize_fp8(x, x_row_stride, x_head_stride, x8, descale, seq_offsets, batch, heads, dim, dtype, index_dtype,
                                    (hipStream_t)stream);
}

// shared checks of the two jagged_dense_bmm entry points (shape and type codes first: they need no pointer)
static int validate_bmm_shape(const char* who, int64_t total_rows, int32_t batch, int32_t k, int32_t n, int dtype, int index_dtype) {
  if (!is_float_dtype(dtype))
    return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32 (got code %d)", who, dtype);
  if (index_dtype != HSTU_INDEX_I32 && index_dtype != HSTU_INDEX_I64)
    return set_error(HSTU_EINVAL, "%s: seq_offsets must be int32 or int64 (got code %d)", who, index_dtype);
  if (k <= 0 || n <= 0) return set_error(HSTU_EINVAL, "%s: K and N must be positive (got %d, %d)", who, k, n);
  if (batch < 0 || total_rows < 0) return set_error(HSTU_EINVAL, "%s: negative batch / total_rows", who);
  const int epu = dtype == HSTU_DTYPE_F32 ? 4 : 8;
  if (k % epu || n % epu)
    return set_error(HSTU_EINVAL, "%s: K and N (%d, %d) must be multiples of %d elements (16 bytes); zero-pad them", who, k, n, epu);
  return HSTU_OK;
}

static bool bmm_aligned(int eb, const void* p, std::initializer_list<int64_t> strides) {
  if ((uintptr_t)p & 15) return false;
  for (int64_t s : strides)
    if ((s * eb) % 16) return false;
  return true;
}

size_t hstu_jagged_dense_bmm_workspace_bytes(int32_t batch) { return jagged_bmm_workspace_bytes(batch); }

int hstu_jagged_dense_bmm_fwd(const void* jagged, int64_t jagged_row_stride, const void* dense, int64_t dense_batch_stride,
                              int64_t dense_k_stride, int64_t dense_n_stride, const float* bias, int64_t bias_batch_stride,
                              void* out, int64_t out_row_stride, const void* seq_offsets, int64_t total_rows, int32_t batch,
                              int32_t k, int32_t n, void* workspace, int dtype, int index_dtype, void* stream) {
  const char* who = "hstu_jagged_dense_bmm_fwd";
  if (int e = validate_bmm_shape(who, total_rows, batch, k, n, dtype, index_dtype)) return e;
  if (batch == 0 || total_rows == 0) return HSTU_OK;
  if (!jagged || !dense || !out || !seq_offsets || !workspace)
    return set_error(HSTU_EINVAL, "%s: jagged, dense, out, seq_offsets and workspace must be non-NULL", who);
  const int eb = dtype_bytes(dtype);
  if (dense_n_stride != 1 && dense_k_stride != 1)
    return set_error(HSTU_EINVAL, "%s: dense needs a unit stride along K or N (got %lld, %lld)", who, (long long)dense_k_stride,
                     (long long)dense_n_stride);
  if (jagged_row_stride < k || out_row_stride < n) return set_error(HSTU_EINVAL, "%s: a row stride is smaller than a row", who);
  if (!bmm_aligned(eb, jagged, {jagged_row_stride}) || !bmm_aligned(eb, out, {out_row_stride}) ||
      !bmm_aligned(eb, dense, {dense_batch_stride, dense_n_stride == 1 ? dense_k_stride : dense_n_stride}) ||
      ((uintptr_t)workspace & 3) || (bias && ((uintptr_t)bias & 3)))
    return set_error(HSTU_EINVAL, "%s: rows of jagged, dense and out must start 16-byte aligned", who);
  return launch_jagged_bmm_fwd(jagged, jagged_row_stride, dense, dense_batch_stride, dense_k_stride, dense_n_stride, bias,
                               bias_batch_stride, out, out_row_stride, seq_offsets, total_rows, batch, k, n, workspace, dtype,
                               index_dtype, (hipStream_t)stream);
}

int hstu_jagged_dense_bmm_wgrad(const void* jagged, int64_t jagged_row_stride, const void* d_out, int64_t d_out_row_stride,
                                void* d_dense, int64_t d_dense_batch_stride, int64_t d_dense_k_stride, float* d_bias,
                                int64_t d_bias_batch_stride, const void* seq_offsets, int64_t total_rows, int32_t batch, int32_t k,
                                int32_t n, int dtype, int index_dtype, void* stream) {
  const char* who = "hstu_jagged_dense_bmm_wgrad";
  if (int e = validate_bmm_shape(who, total_rows, batch, k, n, dtype, index_dtype)) return e;
  if (batch == 0) return HSTU_OK;
  if (!d_dense || !seq_offsets || (total_rows > 0 && (!jagged || !d_out)))
    return set_error(HSTU_EINVAL, "%s: jagged, d_out, d_dense and seq_offsets must be non-NULL", who);
  const int eb = dtype_bytes(dtype);
  if ((total_rows > 0 && (jagged_row_stride < k || d_out_row_stride < n)) || d_dense_k_stride < n)
    return set_error(HSTU_EINVAL, "%s: a row stride is smaller than a row", who);
  if ((total_rows > 0 && (!bmm_aligned(eb, jagged, {jagged_row_stride}) || !bmm_aligned(eb, d_out, {d_out_row_stride}))) ||
      !bmm_aligned(eb, d_dense, {d_dense_batch_stride, d_dense_k_stride}) || (d_bias && ((uintptr_t)d_bias & 3)))
    return set_error(HSTU_EINVAL, "%s: rows of jagged, d_out and d_dense must start 16-byte aligned", who);
  return launch_jagged_bmm_wgrad(jagged, jagged_row_stride, d_out, d_out_row_stride, d_dense, d_dense_batch_stride,
                                 d_dense_k_stride, d_bias, d_bias_batch_stride, seq_offsets, total_rows, batch, k, n, dtype,
                                 index_dtype, (hipStream_t)stream);
}

size_t hstu_mips_topk_workspace_bytes(int32_t batch, int32_t k) { return mips_topk_workspace_bytes(batch, k); }

int hstu_mips_topk(const void* queries, int64_t q_row_stride, const void* items, int64_t item_row_stride, void* out_scores,
                   int32_t* out_indices, void* workspace, int32_t batch, int32_t num_items, int32_t dim, int32_t k, int dtype,
                   void* stream) {
  const char* who = "hstu_mips_topk";
  if (!is_float_dtype(dtype))
    return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32 (got code %d)", who, dtype);
  if (batch < 0) return set_error(HSTU_EINVAL, "%s: negative batch", who);
  if (num_items <= 0 || dim <= 0) return set_error(HSTU_EINVAL, "%s: num_items and dim must be positive (got %d, %d)", who, num_items, dim);
  const int eb = dtype_bytes(dtype), epu = 16 / eb;
  if (dim % epu) return set_error(HSTU_EINVAL, "%s: dim (%d) must be a multiple of %d elements (16 bytes); zero-pad it", who, dim, epu);
  if (dim > kMipsTopkMaxDim) return set_error(HSTU_EINVAL, "%s: dim %d exceeds the limit of %d", who, dim, kMipsTopkMaxDim);
  if (k < 1 || k > num_items || k > kMipsTopkMaxK)
    return set_error(HSTU_EINVAL, "%s: k must be in [1, min(num_items, %d)] (got k = %d, num_items = %d)", who, kMipsTopkMaxK, k, num_items);
  if (batch == 0) return HSTU_OK;
  if (!queries || !items || !out_scores || !out_indices || !workspace)
    return set_error(HSTU_EINVAL, "%s: queries, items, out_scores, out_indices and workspace must be non-NULL", who);
  if (q_row_stride < dim || item_row_stride < dim) return set_error(HSTU_EINVAL, "%s: a row stride is smaller than a row", who);
  if (!bmm_aligned(eb, queries, {q_row_stride}) || !bmm_aligned(eb, items, {item_row_stride}) || ((uintptr_t)workspace & 15) ||
      ((uintptr_t)out_scores & (eb - 1)) || ((uintptr_t)out_indices & 3))
    return set_error(HSTU_EINVAL, "%s: rows of queries and items and the workspace must start 16-byte aligned", who);
  return launch_mips_topk(queries, q_row_stride, items, item_row_stride, out_scores, out_indices, workspace, batch, num_items, dim, k,
                          dtype, (hipStream_t)stream);
}

int hstu_mol_scores(const void* qc, const void* xc, const void* gq, const void* gi, const void* w1, const void* b1, const void* w2,
                    const void* b2, float* out, int32_t batch, int32_t num_items, int32_t pq, int32_t px, int32_t dim,
                    int32_t hidden, float inv_temperature, int combination, int dtype, void* stream) {
  const char* who = "hstu_mol_scores";
  if (!is_float_dtype(dtype))
    return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32 (got code %d)", who, dtype);
  if (combination != HSTU_MOL_GLU_SILU && combination != HSTU_MOL_GLU_SILU_LN)
    return set_error(HSTU_EINVAL, "%s: combination must be HSTU_MOL_GLU_SILU or HSTU_MOL_GLU_SILU_LN (got %d)", who, combination);
  if (batch < 0 || num_items < 0) return set_error(HSTU_EINVAL, "%s: negative batch or num_items", who);
  if (pq < 1 || px < 1 || (int64_t)pq * px > kMolMaxLogits)
    return set_error(HSTU_EUNSUPPORTED, "%s: %d x %d logits; 1 <= P_Q, P_X and P_Q * P_X <= %d are built", who, pq, px, kMolMaxLogits);
  if (dim < 1 || dim > kMolMaxDim || dim % 8)
    return set_error(HSTU_EUNSUPPORTED, "%s: dot product dimension %d; multiples of 8 up to %d are built (zero-pad it)", who, dim,
                     kMolMaxDim);
  if (hidden < 0 || hidden > kMolMaxHidden)
    return set_error(HSTU_EUNSUPPORTED, "%s: %d hidden units; 0 <= H <= %d are built", who, hidden, kMolMaxHidden);
  if (batch == 0 || num_items == 0) return HSTU_OK;
  if (!qc || !xc || !gq || !gi || !w1 || !b2 || !out || (hidden > 0 && (!b1 || !w2)))
    return set_error(HSTU_EINVAL, "%s: operands, weights and out must be non-NULL", who);
  const int eb = dtype_bytes(dtype);
  if ((((uintptr_t)qc | (uintptr_t)xc) & 15) || (((uintptr_t)gq | (uintptr_t)gi | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2) & (eb - 1)) ||
      ((uintptr_t)out & 3))
    return set_error(HSTU_EINVAL, "%s: qc and xc must be 16-byte aligned, the other operands element aligned", who);
  return launch_mol_scores(qc, xc, gq, gi, w1, b1, w2, b2, out, batch, num_items, pq, px, dim, hidden, inv_temperature,
                           combination == HSTU_MOL_GLU_SILU_LN, dtype, (hipStream_t)stream);
}

// ---- multitask prediction head --------------------------------------------------------------------------------------------
static int validate_multitask(const char* who, const void* x, int64_t x_rs, const void* dx, int64_t dx_rs, const void* ln_w,
                              const void* ln_b, int64_t rows, int32_t dim, int32_t tasks, int32_t nbin, int dtype,
                              std::initializer_list<const void*> f32_ptrs, const void* workspace, bool* vec) {
  if (!is_float_dtype(dtype))
    return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32 (got code %d)", who, dtype);
  if (tasks < 1 || tasks > HSTU_MULTITASK_MAX_TASKS)
    return set_error(HSTU_EINVAL, "%s: num_tasks must be in [1, %d] (got %d)", who, HSTU_MULTITASK_MAX_TASKS, tasks);
  if (nbin < 0 || nbin > tasks)
    return set_error(HSTU_EINVAL, "%s: num_binary must be in [0, num_tasks = %d] (got %d)", who, tasks, nbin);
  if (rows < 0) return set_error(HSTU_EINVAL, "%s: negative rows", who);
  if (dim <= 0) return set_error(HSTU_EINVAL, "%s: dim must be positive (got %d)", who, dim);
  const int eb = dtype_bytes(dtype), epu = 16 / eb;
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)dx | (uintptr_t)ln_w | (uintptr_t)ln_b;
  if (bits & (eb - 1)) return set_error(HSTU_EINVAL, "%s: x, dx and the norm's weight and bias must be aligned to their element size (%d bytes)", who, eb);
  for (const void* p : f32_ptrs)
    if ((uintptr_t)p & 3) return set_error(HSTU_EINVAL, "%s: an fp32 tensor is not 4-byte aligned", who);
  if ((uintptr_t)workspace & 15) return set_error(HSTU_EINVAL, "%s: the workspace must be 16-byte aligned", who);
  if (x_rs < dim || (dx && dx_rs < dim)) return set_error(HSTU_EINVAL, "%s: a row stride is smaller than a row", who);
  *vec = dim % epu == 0 && (bits & 15) == 0 && (x_rs * eb) % 16 == 0 && (!dx || (dx_rs * eb) % 16 == 0);
  const int lim = *vec ? kMultitaskMaxDimVec : kMultitaskMaxDimScalar;
  if (dim > lim) return set_error(HSTU_EINVAL, "%s: dim %d exceeds the %d supported with this alignment", who, dim, lim);
  return HSTU_OK;
}

size_t hstu_multitask_head_workspace_bytes(int32_t dim, int32_t num_tasks) { return multitask_head_workspace_bytes(dim, num_tasks); }

int hstu_multitask_head_fwd(const void* x, int64_t x_row_stride, const void* ln_weight, const void* ln_bias, float eps,
                            const float* w, const float* c, const float* labels, const float* weights, float* logits,
                            float* preds, float* mean, float* rstd, float* loss, float* weight_sum, void* workspace,
                            int64_t rows, int32_t dim, int32_t num_tasks, int32_t num_binary, float loss_scale, int dtype,
                            void* stream) {
  const char* who = "hstu_multitask_head_fwd";
  bool vec = false;
  if (int e = validate_multitask(who, x, x_row_stride, nullptr, 0, ln_weight, ln_bias, rows, dim, num_tasks, num_binary, dtype,
                                 {w, c, labels, weights, logits, preds, mean, rstd, loss, weight_sum}, workspace, &vec))
    return e;
  if (rows == 0) {   // (a (T, 0) labels tensor has no address: the reduced outputs are zeroed wherever they are given)
    if (loss) (void)hipMemsetAsync(loss, 0, num_tasks * sizeof(float), (hipStream_t)stream);
    if (weight_sum) (void)hipMemsetAsync(weight_sum, 0, num_tasks * sizeof(float), (hipStream_t)stream);
    return HSTU_OK;
  }
  if (labels && (!loss || !weight_sum)) return set_error(HSTU_EINVAL, "%s: labels need loss and weight_sum", who);
  if (weights && !labels) return set_error(HSTU_EINVAL, "%s: weights without labels", who);
  if (!x || !ln_weight || !ln_bias || !w || !c || !preds || (labels && !workspace))
    return set_error(HSTU_EINVAL, "%s: x, ln_weight, ln_bias, w, c, preds (and with labels the workspace) must be non-NULL", who);
  return launch_multitask_head_fwd(x, x_row_stride, ln_weight, ln_bias, eps, w, c, labels, weights, logits, preds, mean, rstd, loss,
                                   weight_sum, workspace, rows, dim, num_tasks, num_binary, loss_scale, dtype, vec, (hipStream_t)stream);
}

int hstu_multitask_head_bwd(const float* grad_loss, const float* grad_pred, const void* x, int64_t x_row_stride,
                            const void* ln_weight, const void* ln_bias, const float* w, const float* labels, const float* weights,
                            const float* logits, const float* mean, const float* rstd, const float* weight_sum, void* dx,
                            int64_t dx_row_stride, float* dw, float* dc, float* dln_weight, float* dln_bias, void* workspace,
                            int64_t rows, int32_t dim, int32_t num_tasks, int32_t num_binary, float loss_scale, int dtype,
                            void* stream) {
  const char* who = "hstu_multitask_head_bwd";
  bool vec = false;
  if (int e = validate_multitask(who, x, x_row_stride, dx, dx_row_stride, ln_weight, ln_bias, rows, dim, num_tasks, num_binary, dtype,
                                 {grad_loss, grad_pred, w, labels, weights, logits, mean, rstd, weight_sum, dw, dc, dln_weight, dln_bias},
                                 workspace, &vec))
    return e;
  if (!dw || !dc || !dln_weight || !dln_bias) return set_error(HSTU_EINVAL, "%s: dw, dc, dln_weight and dln_bias are required", who);
  if (rows == 0) {
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(dw, 0, (size_t)num_tasks * dim * sizeof(float), st);
    (void)hipMemsetAsync(dc, 0, num_tasks * sizeof(float), st);
    (void)hipMemsetAsync(dln_weight, 0, dim * sizeof(float), st);
    (void)hipMemsetAsync(dln_bias, 0, dim * sizeof(float), st);
    return HSTU_OK;
  }
  if (grad_loss && (!labels || !weight_sum)) return set_error(HSTU_EINVAL, "%s: grad_loss needs labels and weight_sum", who);
  if (!x || !ln_weight || !ln_bias || !w || !logits || !mean || !rstd || !dx || !workspace)
    return set_error(HSTU_EINVAL, "%s: x, ln_weight, ln_bias, w, logits, mean, rstd, dx and the workspace must be non-NULL", who);
  return launch_multitask_head_bwd(grad_loss, grad_pred, x, x_row_stride, ln_weight, ln_bias, w, labels, weights, logits, mean, rstd,
                                   weight_sum, dx, dx_row_stride, dw, dc, dln_weight, dln_bias, workspace, rows, dim, num_tasks,
                                   num_binary, loss_scale, dtype, vec, (hipStream_t)stream);
}

// ---- jagged causal softmax attention ----------------------------------------------------------------------------------------
// checks that need no pointer first (shape, type codes, ranges), then pointers, then alignment
static int validate_softmax_attn(const char* who, const SoftmaxAttnArgs& a, int64_t total_rows, bool backward, bool* empty) {
  if (!is_float_dtype(a.dtype))
    return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32 (got code %d)", who, a.dtype);
  if (a.index_dtype != HSTU_INDEX_I32 && a.index_dtype != HSTU_INDEX_I64)
    return set_error(HSTU_EINVAL, "%s: seq_offsets must be int32 or int64 (got code %d)", who, a.index_dtype);
  if (a.batch < 0 || total_rows < 0 || a.heads <= 0) return set_error(HSTU_EINVAL, "%s: bad batch / total_rows / heads", who);
  if (a.head_dim <= 0) return set_error(HSTU_EINVAL, "%s: head_dim must be positive (got %d)", who, a.head_dim);
  if (a.head_dim > HSTU_SOFTMAX_ATTN_MAX_HEAD_DIM)
    return set_error(HSTU_EUNSUPPORTED, "%s: head_dim %d exceeds the limit of %d", who, a.head_dim, HSTU_SOFTMAX_ATTN_MAX_HEAD_DIM);
  const int eb = dtype_bytes(a.dtype), epu = 16 / eb;
  if (a.head_dim % epu)
    return set_error(HSTU_EINVAL, "%s: head_dim (%d) must be a multiple of %d elements (16 bytes); zero-pad it", who, a.head_dim, epu);
  if (a.max_seq_len < 1) return set_error(HSTU_EINVAL, "%s: max_seq_len must be at least 1 (got %d)", who, a.max_seq_len);
  if (a.max_seq_len > HSTU_SOFTMAX_ATTN_MAX_SEQ_LEN)
    return set_error(HSTU_EUNSUPPORTED, "%s: max_seq_len %d exceeds the limit of %d", who, a.max_seq_len, HSTU_SOFTMAX_ATTN_MAX_SEQ_LEN);
  if (!(a.dropout_p >= 0.f && a.dropout_p < 1.f)) return set_error(HSTU_EINVAL, "%s: dropout_p must be in [0, 1) (got %g)", who, (double)a.dropout_p);
  if (!(a.scale == a.scale)) return set_error(HSTU_EINVAL, "%s: scale is NaN", who);
  *empty = a.batch == 0 || total_rows == 0;
  if (*empty) return HSTU_OK;
  if (!a.q || !a.k || !a.v || !a.out || !a.lse || !a.offsets)
    return set_error(HSTU_EINVAL, "%s: q, k, v, out, lse and seq_offsets must be non-NULL", who);
  if (backward && (!a.dout || !a.delta || !a.dq || !a.dk || !a.dv))
    return set_error(HSTU_EINVAL, "%s: dout, delta, dq, dk and dv must be non-NULL", who);
  const int64_t strides[] = {a.q_rs, a.q_hs, a.k_rs, a.k_hs, a.v_rs, a.v_hs};
  for (int64_t s : strides)
    if ((s * eb) % 16) return set_error(HSTU_EINVAL, "%s: every (row, head) vector must be 16-byte aligned (stride %lld elements)", who, (long long)s);
  if (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out | (uintptr_t)a.dout | (uintptr_t)a.dq | (uintptr_t)a.dk |
       (uintptr_t)a.dv) & 15)
    return set_error(HSTU_EINVAL, "%s: tensor base pointers must be 16-byte aligned", who);
  if (((uintptr_t)a.lse | (uintptr_t)a.delta) & 3) return set_error(HSTU_EINVAL, "%s: lse / delta must be 4-byte aligned", who);
  return HSTU_OK;
}

int hstu_softmax_attn_supported(int dtype, int32_t head_dim, int32_t max_seq_len) {
  if (!is_float_dtype(dtype)) return 0;
  return head_dim >= 1 && head_dim <= HSTU_SOFTMAX_ATTN_MAX_HEAD_DIM && max_seq_len >= 1 && max_seq_len <= HSTU_SOFTMAX_ATTN_MAX_SEQ_LEN;
}

int hstu_softmax_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k, int64_t k_row_stride,
                          int64_t k_head_stride, const void* v, int64_t v_row_stride, int64_t v_head_stride, void* out, float* lse,
                          const void* seq_offsets, int64_t total_rows, int32_t batch, int32_t heads, int32_t head_dim,
                          int32_t max_seq_len, float scale, float dropout_p, uint64_t seed, int dtype, int index_dtype,
                          void* stream) {
  SoftmaxAttnArgs a{};
  a.q = q; a.k = k; a.v = v;
  a.q_rs = q_row_stride; a.q_hs = q_head_stride; a.k_rs = k_row_stride; a.k_hs = k_head_stride; a.v_rs = v_row_stride; a.v_hs = v_head_stride;
  a.out = out; a.lse = lse; a.offsets = seq_offsets;
  a.batch = batch; a.heads = heads; a.head_dim = head_dim; a.max_seq_len = max_seq_len;
  a.scale = scale; a.dropout_p = dropout_p; a.seed = seed; a.dtype = dtype; a.index_dtype = index_dtype;
  bool empty = false;
  if (int e = validate_softmax_attn("hstu_softmax_attn_fwd", a, total_rows, false, &empty)) return e;
  if (empty) return HSTU_OK;
  return launch_softmax_attn_fwd(a, (hipStream_t)stream);
}

int hstu_softmax_attn_bwd(const void* dout, const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k,
                          int64_t k_row_stride, int64_t k_head_stride, const void* v, int64_t v_row_stride, int64_t v_head_stride,
                          const void* out, const float* lse, float* delta, void* dq, void* dk, void* dv, const void* seq_offsets,
                          int64_t total_rows, int32_t batch, int32_t heads, int32_t head_dim, int32_t max_seq_len, float scale,
                          float dropout_p, uint64_t seed, int dtype, int index_dtype, void* stream) {
  SoftmaxAttnArgs a{};
  a.q = q; a.k = k; a.v = v;
  a.q_rs = q_row_stride; a.q_hs = q_head_stride; a.k_rs = k_row_stride; a.k_hs = k_head_stride; a.v_rs = v_row_stride; a.v_hs = v_head_stride;
  a.out = out; a.lse = lse; a.dout = dout; a.delta = delta; a.dq = dq; a.dk = dk; a.dv = dv; a.offsets = seq_offsets;
  a.batch = batch; a.heads = heads; a.head_dim = head_dim; a.max_seq_len = max_seq_len;
  a.scale = scale; a.dropout_p = dropout_p; a.seed = seed; a.dtype = dtype; a.index_dtype = index_dtype;
  bool empty = false;
  if (int e = validate_softmax_attn("hstu_softmax_attn_bwd", a, total_rows, true, &empty)) return e;
  if (empty) return HSTU_OK;
  return launch_softmax_attn_bwd(a, (hipStream_t)stream);
}

}  // extern "C"
