/*
 * hstu_hip.h -- C ABI of libhstu_hip.so, the MI355X (gfx950) HSTU hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  Every
 * entry point cites the reference interface it replaces (paths relative to
 * /root/reference/generative_recommenders).  All functions are stream-ordered
 * (launch on `stream`, a hipStream_t passed as void*; NULL = default stream),
 * never synchronise the host, never allocate, borrow their inputs and write only
 * to the output / workspace pointers they are given.  Return 0 on success, a
 * negative HSTU_E* code otherwise; hstu_last_error() holds the message (the
 * analogue of the reference's TORCH_CHECK text, ops/cpp/hstu_attention/
 * flash_common.cpp:339-456).
 *
 * Tensors are jagged: row r of user b lives at row (seq_offsets[b] + r) of a
 * (total_rows, heads, head_dim) array whose last dimension is contiguous; row
 * and head strides are given in ELEMENTS and are arbitrary (q/k/v may be views
 * of one fused uvqk buffer, triton_hstu_preprocess_and_attention.py:200-252),
 * but every (row, head) vector must start 16-byte aligned.
 */
#ifndef HSTU_HIP_H_
#define HSTU_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSTU_ABI_VERSION 13

enum {
  HSTU_OK = 0,
  HSTU_EINVAL = -1,      /* bad argument (shape, alignment, dtype) */
  HSTU_EUNSUPPORTED = -2,/* head dim / dtype combination not instantiated */
  HSTU_ELAUNCH = -3,     /* HIP launch error */
};

/* HSTU_DTYPE_FP8_E4M3: attention forward only -- q, k, v are OCP e4m3fn (torch.float8_e4m3fn), out is bf16 */
enum { HSTU_DTYPE_BF16 = 0, HSTU_DTYPE_F16 = 1, HSTU_DTYPE_F32 = 2, HSTU_DTYPE_FP8_E4M3 = 3 };
enum { HSTU_INDEX_I32 = 0, HSTU_INDEX_I64 = 1 };

/*
 * Attention problem description, shared by forward and backward.  Models the
 * argument list of hstu_mha (ops/hstu_attention.py:44-61) /
 * hstu::hstu_mha_fwd|bwd (ops/cpp/hstu_attention/flash_api.cpp:275-352) and the
 * POD role of Flash_fwd_params (ops/cpp/hstu_attention/flash.h:23-141).
 *
 *   P[i,j] = silu(alpha * <q_i, k_j>) * scale * M[i,j],   O = P V
 *
 * scale = 1/max_seq_len in the reference (pt_hstu_attention.py:151); M is the
 * causal/target/window/contextual mask of pt_hstu_attention.py:32-84.
 */
typedef struct HstuAttnParams {
  /* data */
  const void* q;          /* (total_q_rows, H, dqk) */
  const void* k;          /* (total_rows,   H, dqk) */
  const void* v;          /* (total_rows,   H, dv)  */
  void* out;              /* fwd: (total_q_rows, H, dv), written */
  const void* seq_offsets;/* (B+1) int32|int64, device */
  const void* num_targets;/* (B) int32|int64 or NULL */
  int64_t q_row_stride, q_head_stride;
  int64_t k_row_stride, k_head_stride;
  int64_t v_row_stride, v_head_stride;
  int64_t o_row_stride, o_head_stride;
  /* shape */
  int32_t batch;          /* B */
  int32_t heads;          /* H */
  int32_t dqk, dv;        /* head dims; multiples of 8 (16-bit) / 4 (fp32), <= 128 */
  int32_t max_seq_len;    /* N: launch bound on per-user length (grid size) */
  int32_t delta_q;        /* 0: q is jagged like k/v.  >0: q holds the last
                             delta_q rows of every user, densely (B*delta_q rows):
                             delta_hstu_mha, ops/hstu_attention.py:131-203 */
  /* semantics */
  float alpha;
  float scale;            /* 1/max_seq_len of the CALLER (not necessarily 1/N above) */
  int32_t max_attn_len;
  int32_t contextual_seq_len;
  int32_t min_full_attn_seq_len;
  /* types */
  int32_t dtype;          /* HSTU_DTYPE_* of q,k,v,out,dout,dq,dk,dv */
  int32_t offsets_dtype;  /* HSTU_INDEX_* of seq_offsets */
  int32_t targets_dtype;  /* HSTU_INDEX_* of num_targets */
  /*
   * Optional additive pre-activation bias of the research path
   * (RelativeBucketedTimeAndPositionBasedBias, research/modeling/sequential/hstu.py:87-144):
   *   S[i,j] += pos_w[(N-1) + j - i] + ts_w[clamp(floor(log(max(|ts[i+1]-ts[j]|,1)) / bucket_div), 0, num_buckets)]
   * with ts[N] := ts[N-1], shared by all heads, N = max_seq_len.  pos_w == NULL disables it.
   * ts_w / timestamps may be NULL (position-only bias, RelativePositionalBias :66-84).
   */
  const float* pos_w;          /* (2N-1) fp32 */
  const float* ts_w;           /* (num_buckets+1) fp32 or NULL */
  const int64_t* timestamps;   /* (B, ts_row_stride) int64 or NULL */
  int64_t ts_row_stride;
  int32_t num_buckets;         /* 128 in every shipped config */
  float bucket_div;            /* 0.301 */
  /* optional: device pointer to ONE float that replaces `scale` (read by the kernels at launch time, no host
   * sync) -- the reference's `attn_scale` tensor, of which its kernels use element 0 (flash_api.cpp:283,
   * mainloop_fwd_sm80.h:790-793, mainloop_bwd_sm80.h:892-894).  NULL: `scale` is used. */
  const float* attn_scale;
  /* optional: a permutation of 0..batch-1 (int32, device).  Workgroup slot i then takes user user_order[i]: the
   * reference's `sort_by_length` (ops/triton/triton_hstu_attention.py:1968-1973 sorts the lengths in descending order
   * and walks the users in that order; the CUDA kernels' dynamic tile scheduler, flash_common.cpp:496-507, serves the
   * same purpose): with long-tailed length distributions the heavy users start first and the launch does not end on
   * them.  Results never depend on it.  NULL: users in index order. */
  const int32_t* user_order;
} HstuAttnParams;

/*
 * Backward-only additions (hstu::hstu_mha_bwd, flash_api.cpp:323-346: dq/dk/dv
 * are PRE-ALLOCATED by the caller and may be strided views).
 */
typedef struct HstuAttnBwdParams {
  HstuAttnParams fwd;     /* q,k,v,offsets,... as in forward; fwd.out unused */
  const void* dout;       /* (total_rows, H, dv) */
  void* dq; void* dk; void* dv;
  int64_t do_row_stride, do_head_stride;
  int64_t dq_row_stride, dq_head_stride;
  int64_t dk_row_stride, dk_head_stride;
  int64_t dv_row_stride, dv_head_stride;
  void* workspace;        /* hstu_attn_bwd_workspace_bytes() bytes, or NULL if 0 */
  int64_t total_rows;     /* rows of q/k/v (= seq_offsets[B]), needed to size/zero the workspace */
  float* dpos_w;          /* out (2N-1) fp32, required iff fwd.pos_w != NULL */
  float* dts_w;           /* out (num_buckets+1) fp32, required iff fwd.ts_w != NULL */
  int deterministic;      /* ABI v8: != 0 -> every sum in a fixed order (hstu::hstu_mha_bwd's `deterministic`, flash_api.cpp:291;
                           * the CUDA reference serialises its dQ adds with a semaphore, flash_common.cpp:806-858).  One key block
                           * (the folded / 4-wave / one-wave kernels): always the case.  Several key blocks: each block's fp32 dq
                           * partial goes to a slab of its own and the slabs are added in block order (workspace = number of key
                           * blocks x total_rows x heads x dqk x 4 bytes, all of it zeroed and read back: at max_seq_len 8192 that
                           * is dozens of slabs -- hstu_attn_bwd_workspace_bytes reports it, size the batch accordingly).  With the research-path bias
                           * (table gradients are histograms of float atomics) the call is refused: HSTU_EUNSUPPORTED. */
} HstuAttnBwdParams;

/* library identity / errors */
int hstu_abi_version(void);
const char* hstu_last_error(void);

/* HSTU attention forward.  Replaces triton_hstu_attention_fwd
 * (ops/triton/triton_hstu_attention.py:1767-1846), triton_cached_hstu_mha
 * (:2095-2170, when delta_q > 0) and hstu::hstu_mha_fwd (flash_api.cpp:34-110). */
int hstu_attn_fwd(const HstuAttnParams* p, void* stream);

/* HSTU attention backward: dq, dk, dv from dout.  Replaces
 * triton_hstu_attention_bwd (triton_hstu_attention.py:1849-1948) and
 * hstu::hstu_mha_bwd (flash_api.cpp:111-141).  fp32 scratch is needed only when
 * one user's keys do not fit one workgroup. */
size_t hstu_attn_bwd_workspace_bytes(const HstuAttnBwdParams* p);
int hstu_attn_bwd(const HstuAttnBwdParams* p, void* stream);

/* Which kernel instantiation hstu_attn_fwd / hstu_attn_bwd dispatches for these shapes, dtype and mask / bias
 * options (pointers are not dereferenced; only pos_w == NULL or not matters), as the name a profiler shows, e.g.
 * "hstu_attn_bwd_fold_kernel<bf16,128,128>".  Written NUL-terminated into buf (truncated to len); returns HSTU_OK,
 * or the code hstu_attn_* would refuse the call with.  The reference exposes the same information only through its
 * dispatcher branches (ops/hstu_attention.py:87-128, flash_common.cpp:496-507). */
int hstu_attn_fwd_kernel_name(const HstuAttnParams* p, char* buf, size_t len);
int hstu_attn_bwd_kernel_name(const HstuAttnBwdParams* p, char* buf, size_t len);

/*
 * fp8 attention forward (dtype == HSTU_DTYPE_FP8_E4M3): the e4m3 path of hstu::hstu_mha_fwd
 * (ops/cpp/hstu_attention/flash_common.cpp:222-305, 448-536).  q, k, v are e4m3 (row / head strides in ELEMENTS = bytes,
 * 16-byte aligned vectors), out is bf16 (strides in bf16 elements).  Per user b and head h:
 *   out[i,h,:] = sum_j silu(alpha qd kd <q_i,k_j>) * scale * M[i,j] * vd * v_j
 * with qd = q[b * q_batch_stride + h * q_head_stride] (fp32, device) and likewise kd, vd; a NULL pointer means 1.  The
 * reference's kernels load these descales but never apply them; here they are applied.  dqk == dv, multiples of 16, <= 128
 * (64 and 128 instantiated, smaller heads zero-padded to 64); every mask option, attn_scale, user_order and delta_q > 0;
 * no relative bias (pos_w must be NULL).  hstu_attn_fwd takes HSTU_DTYPE_FP8_E4M3 too (all descales 1); the backward
 * entry points answer HSTU_EUNSUPPORTED for it.
 */
typedef struct HstuFp8Descale {
  const float* q;
  const float* k;
  const float* v;
  int64_t q_batch_stride, q_head_stride;
  int64_t k_batch_stride, k_head_stride;
  int64_t v_batch_stride, v_head_stride;
} HstuFp8Descale;
int hstu_attn_fwd_fp8(const HstuAttnParams* p, const HstuFp8Descale* descale, void* stream);

/* Per-(user, head) e4m3 quantizer of a jagged (total_rows, heads, dim) tensor x (bf16 / fp16 / fp32 `dtype`, row / head
 * strides in elements, last dim contiguous -- e.g. a view of the fused uvqk buffer):
 *   descale[b * heads + h] = amax over user b's rows of head h of |x| / 448   (1 when that amax is 0)
 *   x8[r, h, c] = e4m3(clamp(x[r, h, c] / descale[b, h], -448, 448))          (IEEE division, round to nearest even)
 * x8 is a contiguous (total_rows, heads, dim) e4m3 array, descale a contiguous (batch, heads) fp32 array.  The caller has no
 * other way to form per-user amaxes of a jagged tensor. */
int hstu_jagged_quantize_fp8(const void* x, int64_t x_row_stride, int64_t x_head_stride, void* x8, float* descale,
                             const void* seq_offsets, int32_t batch, int32_t heads, int32_t dim, int dtype, int index_dtype,
                             void* stream);

/* out[0] = 0, out[i+1] = sum(in[0..i]); n elements in, n+1 out; dtype preserved.
 * Replaces hstu::complete_cumsum (ops/cpp/complete_cumsum.cu:7-47) and
 * fbgemm::asynchronous_complete_cumsum (call site modules/stu.py:97). */
int hstu_complete_cumsum(const void* in, void* out, int64_t n, int index_dtype, void* stream);

/*
 * Row copies between jagged 2-D tensors (bit-exact, elem_bytes in {1,2,4,8};
 * rows are `dim` elements, contiguous).  Either side may be dense: pass
 * offsets == NULL and its fixed per-user length in max_len_*.
 *
 * concat: out rows of user b = [right[:n_prefix] ; left ; right[n_prefix:]]
 * split : inverse.  n_prefix = 0 gives plain concat_2D_jagged / split_2D_jagged
 * (ops/jagged_tensors.py:55-144, ops/triton/triton_jagged_tensors.py:31-142);
 * n_prefix > 0 gives hstu_concat_l2_embeddings / hstu_split_l2_embeddings
 * (ops/jagged_tensors.py:147-207).
 */
int hstu_concat_2d_jagged(const void* left, const void* right, void* out,
                          const void* offsets_left, const void* offsets_right,
                          int32_t max_len_left, int32_t max_len_right, int32_t max_seq_len,
                          int32_t batch, int32_t dim, int32_t elem_bytes, int32_t n_prefix,
                          int index_dtype, void* stream);
int hstu_split_2d_jagged(const void* in, void* left, void* right,
                         const void* offsets_left, const void* offsets_right,
                         int32_t max_len_left, int32_t max_len_right, int32_t max_seq_len,
                         int32_t batch, int32_t dim, int32_t elem_bytes, int32_t n_prefix,
                         int index_dtype, void* stream);

/* jagged (total, dim) <-> padded dense (batch, max_len, dim); rows >= max_len are
 * dropped, missing rows are filled with zero bytes.  Replaces
 * fbgemm::jagged_to_padded_dense / fbgemm::dense_to_jagged as used at
 * ops/pytorch/pt_hstu_attention.py:97-125,167-171 and
 * research/modeling/sequential/hstu.py:523,534. */
int hstu_jagged_to_padded_dense(const void* values, void* dense, const void* offsets,
                                int32_t batch, int32_t max_len, int32_t dim, int32_t elem_bytes,
                                int index_dtype, void* stream);
int hstu_dense_to_jagged(const void* dense, void* values, const void* offsets,
                         int32_t batch, int32_t max_len, int32_t dim, int32_t elem_bytes,
                         int index_dtype, void* stream);

/* In-place KV-cache append: for every user b the LAST `tail` rows of its region
 * [offsets[b], offsets[b+1]) of the jagged buffer `values` (rows of dim * elem_bytes bytes) are overwritten with
 * dense[b*tail .. (b+1)*tail).  With it STULayer.cached_forward (modules/stu.py:354-418) writes only the new
 * microbatch's K/V rows into a persistent [cache ; delta] buffer instead of rebuilding that buffer with
 * concat_2D_jagged on every call (_construct_full_kv, modules/stu.py:134-172: O(history) bytes per microbatch). */
int hstu_jagged_write_tail(const void* dense, void* values, const void* offsets, int32_t batch, int32_t tail, int32_t dim,
                           int32_t elem_bytes, int index_dtype, void* stream);

/* 1-D jagged helpers: hstu::expand_1d_jagged_to_dense
 * (ops/cpp/expand_1d_jagged_to_dense.cu:31-103; pads with the user's LAST value,
 * zeros if empty) and hstu::concat_1d_jagged_jagged
 * (ops/cpp/concat_1d_jagged_jagged.cu:33-127).  elem_bytes in {4, 8}. */
int hstu_expand_1d_jagged_to_dense(const void* values, const void* offsets, void* dense,
                                   int32_t batch, int32_t max_len, int32_t elem_bytes,
                                   int index_dtype, void* stream);
int hstu_concat_1d_jagged_jagged(const void* values_left, const void* offsets_left,
                                 const void* values_right, const void* offsets_right,
                                 void* out, int32_t batch, int32_t elem_bytes,
                                 int index_dtype, void* stream);

/*
 * Row-wise layer norm with affine, fp32 math (ops/layer_norm.py:46-76,
 * ops/triton/triton_layer_norm.py:312-470).  fwd writes y and (optionally)
 * mean / rstd (fp32, per row); bwd returns dx and fp32 dweight / dbias.
 */
int hstu_layer_norm_fwd(const void* x, const void* weight, const void* bias, void* y,
                        float* mean, float* rstd, int64_t rows, int32_t dim, float eps,
                        int dtype, void* stream);
/* ABI v9: y = LayerNorm(x) . W^T + bias as ONE kernel -- the UVQK projection of hstu_compute_uqvk
 * (ops/hstu_compute.py:62-89: layer_norm + addmm; Triton: ops/triton/triton_layer_norm.py:77-309 followed by
 * ops/triton/triton_addmm.py:185-340).  x (rows, k) with leading dimension ldx, w_nk the (n, k) K-contiguous weight
 * (= the reference's (k, n) parameter transposed), y (rows, n) with leading dimension ldy; normed (rows, k; the
 * normalised rows, as hstu_layer_norm_fwd would write them), mean and rstd (fp32, per row) are optional outputs.
 * bf16 / fp16, k == 512, n a multiple of 32 up to 4096, 16-byte aligned pointers, leading dimensions multiples of 8:
 * hstu_ln_linear_fwd_supported says whether a shape qualifies (callers otherwise run hstu_layer_norm_fwd + a GEMM). */
int hstu_ln_linear_fwd_supported(int64_t rows, int32_t k, int32_t n, int dtype);
int hstu_ln_linear_fwd(const void* x, int64_t ldx, const void* ln_weight, const void* ln_bias, float eps,
                       const void* w_nk, const void* bias, void* y, int64_t ldy, void* normed, int64_t ldn,
                       float* mean, float* rstd, int64_t rows, int32_t k, int32_t n, int dtype, void* stream);
/* ABI v12: y = x * sigmoid(LayerNorm(x)) -- swish_layer_norm (ops/layer_norm.py:79-112; math ops/pytorch/pt_layer_norm.py:41-62;
 * Triton: ops/triton/triton_layer_norm.py), the gate SwishLayerNorm puts in front of the MLPs of the input preprocessors
 * (modules/preprocessors.py:160,181), the contextual MLPs (modules/contextualize_mlps.py:63,116) and DlrmHSTU
 * (modules/dlrm_hstu.py:144,240).  Same contract as hstu_layer_norm_fwd / _bwd: fp32 math, mean / rstd (fp32, per row) are
 * outputs of the forward (may be NULL) and inputs of the backward, dweight / dbias fp32, partial_ws of
 * hstu_norm_bwd_workspace_bytes(rows, dim) bytes; rows == 0 zeroes dweight / dbias. */
int hstu_swish_layer_norm_fwd(const void* x, const void* weight, const void* bias, void* y, float* mean, float* rstd,
                              int64_t rows, int32_t dim, float eps, int dtype, void* stream);
int hstu_swish_layer_norm_bwd(const void* dy, const void* x, const void* weight, const void* bias, const float* mean,
                              const float* rstd, void* dx, float* dweight, float* dbias, float* partial_ws, int64_t rows,
                              int32_t dim, int dtype, void* stream);
/* RMS norm (additive to ABI v13): y = x rstd weight with rstd = 1 / sqrt(mean_j(x_j^2) + eps) -- RMSNorm
 * (ops/layer_norm.py:139-158; Triton: ops/triton/triton_layer_norm.py:525-749, whose semantics these follow: fp32 math,
 * one rounding at the store, y in x's dtype).  Same contract as hstu_layer_norm_fwd / _bwd without the mean and the bias:
 * weight (dim) in `dtype`, rstd (fp32, per row) is an output of the forward (may be NULL) and an input of the backward,
 *   dx = (weight dy - xhat mean_j(xhat weight dy)) rstd,  dweight_j = sum_r dy_rj xhat_rj  (fp32),  xhat = x rstd;
 * partial_ws of hstu_norm_bwd_workspace_bytes(rows, dim) bytes; dweight is summed in a fixed order (no atomics, no locks:
 * bit-identical run to run); rows == 0 launches nothing and zeroes dweight.  dim <= 4096 (rows read in 16-byte pieces) /
 * 2048 (element by element), as hstu_layer_norm_fwd. */
int hstu_rms_norm_fwd(const void* x, const void* weight, void* y, float* rstd, int64_t rows, int32_t dim, float eps,
                      int dtype, void* stream);
int hstu_rms_norm_bwd(const void* dy, const void* x, const void* weight, const float* rstd, void* dx, float* dweight,
                      float* partial_ws, int64_t rows, int32_t dim, int dtype, void* stream);
/* ABI v11: y = x . W^T (+ bias) for a contraction length of 512 -- the same kernel without the LayerNorm (rows of x in
 * registers, W streamed through LDS).  Used for d y = d out . W_out^T in the output stage's backward, where k is the
 * embedding dim and the (n, k) K-contiguous operand is the reference's (3 H d, D) `_output_weight` as stored
 * (dx = torch.mm(dz, w.t()): ops/triton/triton_addmm.py:302-315; caller ops/hstu_compute.py:92-136).  Same shape rule
 * and alignment as hstu_ln_linear_fwd; bias may be NULL. */
int hstu_linear_k512_supported(int64_t rows, int32_t k, int32_t n, int dtype);
int hstu_linear_k512(const void* x, int64_t ldx, const void* w_nk, const void* bias, void* y, int64_t ldy,
                     int64_t rows, int32_t k, int32_t n, int dtype, void* stream);
/* Row-wise e4m3 UVQK projection (additive to ABI v13): the reference's fp8_in_addmm_fwd
 * (ops/cpp/cuda_hstu_preprocess_and_attention.py:75-95,231-245), whose two kernels are outside the open tree.  Arithmetic, with
 * the convention of hstu_jagged_quantize_fp8 (OCP e4m3fn, round to nearest even, IEEE fp32 divisions):
 *   nx = LayerNorm(x) ln_w + ln_b  (fp32, not rounded to the I/O type);  x_scale[r] = max_k |nx[r,k]| / 448  (1 for a zero row);
 *   xq[r,k] = e4m3(clamp(nx[r,k] / x_scale[r], -448, 448));  (wq, w_scale): the (n, k) weight by the same rule, row by row;
 *   y[r,n] = (sum_k xq[r,k] wq[n,k]) x_scale[r] w_scale[n] + bias[n]   (fp32 accumulation, one rounding to the I/O type).
 * A row's result depends on no other row of the call.
 * hstu_quantize_rows_fp8: rows of `src` (bf16 / fp16 / fp32, leading dimension ld in elements) -> dst_q (rows x k bytes,
 *   contiguous) and scale (fp32 per row); k a multiple of 16 up to 4096 (HSTU_EUNSUPPORTED otherwise); src, its rows and dst_q
 *   16-byte aligned.
 * hstu_ln_linear_fp8_fwd: the fused kernel; shape rule and alignment of hstu_ln_linear_fwd (bf16 / fp16, k == 512, n a multiple
 *   of 32 up to 4096: hstu_ln_linear_fp8_supported; HSTU_EUNSUPPORTED otherwise).  wq: n x 512 bytes; bias (I/O type) may be NULL;
 *   xq (rows x 512 bytes), x_scale, mean, rstd (fp32 per row) are optional outputs.
 * hstu_linear_fp8_rowwise: the same kernel without the LayerNorm, on codes and scales (the reference's
 *   fp8_addmm_fwd_rowwise_fused); xq rows x 512 bytes, contiguous. */
int hstu_ln_linear_fp8_supported(int64_t rows, int32_t k, int32_t n, int dtype);
int hstu_quantize_rows_fp8(const void* src, int64_t ld, int64_t rows, int32_t k, int dtype, void* dst_q, float* scale, void* stream);
int hstu_ln_linear_fp8_fwd(const void* x, int64_t ldx, const void* ln_weight, const void* ln_bias, float eps, const void* wq,
                           const float* w_scale, const void* bias, void* y, int64_t ldy, void* xq, float* x_scale, float* mean,
                           float* rstd, int64_t rows, int32_t k, int32_t n, int dtype, void* stream);
int hstu_linear_fp8_rowwise(const void* xq, const float* x_scale, const void* wq, const float* w_scale, const void* bias, void* y,
                            int64_t ldy, int64_t rows, int32_t k, int32_t n, int out_dtype, void* stream);
/* ABI v13: d = a . b + c, row-major, fp32 accumulation, C and D DIFFERENT buffers -- the output stage out = x + y . W_o
 * (`torch.addmm(x, y, output_weight)`, ops/hstu_compute.py:92-136; the reference's own kernel for it: ops/triton/triton_addmm.py:185-340)
 * as ONE hipBLASLt launch.  Through torch.addmm the same product is a copy of x into the result followed by an in-place GEMM with
 * beta = 1 (40 us per layer at 204,800 x 512).  A plain library GEMM: hipBLASLt is looked up at run time (dlopen), nothing links
 * against it; _supported() says whether it was found (else the caller keeps torch.addmm -- the same library behind it).
 * a (m, k) lda, b (k, n) ldb, c (m, n) ldc, d (m, n) ldd: leading dimensions in elements, operands 16-byte aligned, bf16 / fp16;
 * workspace: any size (0 / NULL allowed), handed to hipBLASLt's heuristic as the upper bound. */
int hstu_addmm_residual_supported(void);
int hstu_addmm_residual(const void* c, int64_t ldc, const void* a, int64_t lda, const void* b, int64_t ldb, void* d, int64_t ldd,
                        int64_t m, int32_t n, int32_t k, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int hstu_layer_norm_bwd(const void* dy, const void* x, const void* weight,
                        const float* mean, const float* rstd, void* dx,
                        float* dweight, float* dbias, float* partial_ws,
                        int64_t rows, int32_t dim, int dtype, void* stream);
/* ABI v7: dx = LayerNorm'(dy) + dresidual -- the gradient that reaches x around the norm (the STU layer's residual,
 * stu.py:340-351) added inside the kernel instead of by a separate pass; dresidual (rows, dim) in `dtype`, may be NULL. */
int hstu_layer_norm_bwd_residual(const void* dy, const void* x, const void* weight,
                                 const float* mean, const float* rstd, const void* dresidual,
                                 void* dx, float* dweight, float* dbias, float* partial_ws,
                                 int64_t rows, int32_t dim, int dtype, void* stream);
size_t hstu_norm_bwd_workspace_bytes(int64_t rows, int32_t dim);

/*
 * y = u * Norm(attn) with Norm = LayerNorm over the row or per-head GroupNorm,
 * optionally written as the concatenation [u, attn, y]  (rows, 3*dim).
 * Replaces _ln_mul_dropout_fwd/_bwd and _group_norm_mul_dropout_fwd/_bwd
 * (ops/triton/triton_hstu_linear.py:48-337,570-1036).
 *
 * The _dropout_ entry points (ABI v6) fuse the reference's in-kernel dropout
 * (triton_hstu_linear.py:101-120, 196-215; pt_hstu_linear.py:60-64 drops the concatenated
 * tensor): every element of the (rows, dim | 3 dim) output is zeroed with probability
 * p = round(dropout_ratio * 65536) / 65536 and the survivors are scaled by 1 / (1 - p).
 * The mask is a pure function of (seed, element index): bwd -- and a forward recompute of y --
 * regenerate it from the same seed, nothing is stored.  dropout_ratio == 0 is the plain op.
 * bwd takes dy with respect to the DROPPED output.
 */
int hstu_norm_mul_fwd(const void* attn, const void* u, const void* weight, const void* bias,
                      void* y, float* mean, float* rstd, int64_t rows, int32_t heads,
                      int32_t head_dim, float eps, int group_norm, int concat_ux,
                      int dtype, void* stream);
int hstu_norm_mul_bwd(const void* dy, const void* attn, const void* u, const void* weight,
                      const void* bias, const float* mean, const float* rstd,
                      void* dattn, void* du, float* dweight, float* dbias, float* partial_ws,
                      int64_t rows, int32_t heads, int32_t head_dim, int group_norm,
                      int concat_ux, int dtype, void* stream);
int hstu_norm_mul_dropout_fwd(const void* attn, const void* u, const void* weight,
                              const void* bias, void* y, float* mean, float* rstd, int64_t rows,
                              int32_t heads, int32_t head_dim, float eps, int group_norm,
                              int concat_ux, float dropout_ratio, uint64_t seed, int dtype,
                              void* stream);
int hstu_norm_mul_dropout_bwd(const void* dy, const void* attn, const void* u, const void* weight,
                              const void* bias, const float* mean, const float* rstd,
                              void* dattn, void* du, float* dweight, float* dbias,
                              float* partial_ws, int64_t rows, int32_t heads, int32_t head_dim,
                              int group_norm, int concat_ux, float dropout_ratio, uint64_t seed,
                              int dtype, void* stream);

/* ABI v7: the same with u given by rows `u_row_stride` elements apart and, when u_is_preactivation != 0, as the
 * PRE-activation of SiLU (the u slice of the uvqk buffer): the kernels apply SiLU on the fly, rounded to `dtype` where
 * hstu_silu_fwd would have stored it, and the backward multiplies d u by SiLU' and writes rows `du_row_stride` apart
 * (the u slice of the d uvqk buffer) -- hstu_silu_fwd / hstu_silu_bwd fused away, results bit-identical to the
 * separate calls.  Replaces the F.silu(u) of hstu_compute_uqvk (ops/hstu_compute.py:85) next to
 * _group_norm_mul_dropout_fwd/_bwd inside one STU layer. */
int hstu_norm_mul_silu_fwd(const void* attn, const void* u, int64_t u_row_stride, int u_is_preactivation,
                           const void* weight, const void* bias, void* y, float* mean, float* rstd,
                           int64_t rows, int32_t heads, int32_t head_dim, float eps, int group_norm,
                           int concat_ux, float dropout_ratio, uint64_t seed, int dtype, void* stream);
int hstu_norm_mul_silu_bwd(const void* dy, const void* attn, const void* u, int64_t u_row_stride,
                           int u_is_preactivation, const void* weight, const void* bias,
                           const float* mean, const float* rstd, void* dattn, void* du,
                           int64_t du_row_stride, float* dweight, float* dbias, float* partial_ws,
                           int64_t rows, int32_t heads, int32_t head_dim, int group_norm, int concat_ux,
                           float dropout_ratio, uint64_t seed, int dtype, void* stream);

/* u = silu(u) in place on the leading `u_cols` columns of each row of a
 * (rows, row_stride) matrix, and its backward (du *= silu'(u_pre)); the SiLU-on-u
 * epilogue of hstu_compute_uqvk (ops/hstu_compute.py:85). */
int hstu_silu_fwd(const void* in, void* out, int64_t rows, int32_t cols,
                  int64_t in_row_stride, int64_t out_row_stride, int dtype, void* stream);
int hstu_silu_bwd(const void* dout, const void* in, void* din, int64_t rows, int32_t cols,
                  int64_t dout_row_stride, int64_t in_row_stride, int64_t din_row_stride,
                  int dtype, void* stream);

/* ---- timestamp / position additive encoder (the step before the STU stack) ------------------------------
 * out[row] = alpha * x[row] + pos_w[pos_idx(row)] + ts_w[ts_idx(row)], x / out (sum L, dim) in `dtype`, tables fp32
 * (max_pos_ind, dim) and (>= max_time_bucket + 1, dim); also writes the two int32 table indices of every row (the
 * backward needs them).  Index arithmetic of ops/pytorch/pt_position.py:40-122 (position: bit-exact integers;
 * time: fp32 bucket of query_time - timestamp, time_bucket_fn 0 = sqrt, 1 = log; NB the reference clamps the
 * bucket to ts_embeddings.size(1) - 1, pass that as max_time_bucket).  timestamps (sum L) int64; num_targets may be
 * NULL; seq_offsets / num_targets share `index_dtype`.  Replaces triton_add_timestamp_positional_embeddings
 * (ops/triton/triton_position.py:62-158, 241-337), selected by ops/position.py:38-96. */
int hstu_add_ts_pos_emb_fwd(const void* x, void* out, const void* seq_offsets, const int64_t* timestamps,
                            const void* num_targets, const float* pos_w, const float* ts_w, int32_t* pos_idx,
                            int32_t* ts_idx, int32_t batch, int32_t dim, int32_t max_contextual_seq_len,
                            int32_t max_pos_ind, int32_t max_time_bucket, int32_t interleave_targets,
                            int32_t time_bucket_fn, float alpha, int dtype, int index_dtype, void* stream);
/* table_grad[i, :] = sum over the rows e with idx[e] == i of dout[e, :]  (fp32, (table_rows, dim), zeroed here): the
 * index_select backward of one embedding table.  Rows are grouped by table index inside (a radix sort over the
 * ceil(log2(table_rows)) significant bits, stable: each table row's sum runs in row order), then summed by
 * segment.  `workspace`: device memory, 256-byte aligned, at least hstu_embedding_grad_workspace_bytes(n, table_rows)
 * bytes.  Rows of dout: 16-byte multiples, <= 4 KiB.  0 <= idx[e] < table_rows (not checked).  Replaces
 * _add_embeddings_bwd_kernel and the sort on its host side (ops/triton/triton_position.py:188-238, :339-407). */
int hstu_embedding_grad_workspace_bytes(int64_t n, int32_t table_rows, int64_t* bytes);
int hstu_embedding_grad(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, float* table_grad,
                        void* workspace, int64_t workspace_bytes, int dtype, void* stream);
/* The second half alone, for callers that hold the rows sorted already: table_grad[i, :] = sum over e with
 * sorted_idx[e] == i of dout[sorted_rows[e], :]. */
int hstu_embedding_grad_segment_sum(const void* dout, const int64_t* sorted_rows, const int32_t* sorted_idx, int64_t n,
                                    int32_t dim, int32_t table_rows, float* table_grad, int dtype, void* stream);

/* In-backward sparse row-wise Adagrad of one embedding table (the reference's DLRM-v3 training: RowWiseAdagrad applied
 * in backward, dlrm_v3/train/utils.py:190-227; weight_decay = 0, lr_decay = 0).  For every table row r that occurs in idx,
 * and only for those rows:
 *   G[r, :] = sum over e with idx[e] == r of dout[e, :]   (fp32; duplicates in batch order inside a chunk of 128 sorted
 *             rows -- 32 below 262,144 ids with dim <= 512 --, the pieces of a run that crosses chunks in position order)
 *   momentum1[r] += mean_d(G[r, d]^2);   weight[r, :] -= lr / (sqrt(momentum1[r]) + eps) * G[r, :]
 * in place; every other row of weight (table_rows, dim) fp32 and momentum1 (table_rows) fp32 keeps its bits.  No
 * table-sized temporary, no float atomics, no host synchronisation: results are bit-identical from run to run.  dout
 * (n, dim) in `dtype` (bf16 / fp16 / fp32), rows 16-byte multiples of at most 4 KiB, dout and weight 16-byte aligned;
 * n <= 2^31 - 1, n == 0 touches nothing.  0 <= idx[e] < table_rows is the caller's duty (not checked, as for
 * hstu_embedding_grad).  `workspace`: device memory, 256-byte aligned, at least
 * hstu_embedding_rowwise_adagrad_workspace_bytes(n, table_rows) bytes: O(n) and independent of table_rows and dim -- 8
 * bytes per id for the sorted pairs, the sort's temporary, and two partial sums of the widest row (8 KiB) per 128 ids,
 * i.e. 128 bytes per id. */
int hstu_embedding_rowwise_adagrad_workspace_bytes(int64_t n, int32_t table_rows, int64_t* bytes);
int hstu_embedding_rowwise_adagrad(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows,
                                   float* weight, float* momentum1, float lr, float eps, void* workspace,
                                   int64_t workspace_bytes, int dtype, void* stream);
/* The same update for fp32 gradient rows of up to 2048 columns (8 KiB), the rows hstu_embedding_grad_coalesce writes: G (n, dim)
 * fp32, rows (n) the ids (duplicates are summed in list order, as above).  Everything else, the workspace query included, is
 * hstu_embedding_rowwise_adagrad's with dtype fp32.  The sum of squares of G[r, :] is added in one tree whatever the row
 * layout, so coalescing 16-bit rows and applying them here gives the bits of the one-shot update on the 16-bit rows. */
int hstu_embedding_rowwise_adagrad_coalesced(const float* G, const int32_t* rows, int64_t n, int32_t dim, int32_t table_rows,
                                             float* weight, float* momentum1, float lr, float eps, void* workspace,
                                             int64_t workspace_bytes, void* stream);
/* The same update on a table stored in 16 bits (what the reference's DLRM-v3 configurations declare: data_type = FP16):
 * weight (table_rows, dim) in `weight_dtype` (HSTU_DTYPE_F16 or HSTU_DTYPE_BF16), momentum1 (table_rows) fp32.  A touched row is
 * widened to fp32, updated by exactly the arithmetic above -- for a table holding the same values in fp32,
 * hstu_embedding_rowwise_adagrad[_coalesced] computes the same fp32 row and the same momentum1 bit for bit -- and written
 * back by STOCHASTIC ROUNDING (csrc/stochastic_round.h states the rule): element (r, c) is rounded with the 16 random bits
 * hstu_sr_bits(seed, r, c), a function of the seed, the TABLE row and the column alone, so the result does not depend on
 * the batch order beyond what the sum does, and is bit-identical from run to run.  The caller passes a fresh seed per
 * step.  dim a multiple of 8 and <= 2048; dout (n, dim) in `dtype`: bf16 / fp16 rows, or fp32 rows of up to 8 KiB (both
 * domains of the fp32-table pair above).  Workspace: hstu_embedding_rowwise_adagrad_workspace_bytes. */
int hstu_embedding_rowwise_adagrad_lowp(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows,
                                        void* weight, int weight_dtype, float* momentum1, float lr, float eps, uint64_t seed,
                                        void* workspace, int64_t workspace_bytes, int dtype, void* stream);
/* dst[i, c] = the stochastic rounding of src[i, c] to `dst_dtype` (HSTU_DTYPE_F16 or HSTU_DTYPE_BF16) with the random bits
 * hstu_sr_bits(seed, row_ids ? row_ids[i] : i, c): the cast of an fp32 table or checkpoint to a 16-bit one, and the rule of
 * the update above on its own.  src (n, dim) fp32, dst (n, dim), any dim >= 1 (16-byte pieces when dim is a multiple of 8
 * and both are 16-byte aligned); row_ids (n) int32 or NULL; n == 0 touches nothing. */
int hstu_stochastic_round(const float* src, const int32_t* row_ids, void* dst, int64_t n, int32_t dim, int dst_dtype,
                          uint64_t seed, void* stream);
/* In-backward sparse SGD and sparse Adam on the same segment walk (the other two choices of the reference's
 * sparse_optimizer_factory_and_class, dlrm_v3/train/utils.py:169-206; weight_decay = 0, SGD momentum = 0, no amsgrad).
 * G[r, :] is the sum above, addition for addition.  For every table row r that occurs in idx, and only for those rows:
 *   SGD:   weight[r, :] -= lr * G[r, :]                                          (no state)
 *   Adam:  exp_avg[r, :]    = beta1 * exp_avg[r, :]    + (1 - beta1) * G[r, :]
 *          exp_avg_sq[r, :] = beta2 * exp_avg_sq[r, :] + (1 - beta2) * G[r, :]^2
 *          weight[r, :] -= (lr / bc1) * exp_avg[r, :] / (sqrt(exp_avg_sq[r, :]) / sqrt(bc2) + eps)
 *          with t = step + 1, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t formed on the host in double and rounded to fp32:
 *          torch.optim.Adam's arithmetic (amsgrad off), applied LAZILY -- rows outside the batch do not decay (what
 *          fbgemm's in-backward ADAM and torch.optim.SparseAdam do; eps is placed as in torch.optim.Adam, not SparseAdam).
 * in place; every other row of weight and of exp_avg / exp_avg_sq (both (table_rows, dim) fp32) keeps its bits.  `step` >= 0
 * is the caller's count of updates applied before this one; 0 <= beta1, beta2 < 1.  weight (table_rows, dim) in
 * `weight_dtype`: HSTU_DTYPE_F32, or HSTU_DTYPE_F16 / HSTU_DTYPE_BF16 (dim a multiple of 8) -- then the row is widened, updated by
 * exactly the fp32 table's arithmetic (the same fp32 row, exp_avg and exp_avg_sq bit for bit) and written back by the
 * stochastic rounding of hstu_embedding_rowwise_adagrad_lowp with `seed`; `seed` is read only for 16-bit tables.  dout
 * (n, dim) in `dtype`: bf16 / fp16 rows of at most 4 KiB, or fp32 rows of at most 8 KiB (dim <= 2048), so one entry also takes
 * the coalesced lists of replicated tables.  Alignment, n, idx and the guarantees (no float atomics, no table-sized
 * temporary, bit-identical from run to run) are hstu_embedding_rowwise_adagrad's.  Workspace:
 * hstu_embedding_rowwise_adagrad_workspace_bytes -- the layout is the same. */
int hstu_embedding_sparse_sgd(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, void* weight,
                              int weight_dtype, float lr, uint64_t seed, void* workspace, int64_t workspace_bytes, int dtype,
                              void* stream);
int hstu_embedding_sparse_adam(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, void* weight,
                               int weight_dtype, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                               float eps, int64_t step, uint64_t seed, void* workspace, int64_t workspace_bytes, int dtype,
                               void* stream);
/* The first half of that update alone, for data-parallel ranks that exchange their row gradients before applying them:
 * the batch's (idx, dout) coalesced to one fp32 row per distinct id.
 *   rows[s]  = the s-th smallest distinct id of idx (ascending), s < u = *count
 *   G[s, :]  = scale * (sum over e with idx[e] == rows[s] of dout[e, :])   (fp32; the sum is hstu_embedding_rowwise_adagrad's
 *              for the same (idx, dout, dim, dtype), addition for addition; the multiply is applied once, last)
 *   *count   = u, one int32 in device memory
 * rows (n) int32 and G (n, dim) fp32 have room for n entries; only the first u are written, the rest keeps its bits.
 * n == 0 writes *count = 0 and nothing else.  Same limits and guarantees as the update: dim <= 2048, dout rows 16-byte
 * multiples of at most 4 KiB, dout and G 16-byte aligned, n <= 2^31 - 1, 0 <= idx[e] < table_rows not checked; no float
 * atomics, no host synchronisation, bit-identical from run to run.  `workspace`: device memory, 256-byte aligned, at least
 * hstu_embedding_grad_coalesce_workspace_bytes(n, table_rows) bytes: the update's plus 4 bytes per id for the segments'
 * slots (a scan over the segment-head flags of the sorted ids) -- O(n), independent of table_rows and dim. */
int hstu_embedding_grad_coalesce_workspace_bytes(int64_t n, int32_t table_rows, int64_t* bytes);
int hstu_embedding_grad_coalesce(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, float scale,
                                 int32_t* rows, float* G, int32_t* count, void* workspace, int64_t workspace_bytes, int dtype,
                                 void* stream);

/* ---- output postprocessor: row L2 normalisation ---------------------------------------------------------
 * y = x / max(||x||_2, eps) per row of (rows, dim), and its backward.  Replaces L2NormPostprocessor.forward
 * (modules/postprocessors.py:55-69: seq / linalg.norm(seq, dim=-1).clamp(min=1e-6)) and its autograd. */
int hstu_l2_norm_fwd(const void* x, void* y, int64_t rows, int32_t dim, float eps, int dtype, void* stream);
int hstu_l2_norm_bwd(const void* dy, const void* x, void* dx, int64_t rows, int32_t dim, float eps, int dtype,
                     void* stream);

/* ---- sampled-softmax loss, dot-product similarity --------------------------------------
 * Per supervision row i (n_rows of them):
 *   l_i0 = <q_i, P(pos_emb_i)> / T,  l_ik = <q_i, N(table[neg_rows[i,k]])> / T  for k < num_negatives,
 *   l_ik = -5e4 where neg_ids[i,k] == pos_ids[i];  row_loss_i = logsumexp_k(l_i0, l_i1 ..) - l_i0,  lse_i = that logsumexp;
 *   P / N = x / max(||x||_2, eps) when pos_l2_norm / table_l2_norm, identity otherwise.
 * Replaces SampledSoftmaxLoss.jagged_forward (research/modeling/sequential/losses/sampled_softmax.py:44-95) with the
 * DotProductSimilarity (research/rails/similarities/dot_product_similarity_fn.py:38-62): the caller reduces
 * sum_i w_i row_loss_i / sum_i w_i.  neg_rows index `table`; neg_ids are the item ids of those rows: the same matrix
 * for LocalNegativesSampler (autoregressive_losses.py:112-131: table = the item embedding weight, pos/table l2 norm =
 * the sampler's l2_norm), `cached_ids[offsets]` for InBatchNegativesSampler (:186-204: table = its cached, already
 * normalised embeddings, table_l2_norm = 0).  q, pos_emb, table: (., dim) in `dtype`, rows 16-byte aligned
 * (dim a multiple of 4 for fp32 / 8 for 16-bit, dim * elt <= 1024 bytes); ids int64; row_loss, lse fp32 (n_rows).
 * Indices outside [0, table_rows) are clamped (memory safety only). */
int hstu_sampled_softmax_fwd(const void* q, int64_t q_row_stride, const void* pos_emb, int64_t pos_row_stride,
                             const int64_t* pos_ids, const int64_t* neg_rows, const int64_t* neg_ids, const void* table,
                             int64_t table_row_stride, int64_t table_rows, int64_t n_rows, int32_t num_negatives,
                             int32_t dim, float temperature, int32_t pos_l2_norm, int32_t table_l2_norm, float eps,
                             float* row_loss, float* lse, int dtype, void* stream);
/* Gradients of sum_i grad_row_loss[i] * row_loss_i: dq, dpos_emb (n_rows, dim) in `dtype` (every row written; rows
 * with grad_row_loss == 0 get zeros and gather nothing), dtable (table_rows, dim) fp32 contiguous, ACCUMULATED into
 * (zero it first) with atomics -- the one sum of this op whose order is not fixed.  A masked negative passes no
 * gradient (torch.where picks the constant, sampled_softmax.py:78-82). */
int hstu_sampled_softmax_bwd(const void* q, int64_t q_row_stride, const void* pos_emb, int64_t pos_row_stride,
                             const int64_t* pos_ids, const int64_t* neg_rows, const int64_t* neg_ids, const void* table,
                             int64_t table_row_stride, int64_t table_rows, int64_t n_rows, int32_t num_negatives,
                             int32_t dim, float temperature, int32_t pos_l2_norm, int32_t table_l2_norm, float eps,
                             const float* lse, const float* grad_row_loss, void* dq, int64_t dq_row_stride, void* dpos_emb,
                             int64_t dpos_row_stride, float* dtable, int dtype, void* stream);

/* ---- ABI v10: the glue around the projections of an STU layer ---------------------------------------------
 * hstu_cast_params: up to HSTU_CAST_MAX_ITEMS fp32 tensors -> bf16 / fp16 in ONE launch; an item with transpose != 0 is a
 * (rows, cols) row-major matrix written as its (cols, rows) transpose (the UVQK weight's K-contiguous copy).  Replaces the
 * per-parameter ``.to(x.dtype)`` casts the reference issues in front of every projection (ops/hstu_compute.py:62-72,
 * ops/triton/triton_hstu_linear.py:1160-1170; ops/triton/triton_hstu_preprocess_and_attention.py:60-75). */
#define HSTU_CAST_MAX_ITEMS 8
typedef struct HstuCastItem {
  const float* src;
  void* dst;
  int64_t numel;
  int32_t rows, cols;     /* only read when transpose != 0: rows * cols == numel */
  int32_t transpose;
} HstuCastItem;
int hstu_cast_params(const HstuCastItem* items, int32_t n_items, int dst_dtype, void* stream);
/* out[c] = sum over r < rows of x[r * ldx + c] (fp32, fixed summation order: bit-identical run to run) for a bf16 / fp16
 * matrix -- the bias gradient of a projection (ops/triton/triton_addmm.py:309 ``torch.sum(dz, dim=0)``; d uvqk_beta in
 * ops/triton/triton_hstu_preprocess_and_attention.py:122-293).  cols and ldx multiples of 8, x 16-byte aligned;
 * `workspace`: hstu_column_sum_workspace_bytes(rows, cols) bytes of device memory, 16-byte aligned. */
size_t hstu_column_sum_workspace_bytes(int64_t rows, int32_t cols);
int hstu_column_sum(const void* x, int64_t ldx, int64_t rows, int32_t cols, float* out, void* workspace, int dtype,
                    void* stream);
/* Calibration streams for bench.py (no reference counterpart; measurement only): `iters` x 16 independent 32x32x16 bf16
 * MFMAs per wave, two waves per SIMD on every CU, no memory traffic (*flops = the FLOP the launch performs), and a
 * non-temporal 16-byte-per-lane read of `bytes` bytes without arithmetic.  What this box sustains for the two resources the
 * product kernels are priced against, measured in the same process as they are. */
int hstu_calib_mfma_stream(int32_t iters, float* sink, double* flops, void* stream);
int hstu_calib_read_stream(const void* src, size_t bytes, float* sink, void* stream);

/* ---- jagged_dense_bmm_broadcast_add: a per-user GEMM along the offset vector ------------------------------
 * For user b with rows [s, e) = [seq_offsets[b], seq_offsets[b+1]):
 *   out[s:e] = jagged[s:e] @ dense[b] + bias[b]      fp32 accumulation, one rounding to `dtype`
 * Replaces jagged_dense_bmm_broadcast_add (ops/jagged_tensors.py:210-253; ops/pytorch/pt_jagged.py:77-98, a padded
 * torch.bmm; ops/triton/triton_jagged.py:61-142 and the autograd node :524-632).  jagged (total_rows, K) and out
 * (total_rows, N) in `dtype` with a row stride in elements and unit column stride; dense (batch, K, N) in `dtype`
 * through three strides, one of dense_k_stride / dense_n_stride being 1 (both storage orders give bit-identical
 * results); bias (batch, N) fp32, or NULL for no bias.  The DATA GRADIENT is the same call with d_out as `jagged`,
 * dense's K / N strides (and k / n) swapped and bias = NULL (triton_jagged.py:588-605).  k and n are multiples of 16
 * bytes, every row starts 16-byte aligned (zero-pad what is not).  Rows come from the offsets, not from a max_seq_len:
 * there is none.  `workspace`: hstu_jagged_dense_bmm_workspace_bytes(batch) bytes of device memory (the users' tile
 * offsets, int32).  Offsets are clamped to [0, total_rows].  batch == 0 or total_rows == 0 returns without a launch. */
size_t hstu_jagged_dense_bmm_workspace_bytes(int32_t batch);
int hstu_jagged_dense_bmm_fwd(const void* jagged, int64_t jagged_row_stride, const void* dense, int64_t dense_batch_stride,
                              int64_t dense_k_stride, int64_t dense_n_stride, const float* bias, int64_t bias_batch_stride,
                              void* out, int64_t out_row_stride, const void* seq_offsets, int64_t total_rows, int32_t batch,
                              int32_t k, int32_t n, void* workspace, int dtype, int index_dtype, void* stream);
/* d_dense[b] = jagged[s:e]^T @ d_out[s:e] in `dtype` (batch and K strides in elements, N contiguous) and, when d_bias is
 * not NULL, d_bias[b] = the column sums of d_out[s:e] in fp32 (triton_jagged.py:145-240, which folds the bias reduction
 * into the weight gradient as this does).  Every slab and row is written, zeros for an empty user.  Each sum runs in a
 * fixed order in fp32 registers: no atomics, no workspace, bit-identical run to run.  Alignment as above. */
int hstu_jagged_dense_bmm_wgrad(const void* jagged, int64_t jagged_row_stride, const void* d_out, int64_t d_out_row_stride,
                                void* d_dense, int64_t d_dense_batch_stride, int64_t d_dense_k_stride, float* d_bias,
                                int64_t d_bias_batch_stride, const void* seq_offsets, int64_t total_rows, int32_t batch, int32_t k,
                                int32_t n, int dtype, int index_dtype, void* stream);

/* ---- fused MIPS top-k: the k best items of a table per query, no (batch, num_items) score matrix ----------
 * For every query row b: the k items x with the largest <queries[b], items[x]> (fp32 accumulation), sorted by score
 * descending, then item index ascending; -0.0 and +0.0 are one score.  Replaces MIPSBruteForceTopK.forward
 * (research/rails/indexing/mips_top_k.py:68-81: torch.mm + torch.topk, whose tie order is unspecified).  queries
 * (batch, dim) and items (num_items, dim) in `dtype` with row strides in elements and unit column stride; dim a
 * multiple of 16 bytes and at most 512, rows 16-byte aligned (zero-pad what is not).  out_scores (batch, k) contiguous
 * in `dtype` (the fp32 score, rounded once), out_indices (batch, k) contiguous int32 positions into the table.
 * 1 <= k <= min(num_items, 4096), num_items < 2^31.  `workspace`: hstu_mips_topk_workspace_bytes(batch, k) bytes of
 * device memory, 16-byte aligned -- O(batch * (256 + k)), by construction independent of num_items.  A fixed launch
 * sequence without a host sync; integer atomics only: bit-identical run to run.  batch == 0 returns without a launch. */
size_t hstu_mips_topk_workspace_bytes(int32_t batch, int32_t k);
int hstu_mips_topk(const void* queries, int64_t q_row_stride, const void* items, int64_t item_row_stride, void* out_scores,
                   int32_t* out_indices, void* workspace, int32_t batch, int32_t num_items, int32_t dim, int32_t k, int dtype,
                   void* stream);

/* ---- Mixture-of-Logits scores: every (query, item) pair against a shared table, no (batch, num_items, L) tensor ----
 * With L = pq * px, for every query b and item x (fp32 accumulation and intermediates):
 *   l[n px + m] = <qc[b, n, :], xc[x, m, :]> * inv_temperature            (the reference's "bxnm" reshape order)
 *   t           = w2 silu(w1 l + b1) + b2        hidden > 0: w1 (hidden, L), b1 (hidden), w2 (L, hidden), b2 (L)
 *               = w1 l + b2                      hidden == 0: w1 (L, L), b2 (L); b1 and w2 are not read
 *   g           = gq[b] * gi[x] + t
 *   w           = g sigmoid(g)                   combination HSTU_MOL_GLU_SILU
 *               = g sigmoid(layer_norm(g))       combination HSTU_MOL_GLU_SILU_LN (no affine, eps 1e-5)
 *   out[b, x]   = sum_j softmax(w)_j l_j
 * Replaces MoLSimilarity.forward + MoLGatingFn.forward + SoftmaxDropoutCombiner in eval mode for a shared item table
 * (research/rails/similarities/mol/similarity_fn.py:363-387, :151-204, :35-49), which materialise the (B, X, L) logits
 * and the (B, X, hidden) layer.  qc (batch, pq, dim), xc (num_items, px, dim), gq (batch, L), gi (num_items, L) and the
 * weights: contiguous, all in `dtype` (bf16, fp16, fp32); qc and xc 16-byte aligned.  out (batch, num_items) contiguous
 * fp32, addressed in 64 bits.  fp32 operands use the exact fp32 MFMA; 16-bit operands are rounded to `dtype` where an MFMA
 * reads them.  No atomics: bit-identical run to run.  HSTU_EUNSUPPORTED before any launch unless 1 <= pq, px and
 * L <= HSTU_MOL_MAX_LOGITS, 1 <= dim <= HSTU_MOL_MAX_DIM with dim a multiple of 8 (zero-pad it: a dot product does not
 * change), 0 <= hidden <= HSTU_MOL_MAX_HIDDEN.  batch, num_items < 2^31 (a batch above 4 * 2^20 queries runs as several
 * launches on `stream`); either == 0 returns without a launch. */
#define HSTU_MOL_MAX_LOGITS 64
#define HSTU_MOL_MAX_DIM 128
#define HSTU_MOL_MAX_HIDDEN 256
#define HSTU_MOL_GLU_SILU 0
#define HSTU_MOL_GLU_SILU_LN 1
int hstu_mol_scores(const void* qc, const void* xc, const void* gq, const void* gi, const void* w1, const void* b1, const void* w2,
                    const void* b2, float* out, int32_t batch, int32_t num_items, int32_t pq, int32_t px, int32_t dim,
                    int32_t hidden, float inv_temperature, int combination, int dtype, void* stream);

/* ---- multitask prediction head: SwishLayerNorm + task projection + predictions + task losses in one row pass ----
 * Per row l of x (rows, dim; `dtype`, row stride in elements, unit column stride), fp32 math throughout:
 *   y = x * sigmoid(LayerNorm(x) ln_weight + ln_bias)                  (never written to memory)
 *   logits[t, l] = <y, w[t]> + c[t]                                    w (num_tasks, dim), c (num_tasks): fp32
 *   preds[t, l]  = sigmoid(logits[t, l]) for t < num_binary (the binary tasks come first), logits[t, l] otherwise
 *   loss[t] = sum_l weights[t, l] * (max(z, 0) - z label + log1p(exp(-|z|)) | (z - label)^2)
 *             / max(weight_sum[t], 1) * loss_scale,   weight_sum[t] = sum_l weights[t, l]
 * Replaces everything behind the first projection of DefaultMultitaskModule (modules/multitask_module.py:70-104 predictions,
 * :107-133 labels and weights, :136-191 losses, :233-277 forward) with the prediction module of modules/dlrm_hstu.py:139-149
 * (Linear -> SwishLayerNorm -> Linear): ops/layer_norm.py:79-112 + torch.nn.Linear + the (T, L) torch ops.
 * logits, preds, labels, weights: (num_tasks, rows) fp32 contiguous; mean, rstd (rows) fp32 (outputs of the forward, may be
 * NULL; inputs of the backward); loss, weight_sum (num_tasks) fp32.  ln_weight / ln_bias in `dtype`, as
 * hstu_swish_layer_norm_fwd takes them, and with its dim limits (4096 for rows of 16-byte pieces, 2048 otherwise).
 * weights == NULL: all ones.  labels == NULL (inference): only logits (may be NULL), preds, mean, rstd are written.
 * Sums over rows run in a fixed order (per-workgroup partials in `workspace`, then a finish kernel): no float atomics,
 * bit-identical run to run.  `workspace`: hstu_multitask_head_workspace_bytes(dim, num_tasks) bytes of device memory,
 * 16-byte aligned, independent of rows.  rows == 0 zeroes loss / weight_sum and launches nothing. */
#define HSTU_MULTITASK_MAX_TASKS 8
#define HSTU_MULTITASK_MAX_BLOCKS 1024      /* grid cap of the row kernels (they loop over rows beyond it) ... */
#define HSTU_MULTITASK_ROWS_PER_BLOCK 4     /* ... and the rows a workgroup works on at once (one per wavefront) */
size_t hstu_multitask_head_workspace_bytes(int32_t dim, int32_t num_tasks);
int hstu_multitask_head_fwd(const void* x, int64_t x_row_stride, const void* ln_weight, const void* ln_bias, float eps,
                            const float* w, const float* c, const float* labels, const float* weights, float* logits,
                            float* preds, float* mean, float* rstd, float* loss, float* weight_sum, void* workspace,
                            int64_t rows, int32_t dim, int32_t num_tasks, int32_t num_binary, float loss_scale, int dtype,
                            void* stream);
/* Gradients of sum_t grad_loss[t] loss[t] + sum_{t,l} grad_pred[t, l] preds[t, l] (either may be NULL):
 *   d logits[t, l] = grad_loss[t] loss_scale weights[t, l] / max(weight_sum[t], 1) * (sigmoid(z) - label | 2 (z - label))
 *                    + grad_pred[t, l] * (p (1 - p) | 1)
 * then y is recomputed, d y = sum_t d logits[t] w[t] goes through the SwishLayerNorm backward into dx (`dtype`, row
 * stride in elements), and dw (num_tasks, dim), dc (num_tasks), dln_weight, dln_bias (dim) are accumulated in fp32 in a
 * fixed order.  logits / mean / rstd / weight_sum as the forward wrote them.  rows == 0 zeroes the four reduced outputs. */
int hstu_multitask_head_bwd(const float* grad_loss, const float* grad_pred, const void* x, int64_t x_row_stride,
                            const void* ln_weight, const void* ln_bias, const float* w, const float* labels, const float* weights,
                            const float* logits, const float* mean, const float* rstd, const float* weight_sum, void* dx,
                            int64_t dx_row_stride, float* dw, float* dc, float* dln_weight, float* dln_bias, void* workspace,
                            int64_t rows, int32_t dim, int32_t num_tasks, int32_t num_binary, float loss_scale, int dtype,
                            void* stream);

/* ---- input preprocessors: the action encoder and the content / action / contextual combine as two row passes ----
 * Action encode (ActionEncoder.forward, modules/action_encoder.py:73-112).  User b owns the UIH rows
 * [uih_offsets[b], uih_offsets[b+1]) of `actions` / `watchtimes` (int64) and target_offsets[b+1] - target_offsets[b]
 * target rows; its output rows start at uih_offsets[b] + target_offsets[b], UIH rows first.  For UIH row r
 *   a = actions[r] | OR_k (watchtimes[r] >= thresholds[k] ? threshold_weights[k] : 0)
 * and column block t (embedding_dim columns) of the output row is table[t, :] when (a & weights[t]) > 0 and 0 * table[t, :]
 * otherwise (the reference multiplies the boolean into the table: a zero that keeps the parameter's sign); a target row
 * is target_table.  table (num_types, embedding_dim) and target_table (num_types * embedding_dim)
 * are fp32 device tensors, the output (total_uih_len + total_targets, num_types * embedding_dim) is contiguous in `dtype`
 * (bf16 / fp16 / fp32): every value is a parameter rounded once, or zero.  weights (num_types <= 64), thresholds and
 * threshold_weights (num_thresholds <= 64; watchtimes may be NULL without thresholds) are HOST arrays that travel as
 * kernel arguments.  Offsets int32 or int64 (`index_dtype`).  Replaces two torch bit ops, a (rows, T, Da) fp32 product, a
 * tile, a cast and concat_2D_jagged.  batch == 0 or no rows: returns without a launch.  No host synchronisation. */
#define HSTU_ACTION_ENCODE_MAX_TYPES 64
int hstu_action_encode_fwd(const int64_t* actions, const int64_t* watchtimes, const void* uih_offsets,
                           const void* target_offsets, const float* table, const float* target_table, const int64_t* weights,
                           int32_t num_types, const int64_t* thresholds, const int64_t* threshold_weights,
                           int32_t num_thresholds, void* out, int64_t total_uih_len, int64_t total_targets, int32_t batch,
                           int32_t embedding_dim, int dtype, int index_dtype, void* stream);
/* d_table[t, c] = the sum of d_out[row, t * embedding_dim + c] over the UIH rows whose bit t is set, d_target_table[c'] =
 * the sum of d_out[row, c'] over the target rows; fp32, fixed order (per-workgroup partials over fixed row slabs in
 * `workspace`, then one sum over the workgroups): no float atomics, bit-identical run to run.  `workspace`:
 * hstu_action_encode_bwd_workspace_bytes(rows, num_types * embedding_dim) bytes of device memory, 16-byte aligned.
 * No rows: both gradients are zeroed. */
size_t hstu_action_encode_bwd_workspace_bytes(int64_t total_rows, int32_t width);
int hstu_action_encode_bwd(const void* d_out, const int64_t* actions, const int64_t* watchtimes, const void* uih_offsets,
                           const void* target_offsets, const int64_t* weights, int32_t num_types, const int64_t* thresholds,
                           const int64_t* threshold_weights, int32_t num_thresholds, float* d_table, float* d_target_table,
                           void* workspace, int64_t total_uih_len, int64_t total_targets, int32_t batch, int32_t embedding_dim,
                           int dtype, int index_dtype, void* stream);
/* Combine (ContextualInterleavePreprocessor.combine_embeddings, modules/contextual_interleave_preprocessor.py:101-224).
 * User b has L = seq_offsets[b+1] - seq_offsets[b] rows of content / action (total, dim), T = num_targets[b] of them
 * targets (the last ones), U = L - T.  Its output rows start at out_offsets[b]; row j is contextual[b, j] with timestamp 0
 * for j < contextual_len, and with p = j - contextual_len, o = seq_offsets[b]:
 *   HSTU_COMBINE_SUM              content[o + p] + action[o + p] (fp32 add, one rounding; content alone when action is
 *                                 NULL); contextual_len + L rows
 *   HSTU_COMBINE_INTERLEAVE_ALL   row p >> 1 of content (p even) or action (p odd); contextual_len + 2 L rows
 *   HSTU_COMBINE_INTERLEAVE_UIH   the same for p < 2 U, then content[o + U + (p - 2 U)]; contextual_len + 2 L - T rows
 * and the timestamp (int64) of the source row.  out_offsets is the complete cumsum of those lengths, computed by the
 * caller (hstu_complete_cumsum); the number of output rows follows from total_uih_len, total_targets, batch and
 * contextual_len on the host.  num_targets (same integer type as the offsets) is read for INTERLEAVE_UIH only.  Replaces
 * stack + mask + dense_to_jagged + boolean indexing (a host sync) + two concat_2D_jagged.  Bit-exact; no host sync. */
#define HSTU_COMBINE_SUM 0
#define HSTU_COMBINE_INTERLEAVE_ALL 1
#define HSTU_COMBINE_INTERLEAVE_UIH 2
int hstu_combine_embeddings_fwd(const void* content, const void* action, const void* contextual, const int64_t* timestamps,
                                const void* seq_offsets, const void* num_targets, const void* out_offsets, void* out,
                                int64_t* out_timestamps, int64_t total_uih_len, int64_t total_targets, int32_t batch,
                                int32_t contextual_len, int32_t dim, int mode, int dtype, int index_dtype, void* stream);
/* The inverse gather: every content / action / contextual row reads the one output row that copied it (SUM: content and
 * action the same row; INTERLEAVE_UIH: the target rows of d_action are zeroed).  d_action / d_contextual may be NULL.  No
 * atomics, no workspace, bit-exact. */
int hstu_combine_embeddings_bwd(const void* d_out, const void* seq_offsets, const void* num_targets, const void* out_offsets,
                                void* d_content, void* d_action, void* d_contextual, int64_t total_uih_len,
                                int64_t total_targets, int32_t batch, int32_t contextual_len, int32_t dim, int mode, int dtype,
                                int index_dtype, void* stream);

/* ---- TimestampLayerNormPostprocessor behind its GEMM: time features + rank-2F update + bias + LayerNorm in one row pass ----
 * The postprocessor DlrmHSTU builds (modules/dlrm_hstu.py:182-191, modules/postprocessors.py:105-176) concatenates 2F time
 * features onto every D-wide row, runs Linear(D + 2F, D) and a LayerNorm.  With the combiner weight split W = [Wx | Wt] the
 * GEMM is the aligned z0 = x Wx^T (hstu_linear_k512 at D = 512) and the rest is one row pass over z0.
 * Time features (postprocessors.py:133-165, the reference's fp32 arithmetic, NOT integer arithmetic): for period p
 *   a = (float)t;  units = torch.div(a, period_units[p], rounding_mode="floor")   (fmod-based, IEEE divides)
 *   angle = ((torch.remainder(units, units_per_period[p]) / units_per_period[p]) * 2) * 3.14
 *   features [2p, 2p + 1] = [cos(angle), sin(angle)]
 * period_units, units_per_period: (num_periods) fp32 DEVICE arrays (the module's buffers).  1 <= num_periods <= 4 for the
 * fused row pass; hstu_time_features alone (the unfused composition, any module) takes up to 1024.
 * hstu_time_features writes out (rows, 2 num_periods) fp32 contiguous; timestamps (rows) int64.  rows == 0: no launch. */
#define HSTU_TIME_LN_MAX_PERIODS 4
#define HSTU_TIME_FEATURES_MAX_PERIODS 1024
#define HSTU_TIME_LN_MAX_BLOCKS 1024        /* grid cap of the row kernels (they loop over rows beyond it) */
int hstu_time_features(const int64_t* timestamps, const float* period_units, const float* units_per_period, int32_t num_periods,
                       float* out, int64_t rows, void* stream);
/* Per row l of z0 (rows, dim; contiguous, `dtype`: the GEMM's output), fp32 math throughout:
 *   z = z0 + b + sum_j tf_j(timestamps[l]) wt[j, :]          (never written to memory)
 *   y = (z - mean) rstd ln_weight + ln_bias                   y (rows, dim) contiguous in `dtype`
 * b, ln_weight, ln_bias (dim) and wt (2 num_periods, dim; the transposed time columns of W) are fp32 contiguous; mean, rstd
 * (rows) fp32, may be NULL.  Rows are read in 16-byte pieces when dim and every pointer allow it, element by element
 * otherwise; dim <= 4096 (pieces) / 2048 (elements), as hstu_layer_norm_fwd.  rows == 0 launches nothing. */
int hstu_time_ln_fwd(const void* z0, const int64_t* timestamps, const float* period_units, const float* units_per_period,
                     int32_t num_periods, const float* b, const float* wt, const float* ln_weight, const float* ln_bias, float eps,
                     void* y, float* mean, float* rstd, int64_t rows, int32_t dim, int dtype, void* stream);
/* z is recomputed from z0 and the timestamps; with xhat = (z - mean) rstd and g = dy ln_weight
 *   dz = rstd (g - mean_c(g) - xhat mean_c(g xhat))          dz (rows, dim) in `dtype`: feeds the two GEMM gradients
 *   dln_weight = sum_l dy xhat, dln_bias = sum_l dy, db = sum_l dz (dim), dwt[j] = sum_l tf_j dz (2 num_periods, dim): fp32
 * The 3 + 2 num_periods column sums run in a fixed order (per-workgroup partials in `workspace`, then a finish kernel): no
 * float atomics, bit-identical run to run.  `workspace`: hstu_time_ln_workspace_bytes(dim, num_periods) bytes of device
 * memory, 16-byte aligned, independent of rows.  rows == 0 zeroes the four reduced outputs and launches nothing. */
size_t hstu_time_ln_workspace_bytes(int32_t dim, int32_t num_periods);
int hstu_time_ln_bwd(const void* dy, const void* z0, const int64_t* timestamps, const float* period_units,
                     const float* units_per_period, int32_t num_periods, const float* b, const float* wt, const float* ln_weight,
                     const float* mean, const float* rstd, void* dz, float* dln_weight, float* dln_bias, float* db, float* dwt,
                     void* workspace, int64_t rows, int32_t dim, int dtype, void* stream);

/* ---- jagged causal softmax attention (the SASRec baseline's attention) -----------------------------------------------------
 * What research/modeling/sequential/sasrec.py:209-214 runs through torch.nn.MultiheadAttention on a padded (B, N, D) batch
 * with an (N, N) mask, on jagged rows: row i of user b sees rows j <= i of user b,
 *   S[i,j] = scale <q_i, k_j>,  P = softmax_j(S),  O = dropout_p(P) V,  lse[i] = ln sum_j exp(S[i,j])   (un-dropped scores)
 * No (N, N) object exists in memory.  q, k, v: (total_rows, heads, head_dim) in `dtype` with row / head strides in ELEMENTS
 * (k and v may be column slices of one GEMM output); every (row, head) vector 16-byte aligned, so head_dim is a multiple
 * of 16 bytes (zero-pad it; `scale` is the caller's, usually real_head_dim^-0.5).  out, dout, dq, dk, dv are contiguous
 * (total_rows, heads, head_dim) in `dtype`; lse and delta are contiguous (total_rows, heads) fp32.  Users longer than
 * max_seq_len are a caller error (their rows past it are not written).
 * Fused range (hstu_softmax_attn_supported returns 1): bf16 / fp16 / fp32, 1 <= head_dim <= 64, 1 <= max_seq_len <= 512.
 * Dropout: 0 <= dropout_p < 1; element (row r, head h, key position j inside its user) has the index
 * e = (r heads + h) max_seq_len + j of the generator of hstu_norm_mul_dropout_fwd (same threshold, survivor scale and pair
 * rule); the backward regenerates the mask from `seed`.  batch == 0 or total_rows == 0 launches nothing. */
#define HSTU_SOFTMAX_ATTN_MAX_HEAD_DIM 64
#define HSTU_SOFTMAX_ATTN_MAX_SEQ_LEN 512
int hstu_softmax_attn_supported(int dtype, int32_t head_dim, int32_t max_seq_len);
int hstu_softmax_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k, int64_t k_row_stride,
                          int64_t k_head_stride, const void* v, int64_t v_row_stride, int64_t v_head_stride, void* out, float* lse,
                          const void* seq_offsets, int64_t total_rows, int32_t batch, int32_t heads, int32_t head_dim,
                          int32_t max_seq_len, float scale, float dropout_p, uint64_t seed, int dtype, int index_dtype,
                          void* stream);
/* P is recomputed from q, k and lse; delta = rowsum(dout * out) is written to `delta` (scratch of the call) by the dQ kernel
 * and read by the dK / dV kernel; dS = P (dP - delta).  Every dq / dk / dv row is owned by one wavefront: no float atomics,
 * bit-identical run to run. */
int hstu_softmax_attn_bwd(const void* dout, const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k,
                          int64_t k_row_stride, int64_t k_head_stride, const void* v, int64_t v_row_stride, int64_t v_head_stride,
                          const void* out, const float* lse, float* delta, void* dq, void* dk, void* dv, const void* seq_offsets,
                          int64_t total_rows, int32_t batch, int32_t heads, int32_t head_dim, int32_t max_seq_len, float scale,
                          float dropout_p, uint64_t seed, int dtype, int index_dtype, void* stream);

/* The input-feature preprocessors of the research path (research/modeling/sequential/input_features_preprocessors.py) as
 * one row pass.  past_ids (batch, n) int64, past_embeddings (batch, n, item_dim) in `emb_dtype`, ratings (batch, n) int32 /
 * int64 (`rating_index_dtype`; rated layouts only), pos_table (num_positions, Do) and rating_table (num_ratings, rating_dim)
 * in `out_dtype`.  With s = fl32(Do ** 0.5) and m(b, i) = past_ids[b, i] != 0 (by id, not by length):
 *   out[b, n', c] = m * drop(src(b, n', c) * s + pos_table[n', c]),  valid_mask[b, n'] = m  (fp32 whatever the dtypes)
 *   HSTU_PREPROCESS_PLAIN       Do = item_dim, N' = n: src = past_embeddings[b, n', c]                     (:72-89)
 *   HSTU_PREPROCESS_CONCAT      Do = item_dim + rating_dim, N' = n: columns >= item_dim are
 *                               rating_table[ratings[b, n'], c - item_dim]                                 (:133-152)
 *   HSTU_PREPROCESS_INTERLEAVE  rating_dim == item_dim == Do, N' = 2 n: row 2 i is the item, row 2 i + 1 is
 *                               rating_table[ratings[b, i], :], both masked by m(b, i)                     (:226-260)
 * fp32: fl(src s), fl(. + pos), [fl(. scale) under dropout], fl(. m) are separate roundings -- bit-exact against the
 * reference with dropout off; 16-bit: fp32 arithmetic, one rounding at the store.  `out_dtype` is `emb_dtype`, or fp32 for
 * 16-bit embeddings (torch.result_type of a 16-bit activation and an fp32 module).  Dropout: the generator of
 * hstu_norm_mul_dropout_fwd with element index e = (b N' + n') Do + c (same threshold, survivor scale and pair rule);
 * nothing is stored, the backward regenerates the mask from `seed`.  A rating outside [0, num_ratings) is clamped (memory
 * safety; it is the caller's error).  Do <= HSTU_PREPROCESS_MAX_DIM, N' <= num_positions, batch * N' < 2^31.  batch == 0
 * or n == 0: returns without a launch.  No host synchronisation; nothing is read back. */
#define HSTU_PREPROCESS_PLAIN 0
#define HSTU_PREPROCESS_CONCAT 1
#define HSTU_PREPROCESS_INTERLEAVE 2
#define HSTU_PREPROCESS_MAX_DIM 4096
int hstu_input_preprocess_fwd(const int64_t* past_ids, const void* past_embeddings, const void* ratings, const void* pos_table,
                              const void* rating_table, void* out, float* valid_mask, int32_t batch, int32_t n,
                              int32_t item_dim, int32_t rating_dim, int32_t num_positions, int32_t num_ratings, int layout,
                              float dropout_ratio, uint64_t seed, int emb_dtype, int out_dtype, int rating_index_dtype,
                              void* stream);
/* Given d_out (batch, N', Do) in `out_dtype` and h = d_out * m * keep * scale (fp32):
 *   d_past_embeddings = fl(h s) in `emb_dtype`;  d_pos_table[n', :] = sum_b h[b, n', :], rows >= N' zero;
 *   d_rating_table[r, :] = s * sum of h over the rating columns (CONCAT) / odd rows (INTERLEAVE) of the (b, i) with rating r.
 * Both table gradients are fp32 (num_positions, Do) / (num_ratings, rating_dim), summed in a fixed order -- per-thread
 * running sums over slabs of users (rows), the slabs added in order by a second kernel; no float atomics, bit-identical
 * run to run.  Any of the three outputs may be NULL and is then not computed.  `workspace`:
 * hstu_input_preprocess_bwd_workspace_bytes(...) bytes of device memory, 32-byte aligned (needed for the table gradients). */
size_t hstu_input_preprocess_bwd_workspace_bytes(int32_t batch, int32_t n, int32_t item_dim, int32_t rating_dim,
                                                 int32_t num_ratings, int layout);
int hstu_input_preprocess_bwd(const void* d_out, const int64_t* past_ids, const void* ratings, void* d_past_embeddings,
                              float* d_pos_table, float* d_rating_table, void* workspace, int32_t batch, int32_t n,
                              int32_t item_dim, int32_t rating_dim, int32_t num_positions, int32_t num_ratings, int layout,
                              float dropout_ratio, uint64_t seed, int emb_dtype, int out_dtype, int rating_index_dtype,
                              void* stream);

/* ---- int8 row-wise quantized embedding tables (inference): quantize pass and dequantizing row gather -------------------
 * The serving format of the reference's DLRM-v3 flow (dlrm_v3/inference/model_family.py:122-143: quantize_dynamic of every
 * EmbeddingCollection to QuantEmbeddingCollection, int8 weights, float activations): fbgemm's "fused 8-bit row-wise"
 * arithmetic, with row starts aligned for 16-byte loads.  A quantized table of rows x D is a uint8 array (rows, stride):
 *   meta = round_up(D, 4);  stride = round_up(meta + 8, 16) = hstu_int8_row_stride(D)
 *   bytes [0, D) the codes, [meta, meta + 4) scale (fp32, little endian), [meta + 4, meta + 8) bias (fp32), every other byte 0
 * Per row, for x widened exactly to fp32 (all arithmetic fp32, every operation rounded on its own unless said otherwise):
 *   mn = min(x), mx = max(x), range = mx - mn;   scale = range / 255.0f, bias = mn, inv = 255.0f / (range + 1e-8f)
 *   code  = clamp(round_half_even((x - mn) * inv), 0, 255)             subtract, then multiply
 *   value = code * scale + bias                                         fused multiply-add or not: both are the format
 * A constant row has scale 0, all codes 0 and round-trips exactly.  Inputs are finite with a finite range; anything else
 * gives unspecified values, never an access outside the buffers.  1 <= D <= 2048 (HSTU_EUNSUPPORTED above), rows and
 * n < 2^31; row offsets are 64-bit (rows * stride may exceed 4 GiB).  No atomics, no workspace, bit-identical run to run.
 *
 * hstu_int8_row_stride: the stride above, or HSTU_EINVAL (dim < 1) / HSTU_EUNSUPPORTED (dim > 2048).
 * hstu_quantize_rows_int8: src (rows, dim) in `src_dtype` (bf16, fp16, fp32), row stride in elements, unit column stride,
 * any alignment (rows that start 16-byte aligned are read in 16-byte pieces); dst 16-byte aligned, dst_row_stride in BYTES, a
 * multiple of 16 and >= the stride above; the first `stride` bytes of every row are written.  One pass: a group of lanes
 * owns a row, its min / max is a wave-level exchange.  rows == 0 returns without a launch.
 * hstu_gather_rows_int8: out[i, :] = value(table[idx[i]]) for i < n, in `out_dtype` (bf16, fp16, fp32; 16-bit outputs
 * round the fp32 value to nearest even).  table 16-byte aligned, table_row_stride in bytes as dst_row_stride above.  idx
 * int32 or int64 (`index_type`, HSTU_INDEX_*); idx == NULL is the identity (rows 0 .. n - 1: plain dequantization,
 * n <= table_rows).  Ids outside [0, table_rows) are clamped (memory safety; they are the caller's error).  out_row_stride
 * in elements (out may be a column slice of a wider tensor); every (row, 0) element 16-byte aligned.  n == 0 returns
 * without a launch. */
int hstu_int8_row_stride(int32_t dim);
int hstu_quantize_rows_int8(const void* src, int64_t src_row_stride, int64_t rows, int32_t dim, void* dst, int64_t dst_row_stride,
                            int src_dtype, void* stream);
int hstu_gather_rows_int8(const void* table, int64_t table_row_stride, int64_t table_rows, int32_t dim, const void* idx,
                          int index_type, int64_t n, void* out, int64_t out_row_stride, int out_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSTU_HIP_H_ */
