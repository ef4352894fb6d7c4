// Internal helpers shared by the translation units of libhstu_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/hstu_hip.h"

namespace hstu {
int set_error(int code, const char* fmt, ...);   // records the message, returns `code`
int check_launch(const char* what);              // hipGetLastError() -> HSTU_OK | HSTU_ELAUNCH

// ---- attention dispatch (attn_misc.hip) ----
// One host-side plan decides everything about an attention call exactly once: which kernel family runs, with which grid
// and LDS bytes, and where every piece of the backward's workspace lies.  The kernel-name functions, the workspace-size
// function and the launchers read it and decide nothing themselves.
enum AttnSched : int {
  kSchedNone = 0,     // refused before a kernel was chosen (plan.err / plan.msg)
  kSchedSolo,         // short sequences, one wave per (user, head)                  hstu_attn_{fwd,bwd}_solo_kernel
  kSchedSoloBias,     // ... with the research path's relative bias                  hstu_attn_{fwd,bwd}_solo_bias_kernel
  kSchedQuad,         // backward, head dim 64, <= 7 tiles: four-wave workgroups     hstu_attn_bwd_quad_kernel
  kSchedFold,         // backward, <= 7 tiles: folded schedule                       hstu_attn_bwd_fold_kernel
  kSchedLong,         // backward, longer: dK / dV kernel + dQ kernel                hstu_attn_bwd_{dkv,dq}_kernel
  kSchedFoldBias,     // backward, relative bias on the folded schedule              hstu_attn_bwd_fold_bias_kernel
  kSchedGeneral,      // hstu_attn_{fwd,bwd}_kernel (plan.bias / head_loop / precise pick the instantiation)
};
struct AttnLaunch {
  int tpt;                        // solo kernels: tiles per tensor of the instantiation (2, or 1 for the <= 32-row class)
  int grid, smem;                 // workgroups, dynamic LDS bytes
  int ts_copies, hist, tables;    // relative bias: the kernel's arguments of these names
  int len_lo, len_hi;             // solo kernels: the length class (len_lo, len_hi] this launch takes
  int row0;                       // its first bias-gradient partial row
};
struct AttnPlan {
  int err;                        // HSTU_OK, or the refusal (msg); with a schedule chosen the name is still valid
  char msg[200];
  AttnSched sched;
  int dtype;
  bool backward;
  int a, v;                       // padded head dims
  bool bias, head_loop, precise, contextual;
  int nw, nkb, nqb;               // key tiles per block, key blocks, query blocks (where the schedule has them)
  bool dma_fast;                  // folded / four-wave backward: tile requests as scalar base + 32-bit lane offset (attn_dma_addr.h)
  int n_launch;
  AttnLaunch launch[2];           // solo: the length classes; long: dK / dV, dQ; general: the kernel, the dq conversion
  // backward workspace: [fp32 dq accumulator: n_slabs x slab_bytes] [partial rows x width floats] [chunk sums: chunks x width]
  size_t slab_bytes;              // 0: no accumulator (one key block)
  int n_slabs;
  size_t partial_off;
  int partial_rows, partial_width;
  size_t zero_bytes;              // zeroed from partial_off on: the partial rows and, fold-bias, the user counter behind them
  size_t counter_off;             // fold-bias: the int the workgroups draw users from (the reduce's chunk sums take its place afterwards)
  int red_chunks;
  size_t chunk_off;
  size_t ws_bytes;                // the end of everything above
};
AttnPlan plan_attn_fwd(const HstuAttnParams& p);
AttnPlan plan_attn_bwd(const HstuAttnBwdParams& bp);
int attn_kernel_name(const AttnPlan& pl, char* buf, size_t len);   // profiler name of the instantiation the plan launches

// launchers: one switch on the plan's schedule per dtype (attn_launch.cuh), and below it one function per kernel family,
// each instantiated in the translation unit of its family and dtype (so they compile in parallel)
typedef __bf16 bf16_t;
typedef _Float16 f16_t;
template <typename T> int launch_attn_fwd(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st);
template <typename T> int launch_attn_bwd(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st);
template <typename T> int launch_fwd_bias(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st);        // attn_bias_*.hip
template <typename T> int launch_bwd_bias(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st);    // (general and folded)
template <typename T> int launch_fwd_solo(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st);        // attn_solo_*.hip
template <typename T> int launch_bwd_solo(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st);
template <typename T> int launch_fwd_solo_bias(const AttnPlan& pl, const HstuAttnParams& p, hipStream_t st);
template <typename T> int launch_bwd_solo_bias(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st);
template <typename T> int launch_bwd_fold(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st);    // attn_fold_*.hip (and quad)
template <typename T> int launch_bwd_long(const AttnPlan& pl, const HstuAttnBwdParams& bp, hipStream_t st);    // attn_long_*.hip
// (attn_launch.cuh holds the schedule switch AND the bias launchers it calls: only attn_bias_*.hip instantiate the latter)
#define HSTU_ATTN_BIAS_EXTERN(T)                                                               \
  extern template int launch_fwd_bias<T>(const AttnPlan&, const HstuAttnParams&, hipStream_t); \
  extern template int launch_bwd_bias<T>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
HSTU_ATTN_BIAS_EXTERN(bf16_t) HSTU_ATTN_BIAS_EXTERN(f16_t) HSTU_ATTN_BIAS_EXTERN(float)
#undef HSTU_ATTN_BIAS_EXTERN
// sums the per-workgroup bias-gradient rows of the plan's workspace into dpos_w / dts_w (two fixed-order stages)
int launch_bias_grad_reduce(const AttnPlan& pl, void* workspace, int npos, float* dpos_w, float* dts_w, hipStream_t st);

// compute units of the CURRENT device (cached per device: a host may hold devices of different sizes)
inline int cu_count() {
  static int cache[64] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  if (cache[dev] == 0) {
    int n = 256;
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    cache[dev] = n > 0 ? n : 256;
  }
  return cache[dev];
}
inline int pad_head_dim(int d) { return d <= 32 ? 32 : (d <= 64 ? 64 : (d <= 128 ? 128 : 0)); }
constexpr int kLdsBudget = 160 * 1024;
// more than 64 KiB of dynamic LDS has to be asked for, per kernel
inline int reserve_lds(const void* kern, int smem, const char* who) {
  if (smem <= 64 * 1024) return HSTU_OK;
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  return e == hipSuccess ? HSTU_OK : set_error(HSTU_ELAUNCH, "%s: cannot reserve %d bytes of LDS: %s", who, smem, hipGetErrorString(e));
}
inline int dtype_bytes(int dtype) { return dtype == HSTU_DTYPE_F32 ? 4 : 2; }
inline bool is_float_dtype(int dtype) { return dtype == HSTU_DTYPE_BF16 || dtype == HSTU_DTYPE_F16 || dtype == HSTU_DTYPE_F32; }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- row-pass ops (device side: row_pass.cuh) ----
// Grid of a row kernel with a grid-stride loop over `rows`, `rows_per_block` at a time: exactly the workgroups that are
// resident at once (occupancy x CUs, shared among `cols` workgroup columns), so that every wave walks the same number of
// rows and none starts late; at most max_blocks, at least 1.  Without an answer to the occupancy query: the row count's.
template <typename K>
inline int resident_row_blocks(K kernel, int threads, size_t lds_bytes, int64_t rows, int rows_per_block, int max_blocks, int cols = 1) {
  int64_t nb = (rows + rows_per_block - 1) / rows_per_block;
  if (nb > max_blocks) nb = max_blocks;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds_bytes) == hipSuccess && per_cu >= 1) {
    int64_t resident = (int64_t)per_cu * cu_count() / cols;
    if (resident < 1) resident = 1;
    if (resident < nb) nb = resident;
  }
  return (int)(nb < 1 ? 1 : nb);
}
// Finish of a row-pass backward (aux_ops.hip): column sums of the workgroups' partial rows (nparts rows of pstride floats).
// The columns go to the segments in order, `len` each; columns past the last segment are dropped.  16 columns per block of
// 256 threads: thread (r, cc) adds rows r, r + 16, .. of its column in order, then the 16 sums are added in index order.
struct ColSegment {
  float* out;
  int64_t len;
};
int launch_partial_col_sums(const float* partial, int nparts, int64_t pstride, const ColSegment (&segs)[4], const char* who,
                            hipStream_t st);

// bytes of the bias tables a workgroup stages in LDS: pos_w (2N-1 floats), ts_w (nb+1 floats), N int64 timestamps,
// their int32 offsets
inline int bias_table_bytes(int max_seq_len, int num_buckets) {
  return 128 /* zeros in front of the position table: see stage_bias_tables */ +
         ((2 * max_seq_len * 4 + 15) / 16 + ((num_buckets + 1) * 4 + 15) / 16 + (max_seq_len * 8 + 15) / 16) * 16 +
         (2 * ((max_seq_len + 32 + 3) / 4 * 4) * 4 + 8 * 4 + 15) / 16 * 16;   // + int32 offsets and their copy shifted by one (padded), one range flag per wave
}
inline int zero_workspace(void* ptr, size_t bytes, hipStream_t st) {
  hipError_t e = bytes ? hipMemsetAsync(ptr, 0, bytes, st) : hipSuccess;
  return e == hipSuccess ? HSTU_OK : set_error(HSTU_ELAUNCH, "hstu_attn_bwd: workspace memset failed: %s", hipGetErrorString(e));
}
constexpr int kDqScratchBytes = 8 * 4096;   // general backward, several key blocks: one [32 q][32 d] fp32 tile per wave

// e4m3 attention forward (attn_fp8.hip): head dims multiples of 16 up to 128, instantiated at 64 (smaller ones zero-padded) and 128
inline int fp8_head_dim(int d) { return (d <= 0 || d % 16) ? 0 : (d <= 64 ? 64 : (d <= 128 ? 128 : 0)); }
int launch_attn_fwd_fp8(const HstuAttnParams& p, const HstuFp8Descale& ds, hipStream_t st);
int launch_jagged_quantize_fp8(const void* x, int64_t rs, int64_t hs, void* x8, float* descale, const void* offsets, int batch, int heads,
                               int dim, int dtype, int index_dtype, hipStream_t st);

// jagged_dense_bmm_broadcast_add (jagged_bmm.hip): forward / data gradient and weight + bias gradient; arguments as validated by capi.hip
size_t jagged_bmm_workspace_bytes(int batch);
int launch_jagged_bmm_fwd(const void* jagged, int64_t a_rs, const void* dense, int64_t d_bs, int64_t d_ks, int64_t d_ns,
                          const float* bias, int64_t bias_bs, void* out, int64_t o_rs, const void* offsets,
                          int64_t total_rows, int batch, int k, int n, void* workspace, int dtype, int index_dtype,
                          hipStream_t st);
int launch_jagged_bmm_wgrad(const void* jagged, int64_t a_rs, const void* d_out, int64_t g_rs, void* d_dense, int64_t dd_bs,
                            int64_t dd_ks, float* d_bias, int64_t db_bs, const void* offsets, int64_t total_rows, int batch,
                            int k, int n, int dtype, int index_dtype, hipStream_t st);

// fused MIPS top-k (mips_topk.hip): radix select over recomputed MFMA score tiles; arguments as validated by capi.hip
constexpr int kMipsTopkMaxK = 4096;     // the per-row sort's LDS
constexpr int kMipsTopkMaxDim = 512;
size_t mips_topk_workspace_bytes(int batch, int k);
int launch_mips_topk(const void* queries, int64_t q_rs, const void* items, int64_t i_rs, void* out_scores, int32_t* out_indices,
                     void* workspace, int batch, int num_items, int dim, int k, int dtype, hipStream_t st);

// Mixture-of-Logits scores (mol_ops.hip): logits, gating MLP, gate and softmax-weighted sum per (query, item) pair in
// registers and LDS; arguments as validated by capi.hip
constexpr int kMolMaxLogits = HSTU_MOL_MAX_LOGITS;
constexpr int kMolMaxDim = HSTU_MOL_MAX_DIM;
constexpr int kMolMaxHidden = HSTU_MOL_MAX_HIDDEN;
int launch_mol_scores(const void* qc, const void* xc, const void* gq, const void* gi, const void* w1, const void* b1, const void* w2,
                      const void* b2, float* out, int batch, int num_items, int pq, int px, int dim, int hidden, float inv_temperature,
                      int layer_norm, int dtype, hipStream_t st);

// multitask prediction head (multitask_ops.hip): SwishLayerNorm + task projection + predictions + task losses per row, and
// the backward; arguments as validated by capi.hip.  `vec`: rows are read as 16-byte pieces (dim, pointers and row strides
// allow it), else element by element -- the two dim limits are those of hstu_swish_layer_norm_fwd
constexpr int kMultitaskMaxDimVec = 4096;
constexpr int kMultitaskMaxDimScalar = 2048;
size_t multitask_head_workspace_bytes(int dim, int tasks);
int launch_multitask_head_fwd(const void* x, int64_t x_rs, const void* ln_w, const void* ln_b, float eps, const float* w,
                              const float* c, const float* labels, const float* weights, float* logits, float* preds,
                              float* mean, float* rstd, float* loss, float* weight_sum, void* workspace, int64_t rows, int dim,
                              int tasks, int nbin, float loss_scale, int dtype, bool vec, hipStream_t st);
int launch_multitask_head_bwd(const float* grad_loss, const float* grad_pred, const void* x, int64_t x_rs, const void* ln_w,
                              const void* ln_b, const float* w, const float* labels, const float* weights, const float* logits,
                              const float* mean, const float* rstd, const float* weight_sum, void* dx, int64_t dx_rs, float* dw,
                              float* dc, float* dln_w, float* dln_b, void* workspace, int64_t rows, int dim, int tasks, int nbin,
                              float loss_scale, int dtype, bool vec, hipStream_t st);

// jagged causal softmax attention (softmax_attn.hip): arguments as validated by capi.hip.  Instantiated at head dims 32 and
// 64 (smaller ones are zero-filled on load); one wavefront per (user, head, 32-row tile).
struct SoftmaxAttnArgs {
  const void *q, *k, *v;
  int64_t q_rs, q_hs, k_rs, k_hs, v_rs, v_hs;
  const void* out;         // forward: written
  const float* lse;        // forward: written
  const void* dout;        // backward only from here
  float* delta;
  void *dq, *dk, *dv;
  const void* offsets;
  int batch, heads, head_dim, max_seq_len;
  float scale, dropout_p;
  uint64_t seed;
  int dtype, index_dtype;
};
inline int softmax_attn_head_dim(int d) { return d <= 0 ? 0 : (d <= 32 ? 32 : (d <= HSTU_SOFTMAX_ATTN_MAX_HEAD_DIM ? 64 : 0)); }
int launch_softmax_attn_fwd(const SoftmaxAttnArgs& a, hipStream_t st);
int launch_softmax_attn_bwd(const SoftmaxAttnArgs& a, hipStream_t st);
}  // namespace hstu
