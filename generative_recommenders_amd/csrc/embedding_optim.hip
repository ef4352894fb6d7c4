// In-backward sparse row-wise Adagrad for the embedding tables (the reference trains every DLRM-v3 table with
// RowWiseAdagrad fused into the backward pass: dlrm_v3/train/utils.py:190-227).  For every table row r that occurs in idx:
//     G[r, :] = sum of the dout rows with idx == r;  momentum1[r] += mean_d(G[r, d]^2);
//     W[r, :] -= lr / (sqrt(momentum1[r]) + eps) * G[r, :]
// in one pass that reads the batch's gradient rows once and reads / writes only the touched table rows: no table-sized
// gradient, no memset, O(n) workspace.
//
// 1. rows are grouped by id with the radix sort of embedding_sort.cuh (significant key bits only, stable: the duplicates
//    of an id stay in batch order);
// 2. chunk kernel, one wave per CHUNK of sorted positions (128 of them; 32 below 262,144 ids when dim <= 512, where 128
//    would leave most of the chip without a wave; grid-stride).  The chunk's (id, row) pairs arrive with one
//    coalesced load per 64; a segment head is a position whose id differs from its left neighbour's (a flag per position,
//    read where it is needed: the chunks are the work items, so nothing has to be compacted or counted).  The wave reads U
//    gradient rows at a time (16 bytes per lane and piece of a row) and adds them IN SORTED ORDER into fp32 registers.  With
//    each group it also fetches the table row and the state of every segment that ends in the group and lies wholly inside
//    the chunk, so the update at the segment's end waits for no load of its own: sum of squares reduced across the wave,
//    momentum1[r], then W[r, :].  A segment cut by a chunk boundary is not updated here: its piece of the sum goes to the
//    workspace with plain stores, at slot 2 * chunk + (0 when the segment began before the chunk, 1 when it begins in it);
// 3. combine kernel, one workgroup per chunk: the workgroup whose chunk holds the HEAD of a cut segment owns it.  Its waves
//    add equal shares of the segment's partial sums in position order, hand them over through LDS, wave 0 adds them in wave
//    order and applies the update.  A hot id with thousands of duplicates is therefore summed by many waves in step 2 and
//    by eight in step 3.
// Every segment is finished by exactly one owner before its state is touched; there are no float atomics; the order of
// summation is a function of the sorted positions alone (never of timing or of the grid size), so results are
// bit-identical from run to run.
//
// hstu_embedding_grad_coalesce runs the same three steps with another ending (the kernels' Sink): a finished segment is not
// applied to the table but written out, scale * G[r, :] and r, at the segment's rank among the segment heads -- the short
// list a data-parallel rank exchanges (ops/embedding.py).  The rank comes from an inclusive scan over the head flags of the
// sorted positions (three small kernels in front of the chunk kernel); the sums are the update's, addition for addition.
//
// Every table update -- row-wise Adagrad, sparse SGD and sparse Adam (hstu_embedding_sparse_sgd / hstu_embedding_sparse_adam;
// the other two choices of the reference's sparse_optimizer_factory_and_class), each on fp32, fp16 or bf16 tables -- is ONE
// sink, UpdateSink<W, Rule>: W the table's element type, Rule what the optimizer alone knows.  The sink owns what they share:
// the table row travels with the group of gradient rows (its Pre record; a 16-bit table's row in its raw form, half the
// registers), and at the segment's end it is widened to fp32 piece by piece, run through the rule's element function, and
// written back -- an fp32 table's into the row's own registers and out with one row store, a 16-bit table's through the
// stochastic rounding of stochastic_round.h, whose random bits are a function of (seed, table row, column) alone.  A rule
// names the scalars that travel too (Adagrad: momentum1[r]), what it does once per row (Adagrad: the row's sum of squares,
// momentum1[r], the step), and the arithmetic of one element (adagrad_element, sgd_element, adam_element): the same function
// for every table type and for both kernels, its multiply-adds pinned by fmaf, so a 16-bit table's fp32 row and state equal
// the fp32 table's bit for bit.  Adam's rule prefetches NOTHING and reads exp_avg / exp_avg_sq of the row where the segment
// ends, piece by piece: prefetched like the table row they would be 128 more registers at the reference's row width (dim 256,
// 16-bit gradients, eight rows in flight: 8 + 32 + 64 are held already), which leaves the wave alone on its SIMD, while the
// loads at the segment's end are hidden by the other waves the smaller kernel leaves room for.
//
// What the host decides -- chunk size, row class, workspace layouts, grids, LDS bytes, the widest row of every entry point --
// is embedding_optim_dispatch.h, host-only and swept by a CPU test; this unit compiles exactly the classes it can return.
#include <utility>

#include "hstu_common.cuh"
#include "capi_internal.h"
#include "embedding_optim_dispatch.h"
#include "embedding_sort.cuh"
#include "row_pass.cuh"
#include "stochastic_round.h"

namespace hstu {

using namespace embedding_optim;

// acc[j][c]: column (lane + 64 j) * VEC + c of the row; pieces = dim / VEC of them are real
template <int VEC, int NP>
__device__ __forceinline__ void load_f32_row(const float* __restrict__ row, int lane, int pieces, float (&w)[NP][VEC]) {
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = lane + 64 * j;
    if (p < pieces) {
#pragma unroll
      for (int c = 0; c < VEC; c += 4) *(float4*)&w[j][c] = *(const float4*)(row + (int64_t)p * VEC + c);
    }
  }
}

template <int VEC, int NP>
__device__ __forceinline__ void store_f32_row(float* __restrict__ row, int lane, int pieces, const float (&w)[NP][VEC]) {
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = lane + 64 * j;
    if (p < pieces) {
#pragma unroll
      for (int c = 0; c < VEC; c += 4) *(float4*)(row + (int64_t)p * VEC + c) = *(const float4*)&w[j][c];
    }
  }
}

template <int VEC, int NP>
__device__ __forceinline__ void add_row(float (&acc)[NP][VEC], const float (&v)[NP][VEC], int lane, int pieces) {
#pragma unroll
  for (int j = 0; j < NP; ++j)
    if (lane + 64 * j < pieces) {
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[j][c] += v[j][c];
    }
}

// sum_d G[r, d]^2 of the row in acc, in every lane.  ONE tree for every row layout, so that the same G gives the same bits
// whether it is summed from 16-bit rows (8 columns per lane and piece) or read back as an fp32 row (4 columns per lane and
// piece: the coalesced lists of replicated tables) -- and whichever kernel finishes the segment: every square is rounded
// on its own (no contraction into a fused multiply-add, which the compiler would choose per kernel), then added
// pairwise over the 8 columns of a group g = column / 8, then over the groups by the bits of g: 6, 7 (the lane's pieces,
// 64 groups apart), then 5 .. 0 (the butterfly across the wave).  An fp32 lane holds half a group; lane m, piece j is the
// half b = m & 1 of group (m >> 1) + 32 j: bit 5 of g is bit 0 of j, bits 6 and 7 are bits 1 and 2 of j.  Absent columns add 0.
template <int VEC, int NP>
__device__ __forceinline__ float row_sum_of_squares(const float (&acc)[NP][VEC], int lane, int pieces) {
#pragma clang fp contract(off)
  static_assert(VEC == 4 || VEC == 8, "16-byte pieces of fp32 or 16-bit columns");
  float sq[NP][VEC];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const bool live = lane + 64 * j < pieces;
#pragma unroll
    for (int c = 0; c < VEC; ++c) sq[j][c] = live ? acc[j][c] * acc[j][c] : 0.f;
  }
#pragma unroll
  for (int s = 1; s < VEC; s *= 2)
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int c = 0; c + s < VEC; c += 2 * s) sq[j][c] += sq[j][c + s];
  if constexpr (VEC == 4) {
#pragma unroll
    for (int j = 0; j < NP; ++j) sq[j][0] += __shfl_xor(sq[j][0], 1);     // the two halves of a group
#pragma unroll
    for (int s = 2; s < NP; s *= 2)                 // bits 6, 7 of g
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if ((j & (2 * s - 2)) == 0 && j + s < NP) sq[j][0] += sq[j + s][0];
    if (NP > 1) sq[0][0] += sq[1][0];               // bit 5
  } else {
#pragma unroll
    for (int s = 1; s < NP; s *= 2)
#pragma unroll
      for (int j = 0; j + s < NP; j += 2 * s) sq[j][0] += sq[j + s][0];
  }
  float ss = sq[0][0];
#pragma unroll
  for (int off = 32; off >= (VEC == 4 ? 2 : 1); off >>= 1) ss += __shfl_xor(ss, off);
  return ss;
}

// The registers a prefetched table row waits in: fp32 as loaded, or the raw 16-bit elements, two per register (VEC / 2
// registers per piece: 16 bytes per lane and piece next to 16-bit gradient rows, 8 bytes next to fp32 ones)
template <typename WT, int VEC, int NP>
struct WRow { typedef float type[NP][VEC]; };
template <int VEC, int NP>
struct WRow<f16_t, VEC, NP> { typedef uint32_t type[NP][VEC / 2]; };
template <int VEC, int NP>
struct WRow<bf16_t, VEC, NP> { typedef uint32_t type[NP][VEC / 2]; };

template <int VEC, int NP>
__device__ __forceinline__ void load_w_row(const float* __restrict__ row, int lane, int pieces, float (&w)[NP][VEC]) {
  load_f32_row<VEC, NP>(row, lane, pieces, w);
}
template <int VEC, int NP, typename W>
__device__ __forceinline__ void load_w_row(const W* __restrict__ row, int lane, int pieces, uint32_t (&w)[NP][VEC / 2]) {
  static_assert(sizeof(W) == 2, "16-bit table rows");
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = lane + 64 * j;
    if (p < pieces) {
      if constexpr (VEC == 8) *(u32x4*)&w[j][0] = *(const u32x4*)(row + (int64_t)p * VEC);
      else *(u32x2*)&w[j][0] = *(const u32x2*)(row + (int64_t)p * VEC);
    }
  }
}

// 16 raw bits of a table element -> fp32, and the stochastic rounding back (stochastic_round.h)
template <typename W>
__device__ __forceinline__ float widen16(uint32_t h) {
  if constexpr (__is_same(W, bf16_t)) return __builtin_bit_cast(float, h << 16);
  else return (float)__builtin_bit_cast(f16_t, (uint16_t)h);
}
template <typename W>
__device__ __forceinline__ uint32_t round16(float x, uint32_t r) {
  if constexpr (__is_same(W, bf16_t)) return hstu_sr_bf16(__builtin_bit_cast(uint32_t, x), r);
  else return hstu_sr_f16(__builtin_bit_cast(uint32_t, x), r);
}
// The rule has a PLAIN form wherever it needs none of its special cases: finite values that cannot reach the clamp (bf16),
// finite values of at least 2^-14 (fp16).  There bf16 is the upper half of bits + r, and fp16 is bits + 13 random bits with
// the low 13 cleared -- a value ON the fp16 grid, so the hardware's conversion is exact whatever its rounding mode --,
// clamped to +-65504 as a float.  Same bits as round16 (tests/test_embedding_lowp_gpu.py holds both forms against the numpy
// restatement), a fifth of the instructions: the update is bound by them, not by bytes, at the reference's row width.
template <typename W>
__device__ __forceinline__ bool is_plain16(float x) {
  if constexpr (__is_same(W, bf16_t)) return fabsf(x) <= __builtin_bit_cast(float, 0x7f7f0000u);     // false for NaN
  else return fabsf(x) >= 0x1p-14f && fabsf(x) < __builtin_inff();
}
// (lo, hi) with the 32 random bits h of their column pair -> the two 16-bit results, packed as they lie in memory
template <typename W>
__device__ __forceinline__ uint32_t round_pair_plain(float lo, float hi, uint32_t h) {
  const uint32_t a = __builtin_bit_cast(uint32_t, lo), b = __builtin_bit_cast(uint32_t, hi);
  if constexpr (__is_same(W, bf16_t)) {
    return ((a + (h & 0xffffu)) >> 16) | ((b + (h >> 16)) & 0xffff0000u);
  } else {
    const float x = __builtin_bit_cast(float, (a + (h & 0x1fffu)) & ~0x1fffu);
    const float y = __builtin_bit_cast(float, (b + ((h >> 16) & 0x1fffu)) & ~0x1fffu);
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(fminf(fmaxf(x, -65504.f), 65504.f), fminf(fmaxf(y, -65504.f), 65504.f)));
  }
}
// VEC fp32 values of table row `row` from column pair `pair0` on -> VEC / 2 registers of 16-bit results.  The plain form
// when every value of every lane of the wave allows it (one branch per wave and piece, no divergence), else the rule in full.
template <typename W, int VEC>
__device__ __forceinline__ void round_piece(const float (&x)[VEC], uint64_t seed, uint32_t row, uint32_t pair0, uint32_t (&out)[VEC / 2]) {
  uint32_t h[VEC / 2];
  bool plain = true;
#pragma unroll
  for (int c = 0; c < VEC / 2; ++c) {
    h[c] = hstu_sr_hash(seed, row, pair0 + c);
    plain = plain && is_plain16<W>(x[2 * c]) && is_plain16<W>(x[2 * c + 1]);
  }
  if (__builtin_amdgcn_ballot_w64(!plain) == 0) {
#pragma unroll
    for (int c = 0; c < VEC / 2; ++c) out[c] = round_pair_plain<W>(x[2 * c], x[2 * c + 1], h[c]);
  } else {
#pragma unroll
    for (int c = 0; c < VEC / 2; ++c) out[c] = round16<W>(x[2 * c], h[c] & 0xffffu) | (round16<W>(x[2 * c + 1], h[c] >> 16) << 16);
  }
}

// piece j of a prefetched table row as fp32 (a 16-bit table's is widened) ...
template <typename WT, int VEC, int NP>
__device__ __forceinline__ void widen_piece(const typename WRow<WT, VEC, NP>::type& w, int j, float (&x)[VEC]) {
  if constexpr (sizeof(WT) == 2) {
#pragma unroll
    for (int c = 0; c < VEC / 2; ++c) {
      x[2 * c] = widen16<WT>(w[j][c] & 0xffffu);
      x[2 * c + 1] = widen16<WT>(w[j][c] >> 16);
    }
  } else {
#pragma unroll
    for (int c = 0; c < VEC; ++c) x[c] = w[j][c];
  }
}
// ... and piece p of row `id` of a 16-bit table written back: every element rounded with its own 16 random bits -- one hash per
// column pair (round_piece)
template <typename WT, int VEC>
__device__ __forceinline__ void write_piece(WT* __restrict__ w_row, int p, const float (&x)[VEC], uint64_t seed, int id) {
  static_assert(sizeof(WT) == 2, "an fp32 row goes back into its own registers (UpdateSink::finish)");
  uint32_t out[VEC / 2];
  round_piece<WT, VEC>(x, seed, (uint32_t)id, (uint32_t)(p * (VEC / 2)), out);
  if constexpr (VEC == 8) *(u32x4*)(w_row + (int64_t)p * VEC) = *(const u32x4*)&out[0];
  else *(u32x2*)(w_row + (int64_t)p * VEC) = *(const u32x2*)&out[0];
}

// What the chunk and combine kernels do with a finished segment is their Sink.  A sink names what travels with a group of
// gradient rows for every segment that ends in the group (Pre, filled by prefetch: table row `id`, whose segment ends at the
// sorted position `pos`) and what happens at the segment's end (finish: acc = G[id, :]).  It states kApplies (it updates a
// table: the header's row classes differ) and kRounds (finish rounds a 16-bit row: the combine kernel makes room for that).
// An optimizer's Rule: Pre, the scalars that travel with the table row (prefetch); begin, once per finished row, whose result
// every piece gets; piece, the element function over one piece p of the row -- g = G[id, piece p], x = W[id, piece p] in fp32.
//
// Row-wise Adagrad: momentum1[id] travels; the row's step comes from the sum of squares of G[id, :] ...
__device__ __forceinline__ float adagrad_element(float g, float w, float step) { return fmaf(-step, g, w); }

struct AdagradRule {
  float* momentum1;
  float lr, eps;
  struct Pre {
    float m_old = 0.f;
  };
  __device__ __forceinline__ void prefetch(Pre& s, int id) const { s.m_old = momentum1[id]; }
  template <int VEC, int NP>
  __device__ __forceinline__ float begin(const float (&acc)[NP][VEC], const Pre& s, int id, int lane, int pieces, int dim) const {
    const float ss = row_sum_of_squares<VEC, NP>(acc, lane, pieces);
    const float m_new = s.m_old + ss / (float)dim;
    if (lane == 0) momentum1[id] = m_new;
    return lr / (sqrtf(m_new) + eps);
  }
  template <int VEC>
  __device__ __forceinline__ void piece(const float (&g)[VEC], float (&x)[VEC], float step, int p) const {
#pragma unroll
    for (int c = 0; c < VEC; ++c) x[c] = adagrad_element(g[c], x[c], step);
  }
};

// ... SGD, W[r, :] -= lr * G[r, :]: nothing but the table row travels ...
__device__ __forceinline__ float sgd_element(float g, float w, float lr) { return fmaf(-lr, g, w); }

struct SgdRule {
  float lr;
  struct Pre {};
  __device__ __forceinline__ void prefetch(Pre&, int) const {}
  template <int VEC, int NP>
  __device__ __forceinline__ float begin(const float (&)[NP][VEC], const Pre&, int, int, int, int) const {
    return lr;
  }
  template <int VEC>
  __device__ __forceinline__ void piece(const float (&g)[VEC], float (&x)[VEC], float lr_, int p) const {
#pragma unroll
    for (int c = 0; c < VEC; ++c) x[c] = sgd_element(g[c], x[c], lr_);
  }
};

// ... Adam (torch.optim.Adam's arithmetic, amsgrad off, applied to the touched rows only).  The host forms the bias corrections
// 1 - beta^t in double and hands over: one_minus_beta = (float)(1 - beta), step_size = lr / (float)bc1, sqrt_bc2 =
// sqrtf((float)bc2).  One element, the same function for every table type and both kernels; IEEE sqrt and divide, every
// multiply-add pinned:
struct AdamCoef {
  float beta1, one_minus_beta1, beta2, one_minus_beta2, step_size, sqrt_bc2, eps;
};
__device__ __forceinline__ float adam_element(float g, float& m, float& v, float w, const AdamCoef& k) {
#pragma clang fp contract(off)
  m = fmaf(k.beta1, m, k.one_minus_beta1 * g);
  v = fmaf(k.beta2, v, (k.one_minus_beta2 * g) * g);
  return w - (k.step_size * m) / (sqrtf(v) / k.sqrt_bc2 + k.eps);
}

// Nothing but the table row travels: exp_avg[id, :] and exp_avg_sq[id, :] are read where the segment ends, piece by piece (see
// the head of this file for why).  The row hands its pieces row `id` of the two state tensors.  (Two pointers formed once per row, not
// an offset added per piece: with that the kernels of two and more pieces take some 20 more registers, and several lose a
// wave per SIMD.)
struct AdamRule {
  float *exp_avg, *exp_avg_sq;
  AdamCoef k;
  struct Pre {};
  struct Row {
    float *m, *v;
  };
  __device__ __forceinline__ void prefetch(Pre&, int) const {}
  template <int VEC, int NP>
  __device__ __forceinline__ Row begin(const float (&)[NP][VEC], const Pre&, int id, int, int, int dim) const {
    return Row{exp_avg + (int64_t)id * dim, exp_avg_sq + (int64_t)id * dim};
  }
  template <int VEC>
  __device__ __forceinline__ void piece(const float (&g)[VEC], float (&x)[VEC], const Row& row, int p) const {
    float* m_at = row.m + (int64_t)p * VEC;
    float* v_at = row.v + (int64_t)p * VEC;
    float m[VEC], v[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c += 4) {
      *(float4*)&m[c] = *(const float4*)(m_at + c);
      *(float4*)&v[c] = *(const float4*)(v_at + c);
    }
#pragma unroll
    for (int c = 0; c < VEC; ++c) x[c] = adam_element(g[c], m[c], v[c], x[c], k);
#pragma unroll
    for (int c = 0; c < VEC; c += 4) {
      *(float4*)(m_at + c) = *(const float4*)&m[c];
      *(float4*)(v_at + c) = *(const float4*)&v[c];
    }
  }
};

// The update of a table of W (float, f16_t or bf16_t) by Rule: the table row and the rule's scalars travel; at the segment's
// end every piece is widened, updated and written back.  The one place where the table types part: an fp32 row goes back into
// its own registers and out with one row store, a 16-bit row through write_piece's stochastic rounding with `seed`.
template <typename W, typename Rule>
struct UpdateSink {
  static constexpr bool kApplies = true;
  static constexpr bool kRounds = sizeof(W) == 2;
  W* weight;
  Rule rule;
  uint64_t seed;
  template <int VEC, int NP>
  struct Pre {
    typename WRow<W, VEC, NP>::type w;
    typename Rule::Pre s;
  };
  template <int VEC, int NP>
  __device__ __forceinline__ void prefetch(Pre<VEC, NP>& pre, int id, int64_t pos, int lane, int pieces, int dim) const {
    load_w_row<VEC, NP>(weight + (int64_t)id * dim, lane, pieces, pre.w);
    rule.prefetch(pre.s, id);
  }
  template <int VEC, int NP>
  __device__ __forceinline__ void finish(const float (&acc)[NP][VEC], Pre<VEC, NP>& pre, int id, int lane, int pieces, int dim) const {
    W* __restrict__ w_row = weight + (int64_t)id * dim;
    const auto row = rule.template begin<VEC, NP>(acc, pre.s, id, lane, pieces, dim);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int p = lane + 64 * j;
      if (p < pieces) {
        float x[VEC];
        widen_piece<W, VEC, NP>(pre.w, j, x);
        rule.template piece<VEC>(acc[j], x, row, p);
        if constexpr (kRounds) {
          write_piece<W, VEC>(w_row, p, x, seed, id);
        } else {
#pragma unroll
          for (int c = 0; c < VEC; ++c) pre.w[j][c] = x[c];
        }
      }
    }
    if constexpr (!kRounds) store_f32_row<VEC, NP>(w_row, lane, pieces, pre.w);
  }
};

// ... or write it out (the coalesce): scale * G[r, :] and r at the segment's rank among the segment heads.  rank[p] = number of
// segment heads among the sorted positions 0 .. p, the same for every position of a segment, so any of them names the
// segment's slot rank[p] - 1, which travels
struct EmitSink {
  static constexpr bool kApplies = false;
  static constexpr bool kRounds = false;
  int32_t* rows;
  float* G;
  const int32_t* rank;
  float scale;
  template <int VEC, int NP>
  struct Pre {
    int slot = 0;
  };
  template <int VEC, int NP>
  __device__ __forceinline__ void prefetch(Pre<VEC, NP>& pre, int id, int64_t pos, int lane, int pieces, int dim) const {
    pre.slot = rank[pos] - 1;
  }
  template <int VEC, int NP>
  __device__ __forceinline__ void finish(const float (&acc)[NP][VEC], Pre<VEC, NP>& pre, int id, int lane, int pieces, int dim) const {
    float out[NP][VEC];
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int c = 0; c < VEC; ++c) out[j][c] = scale * acc[j][c];
    store_f32_row<VEC, NP>(G + (int64_t)pre.slot * dim, lane, pieces, out);
    if (lane == 0) rows[pre.slot] = id;
  }
};

template <typename T, int NP, int U, int kChunk, typename Sink>
__global__ __launch_bounds__(kOptWaves * 64) void optim_chunk_kernel(const T* __restrict__ g, const int32_t* __restrict__ perm,
                                                                       const int32_t* __restrict__ sorted_idx, int64_t n, int dim,
                                                                       float* __restrict__ partials, Sink sink) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * kOptWaves;
  const int64_t chunks = (n + kChunk - 1) / kChunk;
  const int pieces = dim / VEC;                     // dim * sizeof(T) is a multiple of 16 (checked by the caller)
  for (int64_t b = (int64_t)blockIdx.x * kOptWaves + (threadIdx.x >> 6); b < chunks; b += waves) {
    const int64_t c0 = b * kChunk;
    const int cnt = (int)min((int64_t)kChunk, n - c0);
    constexpr int kLoads = kChunk > 64 ? 2 : 1;
    static_assert(kChunk <= 128, "id_at / row_at pick one of at most two registers");
    int my_idx[kLoads], my_row[kLoads];
#pragma unroll
    for (int t = 0; t < kLoads; ++t) {
      const int p = lane + 64 * t;
      my_idx[t] = p < cnt ? sorted_idx[c0 + p] : -1;
      my_row[t] = p < cnt ? perm[c0 + p] : 0;
    }
    const int prev_id = c0 > 0 ? sorted_idx[c0 - 1] : -1;               // the neighbours across the chunk's two ends
    const int tail_id = c0 + cnt < n ? sorted_idx[c0 + cnt] : -1;
    // position q of the chunk (the same q in every lane) -> its id / its row number, in a scalar register
    auto id_at = [&](int q) { return __builtin_amdgcn_readfirstlane(__shfl(q < 64 ? my_idx[0] : my_idx[kLoads - 1], q & 63)); };
    auto row_at = [&](int q) { return __builtin_amdgcn_readfirstlane(__shfl(q < 64 ? my_row[0] : my_row[kLoads - 1], q & 63)); };
    bool open_left = id_at(0) == prev_id;           // the segment under way began before this chunk
    float acc[NP][VEC];
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[j][c] = 0.f;
    for (int r0 = 0; r0 < cnt; r0 += U) {
      u32x4 v[U][NP];
      typename Sink::template Pre<VEC, NP> pre[U];
      int id[U];
      bool ends[U], whole[U];
      bool began_before = open_left;                // of the segment that row u belongs to
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool live = r0 + u < cnt;
        const int q = min(r0 + u, cnt - 1);
        id[u] = id_at(q);
        const int next_id = q + 1 < cnt ? id_at(q + 1) : tail_id;
        ends[u] = live && (q == cnt - 1 || next_id != id[u]);
        whole[u] = ends[u] && !began_before && next_id != id[u];
        if (ends[u]) began_before = false;
        const char* row = (const char*)(g + (int64_t)row_at(q) * dim);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          const int p = lane + 64 * j;
          if (p < pieces) v[u][j] = *(const u32x4*)(row + 16 * p);
        }
        if (whole[u]) sink.template prefetch<VEC, NP>(pre[u], id[u], c0 + q, lane, pieces, dim);   // travels with the gradient rows
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (r0 + u >= cnt) break;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          if (lane + 64 * j < pieces) {
            const T* x = (const T*)&v[u][j];
#pragma unroll
            for (int c = 0; c < VEC; ++c) acc[j][c] += (float)x[c];
          }
        }
        if (ends[u]) {
          if (whole[u]) {
            sink.template finish<VEC, NP>(acc, pre[u], id[u], lane, pieces, dim);
          } else {
            store_f32_row<VEC, NP>(partials + (2 * b + (open_left ? 0 : 1)) * dim, lane, pieces, acc);
          }
          open_left = false;
#pragma unroll
          for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int c = 0; c < VEC; ++c) acc[j][c] = 0.f;
        }
      }
    }
  }
}

// One workgroup per chunk.  The chunk's last segment is cut when it goes on in the next chunk; this workgroup owns it when
// its head lies in this chunk.  Its partial sums, in position order: slot (b, 1), then slot (k, 0) of every following chunk
// k up to the first one the segment does not leave.  Wave w adds the w-th share of that list; wave 0 adds the shares in wave
// order.  (Every condition below is the same in all threads of the workgroup: the barriers are reached by all or none.)
template <int VEC, int NP, int kChunk, typename Sink>
__global__ __launch_bounds__(kCombineWaves * 64) void optim_combine_kernel(const int32_t* __restrict__ sorted_idx, int64_t n, int dim,
                                                                             const float* __restrict__ partials, Sink sink) {
  extern __shared__ __attribute__((aligned(16))) float shares[];       // (kCombineWaves - 1) rows of dim floats
  constexpr int U = NP >= 8 ? 1 : NP * VEC >= 32 ? 2 : NP * VEC >= 16 ? 4 : 8;   // partial sums in flight: 64 registers (32 in eight pieces)
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t chunks = (n + kChunk - 1) / kChunk;
  const int pieces = dim / VEC;
  for (int64_t b = blockIdx.x; b + 1 < chunks; b += gridDim.x) {
    const int64_t c0 = b * kChunk, c1 = c0 + kChunk;        // c1 < n: this is not the last chunk
    const int id = sorted_idx[c1 - 1];
    if (sorted_idx[c1] != id) continue;                      // nothing leaves this chunk
    if (b > 0 && sorted_idx[c0] == id && sorted_idx[c0 - 1] == id) continue;   // the head lies in an earlier chunk
    // the last chunk that holds a piece of the segment: the first k > b that the segment does not leave
    int64_t last = b + 1;
    for (;;) {
      const int64_t k = last + lane;
      const bool leaves = k + 1 < chunks && sorted_idx[(k + 1) * kChunk] == id;
      const unsigned long long stay = __ballot(!leaves);
      if (stay) {
        last += __ffsll((long long)stay) - 1;
        break;
      }
      last += 64;
    }
    const int64_t total = last - b + 1;                      // list item 0: slot (b, 1); item i > 0: slot (b + i, 0)
    const int64_t share = (total + kCombineWaves - 1) / kCombineWaves;
    const int64_t i0 = wave * share, i1 = min(total, i0 + share);
    typename Sink::template Pre<VEC, NP> pre;
    float acc[NP][VEC];
    if (wave == 0) sink.template prefetch<VEC, NP>(pre, id, c1 - 1, lane, pieces, dim);
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[j][c] = 0.f;
    for (int64_t k0 = i0; k0 < i1; k0 += U) {
      float v[U][NP][VEC];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = min(k0 + u, i1 - 1);
        load_f32_row<VEC, NP>(partials + (i == 0 ? 2 * b + 1 : 2 * (b + i)) * dim, lane, pieces, v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k0 + u >= i1) break;
        add_row<VEC, NP>(acc, v[u], lane, pieces);
      }
    }
    if (wave > 0) store_f32_row<VEC, NP>(shares + (int64_t)(wave - 1) * dim, lane, pieces, acc);
    __syncthreads();
    if (wave == 0) {
      // eight pieces: one share at a time, or the row's registers spill; so do four next to a 16-bit table's rounding
      constexpr int kShareUnroll = NP >= 8 || (NP >= 4 && Sink::kRounds) ? 1 : kCombineWaves - 1;
#pragma unroll kShareUnroll
      for (int s = 0; s < kCombineWaves - 1; ++s) {
        float v[NP][VEC];
        load_f32_row<VEC, NP>(shares + (int64_t)s * dim, lane, pieces, v);
        add_row<VEC, NP>(acc, v, lane, pieces);
      }
      sink.template finish<VEC, NP>(acc, pre, id, lane, pieces, dim);
    }
    __syncthreads();                                         // the shares are read before the next segment's are written
  }
}

// ---- the coalesce's slots: rank[p] = number of segment heads among the sorted positions 0 .. p (an inclusive scan of the
// head flags; integers, so any order gives the same result).  Tiles of kScanTile positions: count the heads per tile,
// scan the tile counts in one workgroup (which also knows the total: *count), scan every tile from its offset.
// exclusive scan of one value per thread across the workgroup (THREADS / 64 waves); total: the sum, in every thread
template <int THREADS>
__device__ __forceinline__ int block_exclusive_scan(int v, int* wave_sums, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off *= 2) {
    const int t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const int s = wave_sums[w];
    before += w < wave ? s : 0;
    total += s;
  }
  __syncthreads();                                  // wave_sums is written again by the caller's next round
  return before + incl - v;
}

// the head flags of the thread's kScanItems positions from p0 on (positions >= n: 0); returns their sum
__device__ __forceinline__ int head_flags(const int32_t* __restrict__ sorted_idx, int64_t n, int64_t p0, int (&flag)[kScanItems]) {
  int prev = p0 > 0 && p0 <= n ? sorted_idx[p0 - 1] : -1;          // ids are >= 0: position 0 is a head
  int sum = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    const bool live = p0 + i < n;
    const int id = live ? sorted_idx[p0 + i] : prev;
    flag[i] = live && id != prev;
    sum += flag[i];
    prev = id;
  }
  return sum;
}

__global__ __launch_bounds__(kScanThreads) void head_count_kernel(const int32_t* __restrict__ sorted_idx, int64_t n, int64_t tiles,
                                                                  int32_t* __restrict__ tile_heads) {
  __shared__ int wave_sums[kScanThreads / 64];
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    int flag[kScanItems], total;
    const int mine = head_flags(sorted_idx, n, t * kScanTile + (int64_t)threadIdx.x * kScanItems, flag);
    (void)block_exclusive_scan<kScanThreads>(mine, wave_sums, total);
    if (threadIdx.x == 0) tile_heads[t] = total;
  }
}

// one workgroup, in place: tile_heads[t] -> the heads in front of tile t; *count = all of them
__global__ __launch_bounds__(kTileScanThreads) void tile_offsets_kernel(int32_t* __restrict__ tile_heads, int64_t tiles,
                                                                        int32_t* __restrict__ count) {
  __shared__ int wave_sums[kTileScanThreads / 64];
  int carry = 0;
  for (int64_t t0 = 0; t0 < tiles; t0 += kTileScanThreads) {
    const int64_t t = t0 + threadIdx.x;
    const int v = t < tiles ? tile_heads[t] : 0;
    int total;
    const int before = block_exclusive_scan<kTileScanThreads>(v, wave_sums, total);
    if (t < tiles) tile_heads[t] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(kScanThreads) void head_rank_kernel(const int32_t* __restrict__ sorted_idx, int64_t n, int64_t tiles,
                                                                 const int32_t* __restrict__ tile_offsets, int32_t* __restrict__ rank) {
  __shared__ int wave_sums[kScanThreads / 64];
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t p0 = t * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int flag[kScanItems], total;
    const int mine = head_flags(sorted_idx, n, p0, flag);
    int r = tile_offsets[t] + block_exclusive_scan<kScanThreads>(mine, wave_sums, total);
    int out[kScanItems];
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) out[i] = r += flag[i];
    if (p0 + kScanItems <= n) {                     // rank is 256-byte aligned and p0 a multiple of 8: 16-byte stores
#pragma unroll
      for (int i = 0; i < kScanItems; i += 4) *(int4*)(rank + p0 + i) = *(const int4*)&out[i];
    } else {
#pragma unroll
      for (int i = 0; i < kScanItems; ++i)
        if (p0 + i < n) rank[p0 + i] = out[i];
    }
  }
}

// what the kernels walk: the gradient rows and the carved workspace (rank, tile_heads: the coalesce's)
struct OptArgs {
  const void* g;
  const int32_t *perm, *sorted_idx;
  int64_t n;
  int dim;
  float* partials;
  int32_t *rank, *tile_heads;
  hipStream_t st;
};

static int launch_head_ranks(const OptArgs& a, const Plan& p, int32_t* count, const char* what) {
  const dim3 grid((unsigned)p.scan_grid);
  hipLaunchKernelGGL(head_count_kernel, grid, dim3(kScanThreads), 0, a.st, a.sorted_idx, a.n, p.scan_tiles, a.tile_heads);
  if (int rc = check_launch(what)) return rc;
  hipLaunchKernelGGL(tile_offsets_kernel, dim3(1), dim3(kTileScanThreads), 0, a.st, a.tile_heads, p.scan_tiles, count);
  if (int rc = check_launch(what)) return rc;
  hipLaunchKernelGGL(head_rank_kernel, grid, dim3(kScanThreads), 0, a.st, a.sorted_idx, a.n, p.scan_tiles, (const int32_t*)a.tile_heads,
                     a.rank);
  return check_launch(what);
}

// The class (T, NP, U, kChunk) of the plan's kernels, compiled where the plan can name it and nowhere else; true: it was p's
template <typename T, int NP, int U, int kChunk, typename Sink>
static bool opt_launch(const OptArgs& a, const Plan& p, const Sink& sink, const char* what, int* rc) {
  if constexpr (reachable((int)sizeof(T), NP, U, kChunk, Sink::kApplies)) {
    if (p.np != NP || p.u != U || p.chunk != kChunk) return false;
    constexpr int VEC = 16 / (int)sizeof(T);
    hipLaunchKernelGGL((optim_chunk_kernel<T, NP, U, kChunk, Sink>), dim3((unsigned)p.chunk_grid), dim3(kOptWaves * 64), 0, a.st,
                       (const T*)a.g, a.perm, a.sorted_idx, a.n, a.dim, a.partials, sink);
    *rc = check_launch(what);
    if (*rc || !p.combine_grid) return true;
    hipLaunchKernelGGL((optim_combine_kernel<VEC, NP, kChunk, Sink>), dim3((unsigned)p.combine_grid), dim3(kCombineWaves * 64),
                       p.combine_lds, a.st, a.sorted_idx, a.n, a.dim, a.partials, sink);
    *rc = check_launch(what);
    return true;
  }
  return false;
}

// every row class of the header at both chunk sizes: the first that is the plan's launches (row_class returns no other)
template <typename T, typename Sink, size_t... I>
static int opt_dispatch(const OptArgs& a, const Sink& sink, const char* what, std::index_sequence<I...>) {
  const Plan p = plan((int)sizeof(T), a.dim, a.n, Sink::kApplies);
  int rc = HSTU_OK;
  (void)((opt_launch<T, kRowClasses[I].np, kRowClasses[I].u, kChunkSmall>(a, p, sink, what, &rc) ||
          opt_launch<T, kRowClasses[I].np, kRowClasses[I].u, kChunkLarge>(a, p, sink, what, &rc)) || ...);
  return rc;
}

// hstu_stochastic_round: one wave per row (grid-stride), lanes own 16-byte pieces of the 16-bit row (VEC = 8; VEC = 1 for
// rows that are no 16-byte multiples), every element rounded with the bits of (seed, row id, column)
constexpr int kSrWaves = 4;
template <typename W, int VEC>
__global__ __launch_bounds__(kSrWaves * 64) void stochastic_round_kernel(const float* __restrict__ src, const int32_t* __restrict__ row_ids,
                                                                         void* __restrict__ dst_, int64_t n, int dim, uint64_t seed) {
  uint16_t* __restrict__ dst = (uint16_t*)dst_;
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * kSrWaves + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * kSrWaves) {
    const uint32_t row = row_ids ? (uint32_t)row_ids[i] : (uint32_t)i;
    for (int c0 = lane * VEC; c0 < dim; c0 += 64 * VEC) {     // dim % VEC == 0: a piece is whole or absent
      float x[VEC];
      load_param<VEC>(x, src + i * dim + c0, true);
      if constexpr (VEC == 1) {
        dst[i * dim + c0] = (uint16_t)round16<W>(x[0], hstu_sr_bits(seed, row, (uint32_t)c0));
      } else {
        uint32_t out[VEC / 2];
        round_piece<W, VEC>(x, seed, row, (uint32_t)(c0 / 2), out);
        *(u32x4*)(dst + i * dim + c0) = *(const u32x4*)&out[0];
      }
    }
  }
}

template <typename Sink>
static int opt_dispatch_dtype(int dtype, const OptArgs& a, const Sink& sink, const char* what) {
  constexpr auto classes = std::make_index_sequence<sizeof(kRowClasses) / sizeof(kRowClasses[0])>{};
  switch (dtype) {
    case HSTU_DTYPE_BF16: return opt_dispatch<bf16_t>(a, sink, what, classes);
    case HSTU_DTYPE_F16: return opt_dispatch<f16_t>(a, sink, what, classes);
    default: return opt_dispatch<float>(a, sink, what, classes);
  }
}

// an update's sink for the table's element type: UpdateSink<float | f16_t | bf16_t, Rule> (an fp32 table is not rounded: seed 0)
template <typename Rule>
static int update_dispatch(int weight_dtype, void* weight, const Rule& rule, uint64_t seed, int dtype, const OptArgs& a, const char* what) {
  switch (weight_dtype) {
    case HSTU_DTYPE_F16: return opt_dispatch_dtype(dtype, a, UpdateSink<f16_t, Rule>{(f16_t*)weight, rule, seed}, what);
    case HSTU_DTYPE_BF16: return opt_dispatch_dtype(dtype, a, UpdateSink<bf16_t, Rule>{(bf16_t*)weight, rule, seed}, what);
    default: return opt_dispatch_dtype(dtype, a, UpdateSink<float, Rule>{(float*)weight, rule, 0}, what);
  }
}

static size_t sort_temp(int64_t n, int table_rows) { return n ? sort_temp_bytes(n, table_rows) : 0; }

}  // namespace hstu

using namespace hstu;

extern "C" {

int hstu_embedding_rowwise_adagrad_workspace_bytes(int64_t n, int32_t table_rows, int64_t* bytes) {
  if (!bytes || n < 0 || n > 0x7fffffffLL || table_rows <= 0)
    return set_error(HSTU_EINVAL, "hstu_embedding_rowwise_adagrad_workspace_bytes: bad arguments");
  *bytes = (int64_t)opt_layout(n, sort_temp(n, table_rows)).total;
  return HSTU_OK;
}

int hstu_embedding_grad_coalesce_workspace_bytes(int64_t n, int32_t table_rows, int64_t* bytes) {
  if (!bytes || n < 0 || n > 0x7fffffffLL || table_rows <= 0)
    return set_error(HSTU_EINVAL, "hstu_embedding_grad_coalesce_workspace_bytes: bad arguments");
  *bytes = (int64_t)coalesce_layout(n, sort_temp(n, table_rows)).total;
  return HSTU_OK;
}

// What every entry point that walks gradient rows takes, and the part they share: the checks, the carving of the workspace
// and the sort.  max_row_bytes: the widest dout row the entry point takes; out: the rows it writes with 16-byte stores (the
// table, or the coalesce's G); weight_dtype: fp32, or a 16-bit table written back by stochastic rounding; coalesce: the
// workspace is the coalesce's (rank and scan tiles behind the update's).
struct SparseCall {
  const char* what;
  int max_row_bytes;
  const void* dout;
  const int32_t* idx;
  int64_t n;
  int32_t dim, table_rows;
  void* out;
  int weight_dtype;
  void* workspace;
  int64_t workspace_bytes;
  int dtype;
  void* stream;
  bool coalesce;
};

// required_ok: the pointers named in `required` are there (checked first); outputs_ok: those that only a non-empty batch
// needs.  *go is false when there is nothing to launch.
static int sparse_begin(const SparseCall& c, bool required_ok, const char* required, bool outputs_ok, OptArgs* a, bool* go) {
  const char* what = c.what;
  *go = false;
  if (!required_ok || c.table_rows <= 0 || c.dim <= 0)
    return set_error(HSTU_EINVAL, "%s: %s must be non-NULL, sizes positive", what, required);
  if (!is_float_dtype(c.dtype)) return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32", what);
  if (c.weight_dtype != HSTU_DTYPE_F32 && c.dim % 8)
    return set_error(HSTU_EINVAL, "%s: 16-bit table rows must be 16-byte multiples (dim %d is not a multiple of 8)", what, c.dim);
  const int es = dtype_bytes(c.dtype);
  if (c.dim > kOptMaxDim)                           // before any product with dim: dim * es must not wrap
    return set_error(HSTU_EUNSUPPORTED, "%s: rows of %d columns > %d", what, c.dim, kOptMaxDim);
  if ((c.dim * es) % 16 || ((uintptr_t)c.dout & 15) || ((uintptr_t)c.out & 15))
    return set_error(HSTU_EINVAL, "%s: rows must be 16-byte multiples and 16-byte aligned", what);
  if (c.dim * es > c.max_row_bytes)
    return set_error(HSTU_EUNSUPPORTED, "%s: rows of %d bytes > %d", what, c.dim * es, c.max_row_bytes);
  if (c.n < 0 || c.n > 0x7fffffffLL) return set_error(HSTU_EINVAL, "%s: n out of range", what);
  if (c.n == 0) return HSTU_OK;
  if (!c.dout || !c.idx || !outputs_ok || !c.workspace) return set_error(HSTU_EINVAL, "%s: NULL input", what);
  const CoalesceLayout l = coalesce_layout(c.n, sort_temp(c.n, c.table_rows));
  if (c.workspace_bytes < (int64_t)(c.coalesce ? l.total : l.opt.total) || ((uintptr_t)c.workspace & 255))
    return set_error(HSTU_EINVAL, "%s: workspace too small or not 256-byte aligned (%s)", what,
                     c.coalesce ? "hstu_embedding_grad_coalesce_workspace_bytes" : "hstu_embedding_rowwise_adagrad_workspace_bytes");
  hipStream_t st = (hipStream_t)c.stream;
  char* ws = (char*)c.workspace;
  int32_t* sorted_idx = (int32_t*)ws;
  int32_t* perm = (int32_t*)(ws + l.opt.part);
  size_t temp = l.opt.temp_bytes;
  hipError_t e = sort_indices(ws + l.opt.temp_off, temp, c.idx, sorted_idx, perm, c.n, c.table_rows, st);
  if (e != hipSuccess) return set_error(HSTU_ELAUNCH, "%s: sort failed: %s", what, hipGetErrorString(e));
  *a = OptArgs{c.dout, perm, sorted_idx, c.n, c.dim, (float*)(ws + l.opt.partials_off), nullptr, nullptr, st};
  if (c.coalesce) {
    a->rank = (int32_t*)(ws + l.rank_off);
    a->tile_heads = (int32_t*)(ws + l.tiles_off);
  }
  *go = true;
  return HSTU_OK;
}

static int rowwise_adagrad_impl(const char* what, int max_row_bytes, const void* dout, const int32_t* idx, int64_t n, int32_t dim,
                                int32_t table_rows, void* weight, int weight_dtype, float* momentum1, float lr, float eps, uint64_t seed,
                                void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
  const SparseCall c{what, max_row_bytes, dout, idx, n, dim, table_rows, weight, weight_dtype, workspace, workspace_bytes, dtype, stream, false};
  OptArgs a;
  bool go;
  if (int rc = sparse_begin(c, weight && momentum1, "weight and momentum1", true, &a, &go)) return rc;
  if (!go) return HSTU_OK;
  return update_dispatch(weight_dtype, weight, AdagradRule{momentum1, lr, eps}, seed, dtype, a, what);
}

static bool is_table_dtype(int weight_dtype) {
  return weight_dtype == HSTU_DTYPE_F32 || weight_dtype == HSTU_DTYPE_F16 || weight_dtype == HSTU_DTYPE_BF16;
}

int hstu_embedding_sparse_sgd(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, void* weight,
                              int weight_dtype, float lr, uint64_t seed, void* workspace, int64_t workspace_bytes, int dtype,
                              void* stream) {
  const char* what = "hstu_embedding_sparse_sgd";
  if (!is_table_dtype(weight_dtype)) return set_error(HSTU_EINVAL, "%s: weight_dtype must be fp32, fp16 or bf16", what);
  const SparseCall c{what, max_row_bytes(dtype_bytes(dtype), true), dout, idx, n, dim, table_rows, weight, weight_dtype, workspace,
                     workspace_bytes, dtype, stream, false};
  OptArgs a;
  bool go;
  if (int rc = sparse_begin(c, weight != nullptr, "weight", true, &a, &go)) return rc;
  if (!go) return HSTU_OK;
  return update_dispatch(weight_dtype, weight, SgdRule{lr}, seed, dtype, a, what);
}

int hstu_embedding_sparse_adam(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, void* weight,
                               int weight_dtype, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                               int64_t step, uint64_t seed, void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
  const char* what = "hstu_embedding_sparse_adam";
  if (!is_table_dtype(weight_dtype)) return set_error(HSTU_EINVAL, "%s: weight_dtype must be fp32, fp16 or bf16", what);
  if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f))      // false for NaN
    return set_error(HSTU_EINVAL, "%s: beta1 and beta2 must lie in [0, 1), got %g and %g", what, (double)beta1, (double)beta2);
  if (step < 0) return set_error(HSTU_EINVAL, "%s: step must be >= 0 (the updates applied before this one)", what);
  if (((uintptr_t)exp_avg & 15) || ((uintptr_t)exp_avg_sq & 15))
    return set_error(HSTU_EINVAL, "%s: exp_avg and exp_avg_sq must be 16-byte aligned", what);
  const SparseCall c{what, max_row_bytes(dtype_bytes(dtype), true), dout, idx, n, dim, table_rows, weight, weight_dtype, workspace,
                     workspace_bytes, dtype, stream, false};
  OptArgs a;
  bool go;
  if (int rc = sparse_begin(c, weight && exp_avg && exp_avg_sq, "weight, exp_avg and exp_avg_sq", true, &a, &go)) return rc;
  if (!go) return HSTU_OK;
  // t = step + 1; the bias corrections in double, handed to the kernels as floats.  fp32 state rows of a dim that is a multiple
  // of 4 are 16-byte multiples (dim * es % 16 == 0 gives dim % 4 == 0 for every dout dtype)
  const double t = (double)step + 1.0;
  const float bc1 = (float)(1.0 - pow((double)beta1, t)), bc2 = (float)(1.0 - pow((double)beta2, t));
  const AdamCoef k{beta1, (float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2), lr / bc1, sqrtf(bc2), eps};
  return update_dispatch(weight_dtype, weight, AdamRule{exp_avg, exp_avg_sq, k}, seed, dtype, a, what);
}

int hstu_embedding_rowwise_adagrad(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, float* weight,
                                   float* momentum1, float lr, float eps, void* workspace, int64_t workspace_bytes, int dtype,
                                   void* stream) {
  return rowwise_adagrad_impl("hstu_embedding_rowwise_adagrad", max_row_bytes(dtype_bytes(dtype), false), dout, idx, n, dim, table_rows,
                              weight, HSTU_DTYPE_F32, momentum1, lr, eps, 0, workspace, workspace_bytes, dtype, stream);
}

int hstu_embedding_rowwise_adagrad_coalesced(const float* G, const int32_t* rows, int64_t n, int32_t dim, int32_t table_rows,
                                             float* weight, float* momentum1, float lr, float eps, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
  return rowwise_adagrad_impl("hstu_embedding_rowwise_adagrad_coalesced", max_row_bytes(4, true), G, rows, n, dim, table_rows, weight,
                              HSTU_DTYPE_F32, momentum1, lr, eps, 0, workspace, workspace_bytes, HSTU_DTYPE_F32, stream);
}

int hstu_embedding_rowwise_adagrad_lowp(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, void* weight,
                                        int weight_dtype, float* momentum1, float lr, float eps, uint64_t seed, void* workspace,
                                        int64_t workspace_bytes, int dtype, void* stream) {
  const char* what = "hstu_embedding_rowwise_adagrad_lowp";
  if (weight_dtype != HSTU_DTYPE_F16 && weight_dtype != HSTU_DTYPE_BF16)
    return set_error(HSTU_EINVAL, "%s: weight_dtype must be fp16 or bf16 (fp32 tables: hstu_embedding_rowwise_adagrad)", what);
  return rowwise_adagrad_impl(what, max_row_bytes(dtype_bytes(dtype), true), dout, idx, n, dim, table_rows, weight, weight_dtype,
                              momentum1, lr, eps, seed, workspace, workspace_bytes, dtype, stream);
}

int hstu_embedding_grad_coalesce(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, float scale,
                                 int32_t* rows, float* G, int32_t* count, void* workspace, int64_t workspace_bytes, int dtype,
                                 void* stream) {
  const char* what = "hstu_embedding_grad_coalesce";
  const SparseCall c{what, max_row_bytes(dtype_bytes(dtype), false), dout, idx, n, dim, table_rows, G, HSTU_DTYPE_F32, workspace,
                     workspace_bytes, dtype, stream, true};
  OptArgs a;
  bool go;
  if (int rc = sparse_begin(c, count != nullptr, "count", rows && G, &a, &go)) return rc;
  if (!go) {                                        // an empty batch: no segment heads
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t), (hipStream_t)stream);
    return e == hipSuccess ? HSTU_OK : set_error(HSTU_ELAUNCH, "%s: clearing count failed: %s", what, hipGetErrorString(e));
  }
  if (int rc = launch_head_ranks(a, plan(dtype_bytes(dtype), dim, n, false), count, what)) return rc;
  return opt_dispatch_dtype(dtype, a, EmitSink{rows, G, a.rank, scale}, what);
}

int hstu_stochastic_round(const float* src, const int32_t* row_ids, void* dst, int64_t n, int32_t dim, int dst_dtype, uint64_t seed,
                          void* stream) {
  const char* what = "hstu_stochastic_round";
  if (dst_dtype != HSTU_DTYPE_F16 && dst_dtype != HSTU_DTYPE_BF16) return set_error(HSTU_EINVAL, "%s: dst_dtype must be fp16 or bf16", what);
  if (n < 0 || dim <= 0) return set_error(HSTU_EINVAL, "%s: n must be >= 0 and dim positive", what);
  if (n == 0) return HSTU_OK;
  if (!src || !dst) return set_error(HSTU_EINVAL, "%s: NULL input", what);
  const bool wide = dim % 8 == 0 && !((uintptr_t)src & 15) && !((uintptr_t)dst & 15);
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kernel) {
    const int blocks = resident_row_blocks(kernel, kSrWaves * 64, 0, n, kSrWaves, 65535);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kSrWaves * 64), 0, st, src, row_ids, dst, n, dim, seed);
    return check_launch(what);
  };
  if (dst_dtype == HSTU_DTYPE_F16) return wide ? launch(stochastic_round_kernel<f16_t, 8>) : launch(stochastic_round_kernel<f16_t, 1>);
  return wide ? launch(stochastic_round_kernel<bf16_t, 8>) : launch(stochastic_round_kernel<bf16_t, 1>);
}

}  // extern "C"
