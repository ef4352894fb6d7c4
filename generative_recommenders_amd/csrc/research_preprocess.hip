// The input-feature preprocessors of the research path (gfx950, HBM-bound): one kernel template, three layouts.
//
//   hstu_input_preprocess_{fwd,bwd}   research/modeling/sequential/input_features_preprocessors.py:
//     PLAIN       LearnablePositionalEmbeddingInputFeaturesPreprocessor        (:72-89)
//     CONCAT      LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor   (:133-152)  columns >= Di are the rating row
//     INTERLEAVE  CombinedItemAndRatingInputFeaturesPreprocessor               (:226-260)  odd output rows are the rating row
//   out[b, n', c] = m(b, n) * drop(src * s + pos[n', c]),  s = fl32(sqrt(Do)),  m = past_ids[b, n] != 0
//   -- the reference's scale, (B, N, D) positional gather, add, dropout, mask multiply (and rating gather + cat) in one
//   read and one write.  fp32 keeps the reference's roundings (fl(src s), fl(. + pos), [fl(. scale)], fl(. m): four
//   separate operations, never an FMA), 16-bit I/O computes in fp32 and rounds at the store.
//
// Geometry: a thread owns one piece (V elements) of the (N', Do) plane of a user -- its position row, its column and its
// source are fixed -- and walks a slab of users; blockIdx.y picks the slab.  The forward therefore reads the position
// table once per slab, and the backward's d_pos is a per-thread running sum over the slab in user order: the partial
// of slab g goes to workspace[g], a second kernel adds the slabs in slab order.  d_rating re-reads the rating part of
// d_out: workgroup (slab of source rows, rating value) sums the rows of its slab that carry that rating, in row order,
// then the slabs are added in order and scaled by s.  No float atomics anywhere: both table gradients are bit-identical
// from run to run.  V is chosen once on the host: the widest of 8 / 4 / 2 / 1 elements (at most 16 bytes of the output
// dtype) that divides Do, Di and Dr and that the base pointers are aligned to.
#include <math.h>

#include "hstu_common.cuh"
#include "capi_internal.h"
#include "drop_hash.cuh"
#include "input_stage_dispatch.h"

// every product and sum below is its own rounding (the fp32 path restates the reference's op-by-op chain bit for bit): no
// FMA contraction in this file.  (__fmul_rn / __fadd_rn are plain operators in the HIP headers, parsed under the
// default contraction mode, so they would not keep the compiler from fusing them.)
#pragma clang fp contract(off)

namespace hstu {
namespace {
using namespace input_stage;      // kThreads and every grid, slab count, piece width and workspace size: input_stage_dispatch.h
static_assert(kLayoutPlain == HSTU_PREPROCESS_PLAIN, "input_stage_dispatch.h");

HSTU_DEV float mul_rn(float a, float b) { return a * b; }
HSTU_DEV float add_rn(float a, float b) { return a + b; }

// the fp32 value rounded to the stored dtype.  In the one-element fp16 kernels the value is pinned in its register first:
// there the compiler folds the product in front of the store into the conversion (one v_fma_mixlo_f16 with a +0 addend),
// which rounds once where fl16(fl32(.)) is promised and turns the -0 of a masked row into +0.  (The pin is an asm
// statement, which rules out a partial unroll: those kernels ask for none.)
template <typename T, int V> constexpr bool kPinned = V == 1 && __is_same(T, f16_t);
template <typename T, int V> constexpr int kUserUnroll = kPinned<T, V> ? 1 : 2;      // of the loop over a slab's users
template <typename T, int V>
HSTU_DEV T narrow(float x) {
  if constexpr (kPinned<T, V>) asm("" : "+v"(x));
  return (T)x;
}

template <typename T, int V> struct alignas(sizeof(T) * V) Pack { T e[V]; };
template <typename T, int V> HSTU_DEV Pack<T, V> load_pack(const T* p) { return *reinterpret_cast<const Pack<T, V>*>(p); }
template <typename T, int V> HSTU_DEV void store_pack(T* p, const Pack<T, V>& v) { *reinterpret_cast<Pack<T, V>*>(p) = v; }

struct PreArgs {
  const int64_t* ids;      // (B, N)
  const void* ratings;     // (B, N) int32 / int64, rated layouts only
  int r64;
  int B, N, Nout, Di, Dr, Do, R;
  float s;                 // fl32(sqrt(Do))
  uint32_t thr;            // 0: no dropout
  float scale;
  uint32_t s0, s1;
};

// bit i: element e0 + i survives (e0 a multiple of V when V > 1, so the V / 2 pairs are whole)
template <int V>
HSTU_DEV uint32_t keep_bits(uint64_t e0, const PreArgs& a) {
  if constexpr (V == 1) {
    return drop_r16(e0, a.s0, a.s1) >= a.thr ? 1u : 0u;
  } else {
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < V / 2; ++i) {
      const uint64_t pe = (e0 >> 1) + i;
      const uint32_t h = drop_hash((uint32_t)pe, drop_key((uint32_t)(pe >> 32), a.s0, a.s1), a.s0, a.s1);
      bits |= ((h & 0xffffu) >= a.thr ? 1u : 0u) << (2 * i);
      bits |= ((h >> 16) >= a.thr ? 1u : 0u) << (2 * i + 1);
    }
    return bits;
  }
}

HSTU_DEV int rating_of(const PreArgs& a, int64_t row) {
  int64_t r = load_index(a.ratings, row, a.r64);
  r = r < 0 ? 0 : (r >= a.R ? a.R - 1 : r);      // memory safety only: an out-of-range rating is the caller's error
  return (int)r;
}

// where piece j of the (N', Do) plane comes from
struct Piece {
  int np, n, c, cs;        // output row, source row, output column, column inside the source row
  bool rating;
};
template <int LAYOUT, int V>
HSTU_DEV Piece piece_of(int64_t j, int upr, const PreArgs& a) {
  Piece p;
  p.np = (int)(j / upr);
  p.c = (int)(j - (int64_t)p.np * upr) * V;
  p.n = LAYOUT == HSTU_PREPROCESS_INTERLEAVE ? p.np >> 1 : p.np;
  p.rating = LAYOUT == HSTU_PREPROCESS_CONCAT ? p.c >= a.Di : (LAYOUT == HSTU_PREPROCESS_INTERLEAVE ? (p.np & 1) != 0 : false);
  p.cs = (LAYOUT == HSTU_PREPROCESS_CONCAT && p.rating) ? p.c - a.Di : p.c;
  return p;
}

template <typename TE, typename TO, int LAYOUT, int V>
__global__ __launch_bounds__(kThreads) void input_preprocess_fwd_kernel(
    const TE* __restrict__ emb, const TO* __restrict__ pos, const TO* __restrict__ rat, TO* __restrict__ out,
    float* __restrict__ valid, const PreArgs a, int users_per_group) {
  const int upr = a.Do / V;
  const int64_t units = (int64_t)a.Nout * upr;
  const int b0 = blockIdx.y * users_per_group;
  const int b1 = min(b0 + users_per_group, a.B);
  for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < units; j += (int64_t)gridDim.x * kThreads) {
    const Piece p = piece_of<LAYOUT, V>(j, upr, a);
    const Pack<TO, V> pp = load_pack<TO, V>(pos + (int64_t)p.np * a.Do + p.c);
#pragma unroll kUserUnroll<TO, V>
    for (int b = b0; b < b1; ++b) {
      const int64_t row = (int64_t)b * a.N + p.n;
      const int64_t orow = (int64_t)b * a.Nout + p.np;
      const float m = a.ids[row] != 0 ? 1.f : 0.f;
      float x[V];
      if (p.rating) {
        const Pack<TO, V> q = load_pack<TO, V>(rat + (int64_t)rating_of(a, row) * a.Dr + p.cs);
#pragma unroll
        for (int i = 0; i < V; ++i) x[i] = (float)q.e[i];
      } else {
        const Pack<TE, V> q = load_pack<TE, V>(emb + row * a.Di + p.cs);
#pragma unroll
        for (int i = 0; i < V; ++i) x[i] = (float)q.e[i];
      }
      const int64_t e0 = orow * a.Do + p.c;
      const uint32_t kb = a.thr ? keep_bits<V>((uint64_t)e0, a) : 0u;
      Pack<TO, V> o;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float v = add_rn(mul_rn(x[i], a.s), (float)pp.e[i]);
        if (a.thr) v = ((kb >> i) & 1u) ? mul_rn(v, a.scale) : 0.f;
        o.e[i] = narrow<TO, V>(mul_rn(v, m));  // the product, not a select: the reference's masked rows keep their sign
      }
      store_pack<TO, V>(out + e0, o);
      if (p.c == 0) valid[orow] = m;
    }
  }
}

// d_emb = fl(h s) and the running sum of h over the slab's users; h = g m [keep scale]
template <typename TE, typename TO, int LAYOUT, int V>
__global__ __launch_bounds__(kThreads) void input_preprocess_bwd_kernel(
    const TO* __restrict__ g, TE* __restrict__ d_emb, float* __restrict__ partial, const PreArgs a, int users_per_group) {
  const int upr = a.Do / V;
  const int64_t units = (int64_t)a.Nout * upr;
  const int b0 = blockIdx.y * users_per_group;
  const int b1 = min(b0 + users_per_group, a.B);
  for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < units; j += (int64_t)gridDim.x * kThreads) {
    const Piece p = piece_of<LAYOUT, V>(j, upr, a);
    Pack<float, V> acc;
#pragma unroll
    for (int i = 0; i < V; ++i) acc.e[i] = 0.f;
#pragma unroll kUserUnroll<TE, V>
    for (int b = b0; b < b1; ++b) {
      const int64_t row = (int64_t)b * a.N + p.n;
      const int64_t e0 = ((int64_t)b * a.Nout + p.np) * a.Do + p.c;
      const float m = a.ids[row] != 0 ? 1.f : 0.f;
      const Pack<TO, V> gq = load_pack<TO, V>(g + e0);
      const uint32_t kb = a.thr ? keep_bits<V>((uint64_t)e0, a) : 0u;
      Pack<TE, V> o;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float h = mul_rn((float)gq.e[i], m);
        if (a.thr) h = ((kb >> i) & 1u) ? mul_rn(h, a.scale) : 0.f;
        acc.e[i] = add_rn(acc.e[i], h);
        o.e[i] = narrow<TE, V>(mul_rn(h, a.s));
      }
      if (d_emb && !p.rating) store_pack<TE, V>(d_emb + row * a.Di + p.cs, o);
    }
    if (partial) store_pack<float, V>(partial + ((int64_t)blockIdx.y * a.Nout + p.np) * a.Do + p.c, acc);
  }
}

// d_pos[idx] = sum over the slabs, in slab order; the rows of the table beyond N' are zero
__global__ __launch_bounds__(kThreads) void input_preprocess_pos_finish_kernel(const float* __restrict__ partial, int groups,
                                                                               int64_t width, int64_t total,
                                                                               float* __restrict__ d_pos) {
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
    float t = 0.f;
    if (idx < width)
      for (int k = 0; k < groups; ++k) t = add_rn(t, partial[k * width + idx]);
    d_pos[idx] = t;
  }
}

// partial[(group * R + r) * Dr + c] = the sum of h[row, rating column c] over the source rows of slab `group` with rating r.
// Threads are (rows in flight) x (lanes per row); a row slot adds its rows in row order, the slots are added in slot order.
template <typename TO, int LAYOUT, int V>
__global__ __launch_bounds__(kThreads) void input_preprocess_rating_bwd_kernel(const TO* __restrict__ g,
                                                                               float* __restrict__ partial, const PreArgs a) {
  __shared__ float red[kThreads][V + 1];
  const int units = a.Dr / V;
  const RowSlots s = row_slots(units, kThreads);
  const int u = blockIdx.z * s.tpr + s.lane;
  const bool live = u < units;
  const int c = u * V;
  const int want = blockIdx.y;
  int64_t r0, r1;
  slab_of((int64_t)a.B * a.N, &r0, &r1);
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.f;
  if (live) {
    for (int64_t r = r0 + s.slot; r < r1; r += s.rows_par) {
      if (a.ids[r] == 0 || rating_of(a, r) != want) continue;
      // CONCAT: output row r, columns Di + c; INTERLEAVE: output row b 2N + 2n + 1 = 2r + 1, columns c
      const int64_t e0 = LAYOUT == HSTU_PREPROCESS_CONCAT ? r * a.Do + a.Di + c : (2 * r + 1) * a.Do + c;
      const Pack<TO, V> gq = load_pack<TO, V>(g + e0);
      const uint32_t kb = a.thr ? keep_bits<V>((uint64_t)e0, a) : 0u;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float h = (float)gq.e[i];
        if (a.thr) h = ((kb >> i) & 1u) ? mul_rn(h, a.scale) : 0.f;
        acc[i] = add_rn(acc[i], h);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) red[threadIdx.x][i] = acc[i];
  __syncthreads();
  if (s.slot == 0 && live) {
    float* dst = partial + ((int64_t)blockIdx.x * a.R + want) * a.Dr + c;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float t = 0.f;
      for (int k = 0; k < s.rows_par; ++k) t = add_rn(t, red[k * s.tpr + s.lane][i]);
      dst[i] = t;
    }
  }
}

__global__ __launch_bounds__(kThreads) void input_preprocess_rating_finish_kernel(const float* __restrict__ partial, int groups,
                                                                                  int width, float s,
                                                                                  float* __restrict__ d_rating) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= width) return;
  float t = 0.f;
  for (int k = 0; k < groups; ++k) t = add_rn(t, partial[(int64_t)k * width + idx]);
  d_rating[idx] = mul_rn(t, s);
}

// ---------------------------------------------------------------------------------------------------- host side
// (Dims and everything decided from it: input_stage_dispatch.h)
int fill_dims(Dims* d, const char* what, int batch, int n, int item_dim, int rating_dim, int num_positions, int num_ratings,
              int layout) {
  if (layout != HSTU_PREPROCESS_PLAIN && layout != HSTU_PREPROCESS_CONCAT && layout != HSTU_PREPROCESS_INTERLEAVE)
    return set_error(HSTU_EINVAL, "%s: unknown layout %d", what, layout);
  if (batch < 0 || n < 0 || item_dim < 1 || num_positions < 0) return set_error(HSTU_EINVAL, "%s: negative size / empty rows", what);
  d->B = batch; d->N = n; d->Di = item_dim; d->P = num_positions; d->layout = layout;
  d->Dr = layout == HSTU_PREPROCESS_PLAIN ? 0 : rating_dim;
  d->R = layout == HSTU_PREPROCESS_PLAIN ? 0 : num_ratings;
  if (layout != HSTU_PREPROCESS_PLAIN && (rating_dim < 1 || num_ratings < 1 || num_ratings > 65535))
    return set_error(HSTU_EINVAL, "%s: the rated layouts need a rating table of 1 .. 65535 rows (got %d x %d)", what, num_ratings,
                     rating_dim);
  if (layout == HSTU_PREPROCESS_INTERLEAVE && rating_dim != item_dim)
    return set_error(HSTU_EINVAL, "%s: INTERLEAVE needs rating_dim == item_dim (got %d and %d)", what, rating_dim, item_dim);
  d->Do = layout == HSTU_PREPROCESS_CONCAT ? item_dim + rating_dim : item_dim;
  if (d->Do > HSTU_PREPROCESS_MAX_DIM || d->Do < 1)
    return set_error(HSTU_EUNSUPPORTED, "%s: rows of 1 .. %d columns (got %d)", what, HSTU_PREPROCESS_MAX_DIM, d->Do);
  const int64_t nout = layout == HSTU_PREPROCESS_INTERLEAVE ? 2 * (int64_t)n : n;
  if (nout > num_positions)
    return set_error(HSTU_EINVAL, "%s: %lld output positions but the position table has %d rows", what, (long long)nout,
                     num_positions);
  if ((int64_t)batch * nout > INT32_MAX) return set_error(HSTU_EINVAL, "%s: more than 2^31 - 1 output rows", what);
  d->Nout = (int)nout;
  return HSTU_OK;
}

int check_dtypes(const char* what, int emb_dtype, int out_dtype, int rating_index_dtype) {
  const bool e_ok = emb_dtype == HSTU_DTYPE_BF16 || emb_dtype == HSTU_DTYPE_F16 || emb_dtype == HSTU_DTYPE_F32;
  const bool o_ok = out_dtype == HSTU_DTYPE_BF16 || out_dtype == HSTU_DTYPE_F16 || out_dtype == HSTU_DTYPE_F32;
  if (!e_ok || !o_ok) return set_error(HSTU_EINVAL, "%s: dtypes must be bf16, fp16 or fp32", what);
  if (emb_dtype != out_dtype && out_dtype != HSTU_DTYPE_F32)
    return set_error(HSTU_EUNSUPPORTED, "%s: the output dtype is that of the embeddings, or fp32 (the promotion of a 16-bit "
                     "embedding into an fp32 module)", what);
  if (rating_index_dtype != HSTU_INDEX_I32 && rating_index_dtype != HSTU_INDEX_I64)
    return set_error(HSTU_EINVAL, "%s: ratings must be int32 or int64", what);
  return HSTU_OK;
}

PreArgs make_args(const Dims& d, const int64_t* ids, const void* ratings, int rating_index_dtype, float dropout_ratio,
                  uint64_t seed) {
  PreArgs a;
  a.ids = ids; a.ratings = ratings; a.r64 = rating_index_dtype == HSTU_INDEX_I64;
  a.B = d.B; a.N = d.N; a.Nout = d.Nout; a.Di = d.Di; a.Dr = d.Dr; a.Do = d.Do; a.R = d.R;
  a.s = (float)pow((double)d.Do, 0.5);
  a.thr = drop_threshold(dropout_ratio);
  a.scale = drop_scale(a.thr);
  a.s0 = (uint32_t)seed;
  a.s1 = (uint32_t)(seed >> 32);
  return a;
}

template <typename TE, typename TO, int LAYOUT, int V>
int fwd_launch(const Dims& d, const PreArgs& a, const void* emb, const void* pos, const void* rat, void* out, float* valid,
               hipStream_t st) {
  const int gx = unit_blocks(d, V);
  int upg;
  const dim3 grid(gx, slab_count(d.B, fwd_user_groups(d, gx), &upg));
  hipLaunchKernelGGL((input_preprocess_fwd_kernel<TE, TO, LAYOUT, V>), grid, dim3(kThreads), 0, st, (const TE*)emb,
                     (const TO*)pos, (const TO*)rat, (TO*)out, valid, a, upg);
  return check_launch("hstu_input_preprocess_fwd");
}

template <typename TE, typename TO, int LAYOUT, int V>
int bwd_launch(const Dims& d, const PreArgs& a, const void* g, void* d_emb, float* partial, hipStream_t st) {
  const int gx = unit_blocks(d, V);
  const int groups = partial ? bwd_groups(d) : fwd_user_groups(d, gx);
  int upg;
  const dim3 grid(gx, slab_count(d.B, groups, &upg));       // grid.y <= groups: the workspace holds `groups` slabs
  hipLaunchKernelGGL((input_preprocess_bwd_kernel<TE, TO, LAYOUT, V>), grid, dim3(kThreads), 0, st, (const TO*)g, (TE*)d_emb,
                     partial, a, upg);
  return check_launch("hstu_input_preprocess_bwd");
}

template <typename TO, int LAYOUT, int V>
int rating_launch(const Dims& d, const PreArgs& a, const void* g, float* partial, hipStream_t st) {
  const dim3 grid(rating_groups(d), d.R, rating_grid_z(d, V));
  hipLaunchKernelGGL((input_preprocess_rating_bwd_kernel<TO, LAYOUT, V>), grid, dim3(kThreads), 0, st, (const TO*)g, partial, a);
  return check_launch("hstu_input_preprocess_bwd(rating)");
}

// (embedding dtype, output dtype, layout, V) -> instantiation
#define PRE_BY_VEC(FN, ...)                                                            \
  switch (V) {                                                                         \
    case 8:                                                                            \
      if constexpr (sizeof(TO) == 2) return FN<TE, TO, LAYOUT, 8>(__VA_ARGS__);        \
      else return set_error(HSTU_EINVAL, "input_preprocess: 8 fp32 elements per piece"); \
    case 4: return FN<TE, TO, LAYOUT, 4>(__VA_ARGS__);                                 \
    case 2: return FN<TE, TO, LAYOUT, 2>(__VA_ARGS__);                                 \
    default: return FN<TE, TO, LAYOUT, 1>(__VA_ARGS__);                                \
  }
#define PRE_BY_LAYOUT(FN, TE, TO, ...)                                                               \
  switch (d.layout) {                                                                                \
    case HSTU_PREPROCESS_CONCAT: return FN<TE, TO, HSTU_PREPROCESS_CONCAT>(__VA_ARGS__);             \
    case HSTU_PREPROCESS_INTERLEAVE: return FN<TE, TO, HSTU_PREPROCESS_INTERLEAVE>(__VA_ARGS__);     \
    default: return FN<TE, TO, HSTU_PREPROCESS_PLAIN>(__VA_ARGS__);                                  \
  }
#define PRE_BY_DTYPE(FN, ...)                                                                     \
  if (emb_dtype == out_dtype) {                                                                   \
    if (out_dtype == HSTU_DTYPE_BF16) { PRE_BY_LAYOUT(FN, bf16_t, bf16_t, __VA_ARGS__) }          \
    if (out_dtype == HSTU_DTYPE_F16) { PRE_BY_LAYOUT(FN, f16_t, f16_t, __VA_ARGS__) }             \
    PRE_BY_LAYOUT(FN, float, float, __VA_ARGS__)                                                  \
  }                                                                                               \
  if (emb_dtype == HSTU_DTYPE_BF16) { PRE_BY_LAYOUT(FN, bf16_t, float, __VA_ARGS__) }             \
  PRE_BY_LAYOUT(FN, f16_t, float, __VA_ARGS__)

template <typename TE, typename TO, int LAYOUT>
int fwd_by_vec(int V, const Dims& d, const PreArgs& a, const void* emb, const void* pos, const void* rat, void* out, float* valid,
               hipStream_t st) {
  PRE_BY_VEC(fwd_launch, d, a, emb, pos, rat, out, valid, st)
}
template <typename TE, typename TO, int LAYOUT>
int bwd_by_vec(int V, const Dims& d, const PreArgs& a, const void* g, void* d_emb, float* partial, hipStream_t st) {
  PRE_BY_VEC(bwd_launch, d, a, g, d_emb, partial, st)
}
template <typename TE, typename TO, int LAYOUT, int V>
int rating_launch_te(const Dims& d, const PreArgs& a, const void* g, float* partial, hipStream_t st) {
  return rating_launch<TO, LAYOUT, V>(d, a, g, partial, st);
}
template <typename TE, typename TO, int LAYOUT>
int rating_by_vec(int V, const Dims& d, const PreArgs& a, const void* g, float* partial, hipStream_t st) {
  if constexpr (LAYOUT == HSTU_PREPROCESS_PLAIN) {
    return HSTU_OK;
  } else {
    PRE_BY_VEC(rating_launch_te, d, a, g, partial, st)
  }
}

int fwd_dispatch(const Dims& d, const PreArgs& a, int V, int emb_dtype, int out_dtype, const void* emb, const void* pos,
                 const void* rat, void* out, float* valid, hipStream_t st) {
  PRE_BY_DTYPE(fwd_by_vec, V, d, a, emb, pos, rat, out, valid, st)
}

int bwd_dispatch(const Dims& d, const PreArgs& a, int V, int emb_dtype, int out_dtype, const void* g, void* d_emb,
                 float* partial, hipStream_t st) {
  PRE_BY_DTYPE(bwd_by_vec, V, d, a, g, d_emb, partial, st)
}

int rating_dispatch(const Dims& d, const PreArgs& a, int V, int out_dtype, const void* g, float* partial, hipStream_t st) {
  const int emb_dtype = out_dtype;
  PRE_BY_DTYPE(rating_by_vec, V, d, a, g, partial, st)
}

}  // namespace
}  // namespace hstu

using namespace hstu;

extern "C" {

size_t hstu_input_preprocess_bwd_workspace_bytes(int32_t batch, int32_t n, int32_t item_dim, int32_t rating_dim,
                                                 int32_t num_ratings, int layout) {
  Dims d;
  const int64_t nout = layout == HSTU_PREPROCESS_INTERLEAVE ? 2 * (int64_t)n : n;
  if (nout > INT32_MAX) return 0;
  if (fill_dims(&d, "hstu_input_preprocess_bwd_workspace_bytes", batch, n, item_dim, rating_dim, (int)nout, num_ratings, layout))
    return 0;
  return pos_partial_bytes(d) + rating_partial_bytes(d);
}

int hstu_input_preprocess_fwd(const int64_t* past_ids, const void* past_embeddings, const void* ratings, const void* pos_table,
                              const void* rating_table, void* out, float* valid_mask, int32_t batch, int32_t n,
                              int32_t item_dim, int32_t rating_dim, int32_t num_positions, int32_t num_ratings, int layout,
                              float dropout_ratio, uint64_t seed, int emb_dtype, int out_dtype, int rating_index_dtype,
                              void* stream) {
  const char* what = "hstu_input_preprocess_fwd";
  Dims d;
  if (int e = fill_dims(&d, what, batch, n, item_dim, rating_dim, num_positions, num_ratings, layout)) return e;
  if (int e = check_dtypes(what, emb_dtype, out_dtype, rating_index_dtype)) return e;
  if (!(dropout_ratio >= 0.f && dropout_ratio < 1.f)) return set_error(HSTU_EINVAL, "%s: dropout_ratio must be in [0, 1)", what);
  if (batch == 0 || n == 0) return HSTU_OK;
  if (!past_ids || !past_embeddings || !pos_table || !out || !valid_mask) return set_error(HSTU_EINVAL, "%s: NULL tensor", what);
  if (layout != HSTU_PREPROCESS_PLAIN && (!ratings || !rating_table))
    return set_error(HSTU_EINVAL, "%s: the rated layouts need ratings and the rating table", what);
  const PreArgs a = make_args(d, past_ids, ratings, rating_index_dtype, dropout_ratio, seed);
  const int V = pick_vec(d, dtype_bytes(emb_dtype), dtype_bytes(out_dtype), {past_embeddings}, {pos_table, rating_table, out});
  return fwd_dispatch(d, a, V, emb_dtype, out_dtype, past_embeddings, pos_table, rating_table, out, valid_mask,
                      (hipStream_t)stream);
}

int hstu_input_preprocess_bwd(const void* d_out, const int64_t* past_ids, const void* ratings, void* d_past_embeddings,
                              float* d_pos_table, float* d_rating_table, void* workspace, int32_t batch, int32_t n,
                              int32_t item_dim, int32_t rating_dim, int32_t num_positions, int32_t num_ratings, int layout,
                              float dropout_ratio, uint64_t seed, int emb_dtype, int out_dtype, int rating_index_dtype,
                              void* stream) {
  const char* what = "hstu_input_preprocess_bwd";
  Dims d;
  if (int e = fill_dims(&d, what, batch, n, item_dim, rating_dim, num_positions, num_ratings, layout)) return e;
  if (int e = check_dtypes(what, emb_dtype, out_dtype, rating_index_dtype)) return e;
  if (!(dropout_ratio >= 0.f && dropout_ratio < 1.f)) return set_error(HSTU_EINVAL, "%s: dropout_ratio must be in [0, 1)", what);
  if (layout == HSTU_PREPROCESS_PLAIN) d_rating_table = nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (batch == 0 || n == 0) {          // nothing flows: the table gradients are zero
    hipError_t e = hipSuccess;
    if (d_pos_table) e = hipMemsetAsync(d_pos_table, 0, (size_t)d.P * d.Do * sizeof(float), st);
    if (e == hipSuccess && d_rating_table) e = hipMemsetAsync(d_rating_table, 0, (size_t)d.R * d.Dr * sizeof(float), st);
    return e == hipSuccess ? HSTU_OK : set_error(HSTU_ELAUNCH, "%s: memset failed: %s", what, hipGetErrorString(e));
  }
  if (!d_out || !past_ids) return set_error(HSTU_EINVAL, "%s: NULL tensor", what);
  if (layout != HSTU_PREPROCESS_PLAIN && !ratings && d_rating_table) return set_error(HSTU_EINVAL, "%s: d_rating_table without ratings", what);
  if ((d_pos_table || d_rating_table) && (!workspace || ((uintptr_t)workspace & 31)))
    return set_error(HSTU_EINVAL, "%s: the table gradients need the workspace, 32-byte aligned", what);
  const PreArgs a = make_args(d, past_ids, ratings, rating_index_dtype, dropout_ratio, seed);
  float* pos_partial = d_pos_table ? (float*)workspace : nullptr;
  float* rating_partial = d_rating_table ? (float*)((char*)workspace + pos_partial_bytes(d)) : nullptr;
  const int V = pick_vec(d, dtype_bytes(emb_dtype), dtype_bytes(out_dtype), {d_past_embeddings}, {d_out, workspace});
  if (d_past_embeddings || d_pos_table) {
    if (int e = bwd_dispatch(d, a, V, emb_dtype, out_dtype, d_out, d_past_embeddings, pos_partial, st)) return e;
  }
  if (d_pos_table) {
    const int64_t width = (int64_t)d.Nout * d.Do, total = (int64_t)d.P * d.Do;
    int upg;
    const int gy = slab_count(d.B, bwd_groups(d), &upg);
    hipLaunchKernelGGL(input_preprocess_pos_finish_kernel, dim3(pos_finish_blocks(total)), dim3(kThreads), 0, st, pos_partial, gy,
                       width, total, d_pos_table);
    if (int e = check_launch("hstu_input_preprocess_bwd(pos finish)")) return e;
  }
  if (d_rating_table) {
    if (int e = rating_dispatch(d, a, V, out_dtype, d_out, rating_partial, st)) return e;
    const int width = d.R * d.Dr;
    hipLaunchKernelGGL(input_preprocess_rating_finish_kernel, dim3(rating_finish_blocks(width)), dim3(kThreads), 0, st,
                       rating_partial, rating_groups(d), width, a.s, d_rating_table);
    if (int e = check_launch("hstu_input_preprocess_bwd(rating finish)")) return e;
  }
  return HSTU_OK;
}

}  // extern "C"
