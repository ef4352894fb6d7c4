// The two row passes of DLRM-v3's input stage (gfx950, HBM-bound, bit-exact): pure index arithmetic plus at most one add.
//
//   hstu_action_encode_{fwd,bwd}        ActionEncoder.forward (modules/action_encoder.py:73-112): the bit test of every UIH
//                                       row against the action weights, the broadcast product with the embedding table, the
//                                       tiled target table, the cast and the concat_2D_jagged in ONE pass that writes the
//                                       (sum L, T * Da) result; backward = masked column sums in a fixed order.
//   hstu_combine_embeddings_{fwd,bwd}   ContextualInterleavePreprocessor.combine_embeddings
//                                       (modules/contextual_interleave_preprocessor.py:101-224): the stack / mask /
//                                       dense_to_jagged / boolean index / two concat_2D_jagged chain as one gather that writes
//                                       every output row and timestamp once; backward = the inverse gather.
//
// Geometry of all four: the grid is the resident workgroups (at most 8 per CU), every workgroup owns ONE contiguous slab of
// rows, its 256 threads split as (rows in flight) x (lanes per row) by row_slots.h.  The user of a row is found by one
// binary search over the offsets per row slot and then advanced linearly along the slab.  Rows are 16-byte pieces when the
// row bytes and the base pointers allow it (VEC), elements otherwise.  Everything the host decides -- grids, slab counts,
// the piece width, the workspace size -- comes from input_stage_dispatch.h, which a CPU test compiles alone.
#include "hstu_common.cuh"
#include "capi_internal.h"
#include "input_stage_dispatch.h"

namespace hstu {
using namespace input_stage;

constexpr int kActionMaxTypes = HSTU_ACTION_ENCODE_MAX_TYPES;
static_assert(kCombineSum == HSTU_COMBINE_SUM && kCombineInterleaveAll == HSTU_COMBINE_INTERLEAVE_ALL, "input_stage_dispatch.h");

template <typename T> struct Vec16;   // 16 bytes of T
template <> struct Vec16<bf16_t> { typedef bf16_t type __attribute__((ext_vector_type(8))); static constexpr int N = 8; };
template <> struct Vec16<f16_t> { typedef f16_t type __attribute__((ext_vector_type(8))); static constexpr int N = 8; };
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };

// N elements of T: one 16-byte piece (VEC) or one element
template <typename T, bool VEC> struct Piece {
  static constexpr int N = VEC ? Vec16<T>::N : 1;
  T e[N];
  static HSTU_DEV Piece load(const T* p) {
    Piece r;
    if constexpr (VEC) {
      const typename Vec16<T>::type v = __builtin_bit_cast(typename Vec16<T>::type, gload16(p));
#pragma unroll
      for (int i = 0; i < N; ++i) r.e[i] = v[i];
    } else {
      r.e[0] = *p;
    }
    return r;
  }
  static HSTU_DEV Piece zero() {
    Piece r;
#pragma unroll
    for (int i = 0; i < N; ++i) r.e[i] = (T)0.f;
    return r;
  }
  HSTU_DEV void store(T* p) const {
    if constexpr (VEC) {
      typename Vec16<T>::type v;
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = e[i];
      gstore16(p, __builtin_bit_cast(u32x4, v));
    } else {
      *p = e[0];
    }
  }
};

// N fp32 parameters times the row's 0 / 1 mask -> N elements of T (one rounding each).  The product, not a select: the
// reference multiplies the boolean into the table, so a masked-out entry is a zero that keeps the parameter's sign
template <typename T, bool VEC>
HSTU_DEV Piece<T, VEC> cast_piece(const float* p, float m) {
  Piece<T, VEC> r;
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < Piece<T, VEC>::N / 4; ++q) {
      const f32x4 v = *(const f32x4*)(p + 4 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i) r.e[4 * q + i] = (T)(m * v[i]);
    }
  } else {
    r.e[0] = (T)(m * p[0]);
  }
  return r;
}

// ------------------------------------------------------------------------------------------------ action encode
struct ActionArgs {
  int64_t weight[kActionMaxTypes];        // the combined action weights: one bit pattern per column block
  int64_t threshold[kActionMaxTypes];     // watchtime >= threshold[k] -> action |= threshold_weight[k]
  int64_t threshold_weight[kActionMaxTypes];
  int32_t num_types, num_thresholds;
};

HSTU_DEV int64_t effective_action(const int64_t* actions, const int64_t* watchtimes, const ActionArgs& a, int64_t row) {
  int64_t act = actions[row];
  if (a.num_thresholds > 0) {
    const int64_t w = watchtimes[row];
    for (int k = 0; k < a.num_thresholds; ++k)
      if (w >= a.threshold[k]) act |= a.threshold_weight[k];
  }
  return act;
}

// out (rows, num_types * da): a UIH row gets cast(table) in the column blocks whose bit is set and cast(0 * table)
// elsewhere, a target row cast(target_table)
template <typename T, bool VEC>
__global__ __launch_bounds__(kPreThreads) void action_encode_fwd_kernel(
    const int64_t* __restrict__ actions, const int64_t* __restrict__ watchtimes, const void* __restrict__ uih_off,
    const void* __restrict__ tgt_off, const float* __restrict__ table, const float* __restrict__ target_table,
    const ActionArgs a, T* __restrict__ out, int64_t rows, int64_t total_uih, int batch, int da, int is64) {
  constexpr int N = Piece<T, VEC>::N;
  const int width = a.num_types * da;
  const int units = width / N;
  const RowSlots s = row_slots(units, kPreThreads);
  int64_t r0, r1;
  slab_of(rows, &r0, &r1);
  int64_t r = r0 + s.slot;
  if (r >= r1) return;
  auto off = [&](int b) { return load_index(uih_off, b, is64) + load_index(tgt_off, b, is64); };
  int b = find_user(off, batch, r);
  for (; r < r1; r += s.rows_par) {
    while (b + 1 < batch && r >= off(b + 1)) ++b;
    const int64_t uo = load_index(uih_off, b, is64);
    const int64_t i = r - (uo + load_index(tgt_off, b, is64));
    const int64_t U = load_index(uih_off, b + 1, is64) - uo;
    const int64_t Tn = load_index(tgt_off, b + 1, is64) - load_index(tgt_off, b, is64);
    if (i < 0 || i >= U + Tn) continue;            // the offsets do not describe this row
    const bool target = i >= U;
    uint64_t mask = 0;
    if (!target) {
      if (uo + i >= total_uih) continue;
      const int64_t act = effective_action(actions, watchtimes, a, uo + i);
      for (int t = 0; t < a.num_types; ++t) mask |= (uint64_t)((act & a.weight[t]) > 0) << t;
    }
    T* o = out + r * (int64_t)width;
    for (int u = s.lane; u < units; u += s.tpr) {
      const int c = u * N;
      const Piece<T, VEC> p = target ? cast_piece<T, VEC>(target_table + c, 1.f)
                                     : cast_piece<T, VEC>(table + c, ((mask >> (c / da)) & 1) ? 1.f : 0.f);
      p.store(o + c);
    }
  }
}

// partial[(g * 2 + k) * width + c]: k = 0 the sum of d_out[row, c] over the UIH rows of slab g whose bit c / da is set,
// k = 1 over its target rows.  A row slot adds its rows in row order, the slots are added in slot order.
template <typename T, bool VEC>
__global__ __launch_bounds__(kPreThreads) void action_encode_bwd_kernel(
    const T* __restrict__ d_out, const int64_t* __restrict__ actions, const int64_t* __restrict__ watchtimes,
    const void* __restrict__ uih_off, const void* __restrict__ tgt_off, const ActionArgs a, float* __restrict__ partial,
    int64_t rows, int64_t total_uih, int batch, int da, int is64) {
  constexpr int N = Piece<T, VEC>::N;
  __shared__ float red[kPreThreads][2 * N + 1];
  const int width = a.num_types * da;
  const int units = width / N;
  const RowSlots s = row_slots(units, kPreThreads);
  const int u = blockIdx.y * s.tpr + s.lane;
  const bool live = u < units;
  const int c = u * N;
  const int64_t wbit = live ? a.weight[c / da] : 0;
  float acc[2][N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[0][e] = acc[1][e] = 0.f;
  int64_t r0, r1;
  slab_of(rows, &r0, &r1);
  int64_t r = r0 + s.slot;
  if (live && r < r1) {
    auto off = [&](int b) { return load_index(uih_off, b, is64) + load_index(tgt_off, b, is64); };
    int b = find_user(off, batch, r);
    for (; r < r1; r += s.rows_par) {
      while (b + 1 < batch && r >= off(b + 1)) ++b;
      const int64_t uo = load_index(uih_off, b, is64);
      const int64_t i = r - (uo + load_index(tgt_off, b, is64));
      const int64_t U = load_index(uih_off, b + 1, is64) - uo;
      const int64_t Tn = load_index(tgt_off, b + 1, is64) - load_index(tgt_off, b, is64);
      if (i < 0 || i >= U + Tn) continue;
      const bool target = i >= U;
      if (!target) {
        if (uo + i >= total_uih) continue;
        if (!((effective_action(actions, watchtimes, a, uo + i) & wbit) > 0)) continue;
      }
      const Piece<T, VEC> g = Piece<T, VEC>::load(d_out + r * (int64_t)width + c);
      if (target) {
#pragma unroll
        for (int e = 0; e < N; ++e) acc[1][e] += (float)g.e[e];
      } else {
#pragma unroll
        for (int e = 0; e < N; ++e) acc[0][e] += (float)g.e[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < N; ++e) {
    red[threadIdx.x][e] = acc[0][e];
    red[threadIdx.x][N + e] = acc[1][e];
  }
  __syncthreads();
  if (s.slot == 0 && live) {
    float* dst = partial + (int64_t)blockIdx.x * 2 * width + c;
#pragma unroll
    for (int e = 0; e < 2 * N; ++e) {
      float t = 0.f;
      for (int k = 0; k < s.rows_par; ++k) t += red[k * s.tpr + s.lane][e];
      dst[(e / N) * width + (e % N)] = t;
    }
  }
}

// d_table[c] = sum_g partial[g][0][c], d_target_table[c] = sum_g partial[g][1][c]: four running sums over g, a fixed order
__global__ __launch_bounds__(256) void action_encode_bwd_finish_kernel(const float* __restrict__ partial, int groups,
                                                                        int width, float* __restrict__ d_table,
                                                                        float* __restrict__ d_target_table) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * width) return;
  const float* p = partial + idx;
  const int64_t step = 2 * (int64_t)width;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int g = 0;
  for (; g + 3 < groups; g += 4) {
    s0 += p[g * step];
    s1 += p[(g + 1) * step];
    s2 += p[(g + 2) * step];
    s3 += p[(g + 3) * step];
  }
  for (; g < groups; ++g) s0 += p[g * step];
  const float t = (s0 + s1) + (s2 + s3);
  if (idx < width) d_table[idx] = t; else d_target_table[idx - width] = t;
}

static int fill_action_args(ActionArgs* a, const int64_t* weights, int num_types, const int64_t* thresholds,
                            const int64_t* threshold_weights, int num_thresholds, const char* what) {
  if (num_types < 1 || num_types > kActionMaxTypes)
    return set_error(HSTU_EINVAL, "%s: 1..%d action types (got %d)", what, kActionMaxTypes, num_types);
  if (num_thresholds < 0 || num_thresholds > kActionMaxTypes)
    return set_error(HSTU_EINVAL, "%s: 0..%d watchtime thresholds (got %d)", what, kActionMaxTypes, num_thresholds);
  if (!weights || (num_thresholds > 0 && (!thresholds || !threshold_weights)))
    return set_error(HSTU_EINVAL, "%s: the weights / thresholds are host arrays and must not be NULL", what);
  for (int t = 0; t < kActionMaxTypes; ++t) {
    a->weight[t] = t < num_types ? weights[t] : 0;
    a->threshold[t] = t < num_thresholds ? thresholds[t] : 0;
    a->threshold_weight[t] = t < num_thresholds ? threshold_weights[t] : 0;
  }
  a->num_types = num_types;
  a->num_thresholds = num_thresholds;
  return HSTU_OK;
}

static int check_sizes(const char* what, int64_t total_a, int64_t total_b, int batch, int dim, int dtype, int index_dtype) {
  if (total_a < 0 || total_b < 0 || batch < 0 || dim < 1) return set_error(HSTU_EINVAL, "%s: negative size / empty rows", what);
  if (!is_float_dtype(dtype)) return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32", what);
  if (index_dtype != HSTU_INDEX_I32 && index_dtype != HSTU_INDEX_I64)
    return set_error(HSTU_EINVAL, "%s: offsets must be int32 or int64", what);
  if (total_a > INT32_MAX || total_b > INT32_MAX || total_a + total_b > INT32_MAX)
    return set_error(HSTU_EINVAL, "%s: more than 2^31 - 1 rows", what);
  return HSTU_OK;
}

template <typename T>
static int action_fwd_t(const int64_t* actions, const int64_t* watchtimes, const void* uo, const void* to, const float* table,
                        const float* target_table, const ActionArgs& a, void* out, int64_t rows, int64_t total_uih, int batch,
                        int da, int is64, hipStream_t st) {
  const int piece = action_fwd_piece(da, sizeof(T), table, target_table, out);
  const dim3 grid(resident_blocks(rows, rows_in_flight(a.num_types * da / piece, kPreThreads), cu_count()));
  if (piece > 1)
    hipLaunchKernelGGL((action_encode_fwd_kernel<T, true>), grid, dim3(kPreThreads), 0, st, actions, watchtimes, uo, to, table,
                       target_table, a, (T*)out, rows, total_uih, batch, da, is64);
  else
    hipLaunchKernelGGL((action_encode_fwd_kernel<T, false>), grid, dim3(kPreThreads), 0, st, actions, watchtimes, uo, to, table,
                       target_table, a, (T*)out, rows, total_uih, batch, da, is64);
  return check_launch("hstu_action_encode_fwd");
}

template <typename T>
static int action_bwd_t(const void* d_out, const int64_t* actions, const int64_t* watchtimes, const void* uo, const void* to,
                        const ActionArgs& a, float* d_table, float* d_target, float* partial, int64_t rows, int64_t total_uih,
                        int batch, int da, int is64, hipStream_t st) {
  const int width = a.num_types * da;
  const int piece = action_bwd_piece(da, sizeof(T), d_out, partial);
  const int units = width / piece;
  const int groups = action_bwd_groups(rows, units, cu_count());
  const dim3 grid(groups, action_bwd_grid_y(units));
  if (piece > 1)
    hipLaunchKernelGGL((action_encode_bwd_kernel<T, true>), grid, dim3(kPreThreads), 0, st, (const T*)d_out, actions, watchtimes,
                       uo, to, a, partial, rows, total_uih, batch, da, is64);
  else
    hipLaunchKernelGGL((action_encode_bwd_kernel<T, false>), grid, dim3(kPreThreads), 0, st, (const T*)d_out, actions, watchtimes,
                       uo, to, a, partial, rows, total_uih, batch, da, is64);
  if (int e = check_launch("hstu_action_encode_bwd")) return e;
  hipLaunchKernelGGL(action_encode_bwd_finish_kernel, dim3(action_bwd_finish_blocks(width)), dim3(256), 0, st, partial, groups, width,
                     d_table, d_target);
  return check_launch("hstu_action_encode_bwd(finish)");
}

// ------------------------------------------------------------------------------------------------ combine
// the output position (behind the contextual rows) of source row i of a user with L rows, U of them UIH
HSTU_DEV int content_pos(int mode, int i, int U) {
  if (mode == HSTU_COMBINE_SUM) return i;
  if (mode == HSTU_COMBINE_INTERLEAVE_ALL || i < U) return 2 * i;
  return 2 * U + (i - U);
}

HSTU_DEV int user_uih_len(const void* num_targets, int b, int L, int mode, int is64) {
  if (mode != HSTU_COMBINE_INTERLEAVE_UIH) return L;
  int64_t t = load_index(num_targets, b, is64);
  t = t < 0 ? 0 : (t > L ? L : t);
  return L - (int)t;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kPreThreads) void combine_fwd_kernel(
    const T* __restrict__ content, const T* __restrict__ action, const T* __restrict__ contextual,
    const int64_t* __restrict__ timestamps, const void* __restrict__ seq_off, const void* __restrict__ num_targets,
    const void* __restrict__ out_off, T* __restrict__ out, int64_t* __restrict__ out_ts, int64_t total_rows, int64_t out_rows,
    int batch, int C, int D, int mode, int is64) {
  constexpr int N = Piece<T, VEC>::N;
  const int units = D / N;
  const RowSlots s = row_slots(units, kPreThreads);
  int64_t r0, r1;
  slab_of(out_rows, &r0, &r1);
  int64_t r = r0 + s.slot;
  if (r >= r1) return;
  auto oo = [&](int b) { return load_index(out_off, b, is64); };
  int b = find_user(oo, batch, r);
  for (; r < r1; r += s.rows_par) {
    while (b + 1 < batch && r >= oo(b + 1)) ++b;
    const int64_t j = r - oo(b);
    if (j < 0) continue;
    T* o = out + r * (int64_t)D;
    if (j < C) {
      const T* src = contextual + ((int64_t)b * C + j) * D;
      for (int u = s.lane; u < units; u += s.tpr) Piece<T, VEC>::load(src + u * N).store(o + u * N);
      if (s.lane == 0) out_ts[r] = 0;
      continue;
    }
    const int64_t so = load_index(seq_off, b, is64);
    const int64_t L64 = load_index(seq_off, b + 1, is64) - so;
    const int64_t p = j - C;
    if (L64 <= 0 || L64 > INT32_MAX || p >= 2 * L64) continue;     // the offsets do not describe this row
    const int L = (int)L64;
    int i;
    bool odd = false;
    if (mode == HSTU_COMBINE_SUM) {
      i = (int)p;
    } else {
      const int U = user_uih_len(num_targets, b, L, mode, is64);
      if (p < 2 * (int64_t)U) { i = (int)(p >> 1); odd = p & 1; }
      else i = U + (int)(p - 2 * (int64_t)U);
    }
    if (i >= L || so + i >= total_rows || so + i < 0) continue;
    const int64_t sr = so + i;
    if (mode == HSTU_COMBINE_SUM && action) {
      const T* x = content + sr * D;
      const T* y = action + sr * D;
      for (int u = s.lane; u < units; u += s.tpr) {
        const Piece<T, VEC> px = Piece<T, VEC>::load(x + u * N), py = Piece<T, VEC>::load(y + u * N);
        Piece<T, VEC> q;
#pragma unroll
        for (int e = 0; e < N; ++e) q.e[e] = (T)((float)px.e[e] + (float)py.e[e]);
        q.store(o + u * N);
      }
    } else {
      const T* src = (odd ? action : content) + sr * D;
      for (int u = s.lane; u < units; u += s.tpr) Piece<T, VEC>::load(src + u * N).store(o + u * N);
    }
    if (s.lane == 0) out_ts[r] = timestamps[sr];
  }
}

// rows [0, total_rows): source row -> d_content (and d_action); rows [total_rows, total_rows + batch * C): d_contextual
template <typename T, bool VEC>
__global__ __launch_bounds__(kPreThreads) void combine_bwd_kernel(
    const T* __restrict__ d_out, const void* __restrict__ seq_off, const void* __restrict__ num_targets,
    const void* __restrict__ out_off, T* __restrict__ d_content, T* __restrict__ d_action, T* __restrict__ d_contextual,
    int64_t total_rows, int64_t out_rows, int batch, int C, int D, int mode, int is64) {
  constexpr int N = Piece<T, VEC>::N;
  const int units = D / N;
  const RowSlots s = row_slots(units, kPreThreads);
  const int64_t ctx_rows = d_contextual ? (int64_t)batch * C : 0;
  int64_t r0, r1;
  slab_of(total_rows + ctx_rows, &r0, &r1);
  int64_t r = r0 + s.slot;
  if (r >= r1) return;
  auto so = [&](int b) { return load_index(seq_off, b, is64); };
  int b = r < total_rows ? find_user(so, batch, r) : 0;
  for (; r < r1; r += s.rows_par) {
    if (r >= total_rows) {
      const int64_t q = r - total_rows;
      const int ub = (int)(q / C);
      const int64_t g = load_index(out_off, ub, is64) + (q % C);
      if (g < 0 || g >= out_rows) continue;
      for (int u = s.lane; u < units; u += s.tpr) Piece<T, VEC>::load(d_out + g * D + u * N).store(d_contextual + q * D + u * N);
      continue;
    }
    while (b + 1 < batch && r >= so(b + 1)) ++b;
    const int64_t i64 = r - so(b);
    const int64_t L64 = so(b + 1) - so(b);
    if (i64 < 0 || i64 >= L64 || L64 > INT32_MAX) continue;
    const int i = (int)i64, L = (int)L64;
    const int U = user_uih_len(num_targets, b, L, mode, is64);
    const int64_t gc = load_index(out_off, b, is64) + C + content_pos(mode, i, U);
    if (gc < 0 || gc >= out_rows) continue;
    // SUM: the action row read the same output row; interleaved: the next one, and a target row of INTERLEAVE_UIH none
    const bool act_zero = mode == HSTU_COMBINE_INTERLEAVE_UIH && i >= U;
    const int64_t ga = mode == HSTU_COMBINE_SUM ? gc : gc + 1;
    const bool act = d_action && !act_zero && ga < out_rows;
    for (int u = s.lane; u < units; u += s.tpr) {
      const Piece<T, VEC> pc = Piece<T, VEC>::load(d_out + gc * D + u * N);
      pc.store(d_content + r * D + u * N);
      if (d_action) {
        Piece<T, VEC> pa = pc;
        if (!act) pa = Piece<T, VEC>::zero();
        else if (ga != gc) pa = Piece<T, VEC>::load(d_out + ga * D + u * N);
        pa.store(d_action + r * D + u * N);
      }
    }
  }
}

template <typename T>
static int combine_fwd_t(const void* content, const void* action, const void* contextual, const int64_t* ts, const void* seq_off,
                         const void* nt, const void* out_off, void* out, int64_t* out_ts, int64_t total_rows, int64_t out_rows,
                         int batch, int C, int D, int mode, int is64, hipStream_t st) {
  const int piece = combine_fwd_piece(D, sizeof(T), content, action, contextual, out);
  const dim3 grid(resident_blocks(out_rows, rows_in_flight(D / piece, kPreThreads), cu_count()));
#define LAUNCH(V)                                                                                                             \
  hipLaunchKernelGGL((combine_fwd_kernel<T, V>), grid, dim3(kPreThreads), 0, st, (const T*)content, (const T*)action,           \
                     (const T*)contextual, ts, seq_off, nt, out_off, (T*)out, out_ts, total_rows, out_rows, batch, C, D, mode,  \
                     is64)
  if (piece > 1) LAUNCH(true); else LAUNCH(false);
#undef LAUNCH
  return check_launch("hstu_combine_embeddings_fwd");
}

template <typename T>
static int combine_bwd_t(const void* d_out, const void* seq_off, const void* nt, const void* out_off, void* d_content,
                         void* d_action, void* d_contextual, int64_t total_rows, int64_t out_rows, int batch, int C, int D,
                         int mode, int is64, hipStream_t st) {
  const int piece = combine_bwd_piece(D, sizeof(T), d_out, d_content, d_action, d_contextual);
  const int64_t rows = combine_bwd_rows(total_rows, batch, C, d_contextual != nullptr);
  const dim3 grid(resident_blocks(rows, rows_in_flight(D / piece, kPreThreads), cu_count()));
#define LAUNCH(V)                                                                                                            \
  hipLaunchKernelGGL((combine_bwd_kernel<T, V>), grid, dim3(kPreThreads), 0, st, (const T*)d_out, seq_off, nt, out_off,        \
                     (T*)d_content, (T*)d_action, (T*)d_contextual, total_rows, out_rows, batch, C, D, mode, is64)
  if (piece > 1) LAUNCH(true); else LAUNCH(false);
#undef LAUNCH
  return check_launch("hstu_combine_embeddings_bwd");
}

}  // namespace hstu

using namespace hstu;

#define PRE_DISPATCH(dtype, CALL)                      \
  switch (dtype) {                                     \
    case HSTU_DTYPE_BF16: { typedef bf16_t T; return CALL; } \
    case HSTU_DTYPE_F16: { typedef f16_t T; return CALL; }   \
    default: { typedef float T; return CALL; }               \
  }

// The argument checks that the forward and the backward of an op share, in the order both make them.  *empty: the call has
// nothing to launch and the offsets were not looked at -- the caller returns HSTU_OK (the action backward after zero-filling
// its tables, which is why `tables`, that d_table / d_target_table are there, is checked in front; the forward passes true).
static int check_action_call(const char* what, ActionArgs* a, const int64_t* weights, int num_types, const int64_t* thresholds,
                             const int64_t* threshold_weights, int num_thresholds, const void* uih_offsets,
                             const void* target_offsets, int64_t total_uih_len, int64_t total_targets, int batch,
                             int embedding_dim, int dtype, int index_dtype, bool tables, bool* empty) {
  if (int e = fill_action_args(a, weights, num_types, thresholds, threshold_weights, num_thresholds, what)) return e;
  if (int e = check_sizes(what, total_uih_len, total_targets, batch, embedding_dim, dtype, index_dtype)) return e;
  if ((int64_t)num_types * embedding_dim > (1 << 24)) return set_error(HSTU_EINVAL, "%s: rows of more than 2^24 columns", what);
  if (!tables) return set_error(HSTU_EINVAL, "%s: d_table / d_target_table are required", what);
  *empty = batch == 0 || total_uih_len + total_targets == 0;
  if (*empty) return HSTU_OK;
  if (!uih_offsets || !target_offsets) return set_error(HSTU_EINVAL, "%s: the offsets are NULL", what);
  return HSTU_OK;
}

static int check_combine_call(const char* what, int mode, int contextual_len, int64_t total_uih_len, int64_t total_targets,
                              int batch, int dim, int dtype, int index_dtype, const void* seq_offsets, const void* out_offsets,
                              const void* num_targets, int64_t* out_rows, bool* empty) {
  if (mode != HSTU_COMBINE_SUM && mode != HSTU_COMBINE_INTERLEAVE_ALL && mode != HSTU_COMBINE_INTERLEAVE_UIH)
    return set_error(HSTU_EINVAL, "%s: unknown mode %d", what, mode);
  if (contextual_len < 0) return set_error(HSTU_EINVAL, "%s: negative contextual length", what);
  if (int e = check_sizes(what, total_uih_len, total_targets, batch, dim, dtype, index_dtype)) return e;
  *out_rows = combine_out_rows(mode, total_uih_len, total_targets, batch, contextual_len);
  if (*out_rows > INT32_MAX) return set_error(HSTU_EINVAL, "%s: more than 2^31 - 1 output rows", what);
  *empty = batch == 0 || *out_rows == 0;
  if (*empty) return HSTU_OK;
  if (!seq_offsets || !out_offsets) return set_error(HSTU_EINVAL, "%s: the offsets are NULL", what);
  if (mode == HSTU_COMBINE_INTERLEAVE_UIH && !num_targets) return set_error(HSTU_EINVAL, "%s: INTERLEAVE_UIH needs num_targets", what);
  return HSTU_OK;
}

extern "C" {

size_t hstu_action_encode_bwd_workspace_bytes(int64_t total_rows, int32_t width) {
  (void)total_rows;
  return action_bwd_workspace_bytes(width);
}

int hstu_action_encode_fwd(const int64_t* actions, const int64_t* watchtimes, const void* uih_offsets, const void* target_offsets,
                           const float* table, const float* target_table, const int64_t* weights, int32_t num_types,
                           const int64_t* thresholds, const int64_t* threshold_weights, int32_t num_thresholds, void* out,
                           int64_t total_uih_len, int64_t total_targets, int32_t batch, int32_t embedding_dim, int dtype,
                           int index_dtype, void* stream) {
  const char* what = "hstu_action_encode_fwd";
  ActionArgs a;
  bool empty;
  if (int e = check_action_call(what, &a, weights, num_types, thresholds, threshold_weights, num_thresholds, uih_offsets,
                                target_offsets, total_uih_len, total_targets, batch, embedding_dim, dtype, index_dtype, true, &empty))
    return e;
  if (empty) return HSTU_OK;
  const int64_t rows = total_uih_len + total_targets;
  if (!table || !target_table || !out || (total_uih_len > 0 && !actions) || (total_uih_len > 0 && num_thresholds > 0 && !watchtimes))
    return set_error(HSTU_EINVAL, "%s: NULL tensor", what);
  hipStream_t st = (hipStream_t)stream;
  const int is64 = index_dtype == HSTU_INDEX_I64;
  PRE_DISPATCH(dtype, (action_fwd_t<T>(actions, watchtimes, uih_offsets, target_offsets, table, target_table, a, out, rows,
                                       total_uih_len, batch, embedding_dim, is64, st)));
}

int hstu_action_encode_bwd(const void* d_out, const int64_t* actions, const int64_t* watchtimes, const void* uih_offsets,
                           const void* target_offsets, const int64_t* weights, int32_t num_types, const int64_t* thresholds,
                           const int64_t* threshold_weights, int32_t num_thresholds, float* d_table, float* d_target_table,
                           void* workspace, int64_t total_uih_len, int64_t total_targets, int32_t batch, int32_t embedding_dim,
                           int dtype, int index_dtype, void* stream) {
  const char* what = "hstu_action_encode_bwd";
  ActionArgs a;
  bool empty;
  if (int e = check_action_call(what, &a, weights, num_types, thresholds, threshold_weights, num_thresholds, uih_offsets,
                                target_offsets, total_uih_len, total_targets, batch, embedding_dim, dtype, index_dtype,
                                d_table && d_target_table, &empty))
    return e;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = total_uih_len + total_targets;
  const size_t bytes = (size_t)num_types * embedding_dim * sizeof(float);
  if (empty) {
    hipError_t e = hipMemsetAsync(d_table, 0, bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_target_table, 0, bytes, st);
    return e == hipSuccess ? HSTU_OK : set_error(HSTU_ELAUNCH, "%s: memset failed: %s", what, hipGetErrorString(e));
  }
  if (!d_out || !workspace || (total_uih_len > 0 && !actions) || (total_uih_len > 0 && num_thresholds > 0 && !watchtimes))
    return set_error(HSTU_EINVAL, "%s: NULL tensor / workspace", what);
  const int is64 = index_dtype == HSTU_INDEX_I64;
  PRE_DISPATCH(dtype, (action_bwd_t<T>(d_out, actions, watchtimes, uih_offsets, target_offsets, a, d_table, d_target_table,
                                       (float*)workspace, rows, total_uih_len, batch, embedding_dim, is64, st)));
}

int hstu_combine_embeddings_fwd(const void* content, const void* action, const void* contextual, const int64_t* timestamps,
                                const void* seq_offsets, const void* num_targets, const void* out_offsets, void* out,
                                int64_t* out_timestamps, int64_t total_uih_len, int64_t total_targets, int32_t batch,
                                int32_t contextual_len, int32_t dim, int mode, int dtype, int index_dtype, void* stream) {
  const char* what = "hstu_combine_embeddings_fwd";
  int64_t out_rows;
  bool empty;
  if (int e = check_combine_call(what, mode, contextual_len, total_uih_len, total_targets, batch, dim, dtype, index_dtype,
                                 seq_offsets, out_offsets, num_targets, &out_rows, &empty))
    return e;
  if (empty) return HSTU_OK;
  if (mode != HSTU_COMBINE_SUM && !action) return set_error(HSTU_EINVAL, "%s: interleaving needs the action rows", what);
  const int64_t total = total_uih_len + total_targets;
  if (!out || !out_timestamps || (total > 0 && (!content || !timestamps)) || (contextual_len > 0 && !contextual))
    return set_error(HSTU_EINVAL, "%s: NULL tensor", what);
  hipStream_t st = (hipStream_t)stream;
  const int is64 = index_dtype == HSTU_INDEX_I64;
  PRE_DISPATCH(dtype, (combine_fwd_t<T>(content, action, contextual, timestamps, seq_offsets, num_targets, out_offsets, out,
                                        out_timestamps, total, out_rows, batch, contextual_len, dim, mode, is64, st)));
}

int hstu_combine_embeddings_bwd(const void* d_out, const void* seq_offsets, const void* num_targets, const void* out_offsets,
                                void* d_content, void* d_action, void* d_contextual, int64_t total_uih_len, int64_t total_targets,
                                int32_t batch, int32_t contextual_len, int32_t dim, int mode, int dtype, int index_dtype,
                                void* stream) {
  const char* what = "hstu_combine_embeddings_bwd";
  int64_t out_rows;
  bool empty;
  if (int e = check_combine_call(what, mode, contextual_len, total_uih_len, total_targets, batch, dim, dtype, index_dtype,
                                 seq_offsets, out_offsets, num_targets, &out_rows, &empty))
    return e;
  if (empty) return HSTU_OK;
  const int64_t total = total_uih_len + total_targets;
  if (!d_out || (total > 0 && !d_content)) return set_error(HSTU_EINVAL, "%s: NULL tensor", what);
  if (contextual_len == 0) d_contextual = nullptr;
  if (total == 0 && !d_contextual) return HSTU_OK;
  hipStream_t st = (hipStream_t)stream;
  const int is64 = index_dtype == HSTU_INDEX_I64;
  PRE_DISPATCH(dtype, (combine_bwd_t<T>(d_out, seq_offsets, num_targets, out_offsets, d_content, d_action, d_contextual, total,
                                        out_rows, batch, contextual_len, dim, mode, is64, st)));
}

}  // extern "C"
