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
#include "hstu_common.cuh"
#include "capi_internal.h"
#include "embedding_sort.cuh"

namespace hstu {

constexpr int kOptWaves = 4;
constexpr int kChunkLarge = 128;       // sorted rows per wave of the chunk kernel: two coalesced loads of the (id, row) pairs
constexpr int kChunkSmall = 32;        // below kSmallBatch ids: four times the waves, a quarter of the groups each walks
constexpr int64_t kSmallBatch = 262144;
constexpr int kSmallChunkMaxDim = 512; // four times the partial sums of a quarter of the widest row: the same workspace
constexpr int kCombineWaves = 8;       // waves that share one cut segment's partial sums
constexpr int kOptMaxPieces = 4;       // 16-byte pieces per lane and dout row: rows of up to 4 KiB
constexpr int kOptMaxDim = 2048;       // 4 KiB of bf16 / fp16: the widest partial sum (8 KiB of fp32)
constexpr int kOptMaxBlocks = 8192;    // grid-stride above this

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

// the update of one finished segment: acc = G[r, :], w = W[r, :] (loaded by the caller ahead of time), m_old =
// momentum1[r].  The squares are added pairwise inside the lane and by a butterfly across the wave: log2(dim) levels.
template <int VEC, int NP>
__device__ __forceinline__ void apply_update(const float (&acc)[NP][VEC], float (&w)[NP][VEC], float m_old, int lane, int pieces, int dim,
                                             float* __restrict__ w_row, float* __restrict__ m_ptr, float lr, float eps) {
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
#pragma unroll
  for (int s = 1; s < NP; s *= 2)
#pragma unroll
    for (int j = 0; j + s < NP; j += 2 * s) sq[j][0] += sq[j + s][0];
  float ss = sq[0][0];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
  const float m_new = m_old + ss / (float)dim;
  const float step = lr / (sqrtf(m_new) + eps);
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int c = 0; c < VEC; ++c) w[j][c] -= step * acc[j][c];
  store_f32_row<VEC, NP>(w_row, lane, pieces, w);
  if (lane == 0) *m_ptr = m_new;
}

template <typename T, int NP, int U, int kChunk>
__global__ __launch_bounds__(kOptWaves * 64) void adagrad_chunk_kernel(const T* __restrict__ g, const int32_t* __restrict__ perm,
                                                                       const int32_t* __restrict__ sorted_idx, int64_t n, int dim,
                                                                       float* __restrict__ weight, float* __restrict__ momentum1,
                                                                       float* __restrict__ partials, float lr, float eps) {
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
      float w[U][NP][VEC], m_old[U];
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
        m_old[u] = 0.f;
        if (whole[u]) {                             // the table row travels with the gradient rows
          load_f32_row<VEC, NP>(weight + (int64_t)id[u] * dim, lane, pieces, w[u]);
          m_old[u] = momentum1[id[u]];
        }
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
            apply_update<VEC, NP>(acc, w[u], m_old[u], lane, pieces, dim, weight + (int64_t)id[u] * dim, momentum1 + id[u], lr, eps);
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
template <int VEC, int NP, int kChunk>
__global__ __launch_bounds__(kCombineWaves * 64) void adagrad_combine_kernel(const int32_t* __restrict__ sorted_idx, int64_t n, int dim,
                                                                             float* __restrict__ weight, float* __restrict__ momentum1,
                                                                             const float* __restrict__ partials, float lr, float eps) {
  extern __shared__ __attribute__((aligned(16))) float shares[];       // (kCombineWaves - 1) rows of dim floats
  constexpr int U = NP * VEC >= 32 ? 2 : NP * VEC >= 16 ? 4 : 8;   // partial sums in flight: 64 registers
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
    float* w_row = weight + (int64_t)id * dim;
    float w[NP][VEC], acc[NP][VEC];
    float m_old = 0.f;
    if (wave == 0) {
      load_f32_row<VEC, NP>(w_row, lane, pieces, w);
      m_old = momentum1[id];
    }
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
      for (int s = 0; s < kCombineWaves - 1; ++s) {
        float v[NP][VEC];
        load_f32_row<VEC, NP>(shares + (int64_t)s * dim, lane, pieces, v);
        add_row<VEC, NP>(acc, v, lane, pieces);
      }
      apply_update<VEC, NP>(acc, w, m_old, lane, pieces, dim, w_row, momentum1 + id, lr, eps);
    }
    __syncthreads();                                         // the shares are read before the next segment's are written
  }
}

struct OptLayout {
  size_t part, partials_off, temp_off, temp_bytes, total;
};

// Small chunks for small batches, where the partial sums (packed at the row's own width) still fit the room laid out below:
// 2 * ceil(n / 32) * dim <= 2 * 4 * ceil(n / 128) * (kOptMaxDim / 4) for dim <= kSmallChunkMaxDim.
static int opt_chunk(int64_t n, int dim) { return n < kSmallBatch && dim <= kSmallChunkMaxDim ? kChunkSmall : kChunkLarge; }
static_assert(kChunkLarge / kChunkSmall * kSmallChunkMaxDim <= kOptMaxDim, "the small chunks' partial sums must fit the workspace");

// sorted_idx | perm (n each) | partial sums (two per 128 positions, sized for the widest row: dim is not known here, and the
// size must not depend on it) | sort temporary
static OptLayout opt_layout(int64_t n, int table_rows) {
  OptLayout l;
  l.part = align256((size_t)n * sizeof(int32_t));
  l.partials_off = 2 * l.part;
  l.temp_off = l.partials_off + align256(2 * (size_t)((n + kChunkLarge - 1) / kChunkLarge) * kOptMaxDim * sizeof(float));
  l.temp_bytes = n ? sort_temp_bytes(n, table_rows) : 0;
  l.total = l.temp_off + align256(l.temp_bytes);
  return l;
}

struct OptArgs {
  const void* g;
  const int32_t *perm, *sorted_idx;
  int64_t n;
  int dim;
  float *weight, *momentum1, *partials;
  float lr, eps;
  hipStream_t st;
};

template <typename T, int NP, int U, int kChunk>
static int opt_launch_chunk(const OptArgs& a, const char* what) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int64_t chunks = (a.n + kChunk - 1) / kChunk;
  const int64_t blocks = (chunks + kOptWaves - 1) / kOptWaves;
  hipLaunchKernelGGL((adagrad_chunk_kernel<T, NP, U, kChunk>), dim3((unsigned)(blocks < kOptMaxBlocks ? blocks : kOptMaxBlocks)),
                     dim3(kOptWaves * 64), 0, a.st, (const T*)a.g, a.perm, a.sorted_idx, a.n, a.dim, a.weight, a.momentum1, a.partials,
                     a.lr, a.eps);
  if (int rc = check_launch(what)) return rc;
  if (chunks < 2) return HSTU_OK;                                          // one chunk: nothing can leave it
  const size_t lds = (size_t)(kCombineWaves - 1) * a.dim * sizeof(float);  // at most 56 KiB
  hipLaunchKernelGGL((adagrad_combine_kernel<VEC, NP, kChunk>), dim3((unsigned)(chunks - 1 < kOptMaxBlocks ? chunks - 1 : kOptMaxBlocks)),
                     dim3(kCombineWaves * 64), lds, a.st, a.sorted_idx, a.n, a.dim, a.weight, a.momentum1, a.partials, a.lr, a.eps);
  return check_launch(what);
}

template <typename T, int NP, int U>
static int opt_launch(const OptArgs& a, const char* what) {
  return opt_chunk(a.n, a.dim) == kChunkSmall ? opt_launch_chunk<T, NP, U, kChunkSmall>(a, what) : opt_launch_chunk<T, NP, U, kChunkLarge>(a, what);
}

// gradient rows in flight per wave: eight for rows of up to 1 KiB (the reference's dim 256 in any dtype), fewer for wider
// rows -- each comes with a table row of twice (16-bit dout) or once its size in registers
template <typename T>
static int opt_dispatch(const OptArgs& a, const char* what) {
  const int row_bytes = a.dim * (int)sizeof(T);
  if (row_bytes <= 1024) return opt_launch<T, 1, 8>(a, what);
  if (row_bytes <= 2048) return opt_launch<T, 2, 4>(a, what);
  return opt_launch<T, 4, (sizeof(T) == 2 ? 2 : 4)>(a, what);
}

}  // namespace hstu

using namespace hstu;

extern "C" {

int hstu_embedding_rowwise_adagrad_workspace_bytes(int64_t n, int32_t table_rows, int64_t* bytes) {
  if (!bytes || n < 0 || n > 0x7fffffffLL || table_rows <= 0)
    return set_error(HSTU_EINVAL, "hstu_embedding_rowwise_adagrad_workspace_bytes: bad arguments");
  *bytes = (int64_t)opt_layout(n, table_rows).total;
  return HSTU_OK;
}

int hstu_embedding_rowwise_adagrad(const void* dout, const int32_t* idx, int64_t n, int32_t dim, int32_t table_rows, float* weight,
                                   float* momentum1, float lr, float eps, void* workspace, int64_t workspace_bytes, int dtype,
                                   void* stream) {
  const char* what = "hstu_embedding_rowwise_adagrad";
  if (!weight || !momentum1 || table_rows <= 0 || dim <= 0)
    return set_error(HSTU_EINVAL, "%s: weight and momentum1 must be non-NULL, sizes positive", what);
  if (!is_float_dtype(dtype)) return set_error(HSTU_EINVAL, "%s: dtype must be bf16, fp16 or fp32", what);
  const int es = dtype_bytes(dtype);
  if (dim > kOptMaxDim)                             // before any product with dim: dim * es must not wrap
    return set_error(HSTU_EUNSUPPORTED, "%s: rows of %d columns > %d", what, dim, kOptMaxDim);
  if ((dim * es) % 16 || ((uintptr_t)dout & 15) || ((uintptr_t)weight & 15))
    return set_error(HSTU_EINVAL, "%s: rows must be 16-byte multiples and 16-byte aligned", what);
  if (dim * es > kOptMaxPieces * 64 * 16)
    return set_error(HSTU_EUNSUPPORTED, "%s: rows of %d bytes > %d", what, dim * es, kOptMaxPieces * 64 * 16);
  if (n < 0 || n > 0x7fffffffLL) return set_error(HSTU_EINVAL, "%s: n out of range", what);
  if (n == 0) return HSTU_OK;
  if (!dout || !idx || !workspace) return set_error(HSTU_EINVAL, "%s: NULL input", what);
  const OptLayout l = opt_layout(n, table_rows);
  if (workspace_bytes < (int64_t)l.total || ((uintptr_t)workspace & 255))
    return set_error(HSTU_EINVAL, "%s: workspace too small or not 256-byte aligned (hstu_embedding_rowwise_adagrad_workspace_bytes)",
                     what);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* sorted_idx = (int32_t*)ws;
  int32_t* perm = (int32_t*)(ws + l.part);
  float* partials = (float*)(ws + l.partials_off);
  size_t temp = l.temp_bytes;
  hipError_t e = sort_indices(ws + l.temp_off, temp, idx, sorted_idx, perm, n, table_rows, st);
  if (e != hipSuccess) return set_error(HSTU_ELAUNCH, "%s: sort failed: %s", what, hipGetErrorString(e));
  const OptArgs a{dout, perm, sorted_idx, n, dim, weight, momentum1, partials, lr, eps, st};
  switch (dtype) {
    case HSTU_DTYPE_BF16: return opt_dispatch<bf16_t>(a, what);
    case HSTU_DTYPE_F16: return opt_dispatch<f16_t>(a, what);
    default: return opt_dispatch<float>(a, what);
  }
}

}  // extern "C"
