// jagged_dense_bmm_broadcast_add for gfx950: a per-user GEMM along the jagged offset vector, no padding.
//
//   out[s:e]      = jagged[s:e] @ dense[b] + bias[b]          [s, e) = [off[b], off[b+1])
//   d_jagged[s:e] = d_out[s:e] @ dense[b]^T                   (the same kernel: dense's strides swapped, no bias)
//   d_dense[b]    = jagged[s:e]^T @ d_out[s:e],  d_bias[b] = column sums of d_out[s:e]
//
// Reference semantics: ops/pytorch/pt_jagged.py:77-98 (padded torch.bmm in fp32, one rounding); the kernels replaced are
// ops/triton/triton_jagged.py:61-142 (forward / data gradient) and :145-240 (weight + bias gradient).
//
// Forward / data gradient (jagged_bmm_fwd_kernel).  A work item is (user, 64-row tile of that user, 128-column tile).  A
// one-workgroup scan (jagged_bmm_tiles_kernel) turns the offsets into tile_off[b] = number of row tiles in front of user
// b; the grid is the host-side bound ceil(rows / 64) + B on that count and every workgroup finds its user by bisection,
// so empty and short users cost nothing and max_seq_len never sizes anything.  K is walked in chunks of 128 bytes per
// row: the jagged rows (16-byte coalesced reads) and the dense chunk go through LDS once per work item, the next chunk's
// global loads are in flight while the MFMAs of the current one run.  dense is read either as [k][n] with n contiguous
// (B operand through the transposing LDS read) or as [n][k] with k contiguous (plain row reads); both feed the SAME
// values into the SAME MFMA slots in the same order, so the two layouts agree bit for bit.  The epilogue adds the fp32
// bias, rounds once and writes 16-byte rows through LDS.
//
// Weight + bias gradient (jagged_bmm_wgrad_kernel).  One workgroup per (user, 64 x 64 tile of dense[b]) walks the user's
// rows front to back in chunks of 32, accumulating in fp32 registers: a fixed order, no atomics, no float workspace, one
// store -- bit-identical run to run.  The tiles of K tile 0 also sum the columns of d_out they have staged anyway (fixed
// order: 8 rows per thread, chunks in sequence, four partial sums combined 0..3).  An empty user's loop runs zero times
// and its slab / row is written as zeros.
//
// LDS: forward 24 KiB (16-bit) / 33.5 KiB (fp32: the epilogue tile), weight gradient 10.2 / 18.4 KiB.  Shapes: K and N
// multiples of 16 bytes and 16-byte aligned rows (the Python layer zero-pads what is not); partial tiles are guarded per
// 16-byte unit and per row, nothing is read or written outside [s, e) x K / N.
#include "capi_internal.h"
#include "hstu_common.cuh"

namespace hstu {

constexpr int kBmmThreads = 256;
constexpr int kBmmTM = 64;      // rows of a forward work item
constexpr int kBmmTN = 128;     // columns of a forward work item
constexpr int kBmmWT = 64;      // the weight gradient's tile of dense[b] is kBmmWT x kBmmWT
constexpr int kBmmRC = 32;      // rows per step of the weight gradient

struct BmmFwdArgs {
  const char* a;          // (rows, K) jagged | d_out
  const char* dense;      // (B, K, N) through strides
  const float* bias;      // (B, N) fp32 or nullptr
  char* out;              // (rows, N)
  const void* offsets;
  const int32_t* tile_off;   // (B + 1), written by jagged_bmm_tiles_kernel
  int64_t a_rs, d_bs, d_ks, d_ns, bias_bs, o_rs, total_rows;
  int32_t batch, k, n, n_tiles, is64;
};

struct BmmWgradArgs {
  const char* a;          // (rows, K) jagged
  const char* g;          // (rows, N) d_out
  char* dd;               // (B, K, N): batch / k strides, n contiguous
  float* db;              // (B, N) fp32 or nullptr
  const void* offsets;
  int64_t a_rs, g_rs, dd_bs, dd_ks, db_bs, total_rows;
  int32_t batch, k, n, k_tiles, n_tiles, is64;
};

// rows [s, e) of user b, clamped to the rows the caller says exist (a bad offset vector must not become a wild read)
HSTU_DEV void bmm_user_rows(const void* offsets, int b, int is64, int64_t total, int64_t* s, int64_t* e) {
  int64_t s_ = load_index(offsets, b, is64), e_ = load_index(offsets, b + 1, is64);
  s_ = min(max(s_, (int64_t)0), total);
  e_ = max(min(e_, total), s_);
  *s = s_;
  *e = e_;
}

template <typename T> HSTU_DEV T bmm_round(float x);
template <> HSTU_DEV float bmm_round<float>(float x) { return x; }
template <> HSTU_DEV bf16_t bmm_round<bf16_t>(float x) {
  return __builtin_bit_cast(bf16_t, (uint16_t)(Elem<bf16_t>::pk2(x, 0.f) & 0xffffu));
}
template <> HSTU_DEV f16_t bmm_round<f16_t>(float x) {
  return __builtin_bit_cast(f16_t, (uint16_t)(Elem<f16_t>::pk2(x, 0.f) & 0xffffu));
}

// tile_off[0] = 0, tile_off[b + 1] = tile_off[b] + ceil(len_b / kBmmTM).  One workgroup, chunked wave scan with carry.
__global__ __launch_bounds__(1024) void jagged_bmm_tiles_kernel(const void* offsets, int32_t* tile_off, int batch, int is64,
                                                                int64_t total) {
  __shared__ int wave_tot[16];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { tile_off[0] = 0; carry_s = 0; }
  __syncthreads();
  for (int base = 0; base < batch; base += 1024) {
    const int i = base + tid;
    int x = 0;
    if (i < batch) {
      int64_t s, e;
      bmm_user_rows(offsets, i, is64, total, &s, &e);
      x = (int)((e - s + kBmmTM - 1) / kBmmTM);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      int y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    int pre = carry_s;
    for (int w = 0; w < wave; ++w) pre += wave_tot[w];
    if (i < batch) tile_off[i + 1] = x + pre;
    __syncthreads();
    if (tid == 1023) carry_s = x + pre;
    __syncthreads();
  }
}

// BT == false: dense[b] is [k][n] with n contiguous;  BT == true: [n][k] with k contiguous
template <typename T, bool BT>
__global__ __launch_bounds__(kBmmThreads) void jagged_bmm_fwd_kernel(const BmmFwdArgs p) {
  typedef typename Elem<T>::Frag Frag;
  constexpr int ES = Elem<T>::kBytes, EPU = 16 / ES;
  constexpr int KC = 128 / ES;                          // k per chunk: 128-byte rows of the jagged tile
  constexpr int UPR_A = 8;
  constexpr int UPR_B = BT ? 8 : kBmmTN / EPU;
  constexpr int A_BYTES = kBmmTM * 128, B_BYTES = kBmmTN * 128;
  constexpr int A_UNITS = A_BYTES / 16 / kBmmThreads, B_UNITS = B_BYTES / 16 / kBmmThreads;   // per thread: 2, 4
  constexpr int O_STRIDE = kBmmTN * ES + 16, O_BYTES = kBmmTM * O_STRIDE;
  constexpr int SMEM = (A_BYTES + B_BYTES) > O_BYTES ? (A_BYTES + B_BYTES) : O_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  char* As = smem;
  char* Bs = smem + A_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n32 = lane & 31, hf = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int t = blockIdx.x / p.n_tiles, n0 = (blockIdx.x % p.n_tiles) * kBmmTN;
  if (t >= p.tile_off[p.batch]) return;
  int lo = 0, hi = p.batch;                              // tile_off[lo] <= t < tile_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.tile_off[mid] <= t) lo = mid; else hi = mid;
  }
  const int b = lo;
  int64_t s, e;
  bmm_user_rows(p.offsets, b, p.is64, p.total_rows, &s, &e);
  const int64_t row0 = s + (int64_t)(t - p.tile_off[b]) * kBmmTM;
  const int rows = (int)min((int64_t)kBmmTM, e - row0);
  if (rows <= 0) return;
  const char* a_base = p.a + row0 * p.a_rs * ES;
  const char* d_base = p.dense + (int64_t)b * p.d_bs * ES;

  u32x4 ra[A_UNITS], rb[B_UNITS];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int q = 0; q < A_UNITS; ++q) {
      const int i = tid + q * kBmmThreads, r = i >> 3, kk = k0 + (i & 7) * EPU;
      ra[q] = u32x4{0, 0, 0, 0};
      if (r < rows && kk < p.k) ra[q] = gload16(a_base + ((int64_t)r * p.a_rs + kk) * ES);
    }
#pragma unroll
    for (int q = 0; q < B_UNITS; ++q) {
      const int i = tid + q * kBmmThreads;
      rb[q] = u32x4{0, 0, 0, 0};
      if constexpr (BT) {
        const int nn = n0 + (i >> 3), kk = k0 + (i & 7) * EPU;
        if (nn < p.n && kk < p.k) rb[q] = gload16(d_base + ((int64_t)nn * p.d_ns + kk) * ES);
      } else {
        const int kk = k0 + i / UPR_B, nn = n0 + (i % UPR_B) * EPU;
        if (kk < p.k && nn < p.n) rb[q] = gload16(d_base + ((int64_t)kk * p.d_ks + nn) * ES);
      }
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int q = 0; q < A_UNITS; ++q) {
      const int i = tid + q * kBmmThreads;
      *LDS_PTR(u32x4, As + tile_off<UPR_A>(i >> 3, i & 7)) = ra[q];
    }
#pragma unroll
    for (int q = 0; q < B_UNITS; ++q) {
      const int i = tid + q * kBmmThreads;
      *LDS_PTR(u32x4, Bs + tile_off<UPR_B>(i / UPR_B, i % UPR_B)) = rb[q];
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  load_chunk(0);
  for (int k0 = 0; k0 < p.k; k0 += KC) {
    store_chunk();
    __syncthreads();
    if (k0 + KC < p.k) load_chunk(k0 + KC);              // in flight while this chunk's MFMAs run
#pragma unroll
    for (int ks = 0; ks < KC / 16; ++ks) {
      const int e0 = ks * 16 + 8 * hf;                   // slot (hf, j) of both operands carries k = e0 + j
      const Frag af = lds_row_frag<T, UPR_A>(As, wm * 32 + n32, e0);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        Frag bf;
        if constexpr (BT) bf = lds_row_frag<T, UPR_B>(Bs, wn * 64 + c * 32 + n32, e0);
        else bf = lds_col_frag<T, UPR_B>(Bs, e0, e0 + 4, wn * 64 + c * 32, lane);
        acc[c] = Elem<T>::mma(af, bf, acc[c]);
      }
    }
    __syncthreads();
  }

  // epilogue: + bias (fp32), one rounding, 16-byte rows through LDS
  const float* bias = p.bias ? p.bias + (int64_t)b * p.bias_bs : nullptr;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = wn * 64 + c * 32 + n32;
    const float bv = (bias && n0 + col < p.n) ? bias[n0 + col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf;
      *LDS_PTR(T, smem + row * O_STRIDE + col * ES) = bmm_round<T>(acc[c][r] + bv);
    }
  }
  __syncthreads();
  constexpr int UPO = kBmmTN / EPU;
  char* o_base = p.out + row0 * p.o_rs * ES;
  for (int i = tid; i < kBmmTM * UPO; i += kBmmThreads) {
    const int r = i / UPO, nn = n0 + (i % UPO) * EPU;
    if (r < rows && nn < p.n)
      gstore16(o_base + ((int64_t)r * p.o_rs + nn) * ES, *LDS_PTR(const u32x4, smem + r * O_STRIDE + (i % UPO) * 16));
  }
}

template <typename T>
__global__ __launch_bounds__(kBmmThreads) void jagged_bmm_wgrad_kernel(const BmmWgradArgs p) {
  typedef typename Elem<T>::Frag Frag;
  constexpr int ES = Elem<T>::kBytes, EPU = 16 / ES;
  constexpr int UPR = kBmmWT / EPU;                      // 8 | 16
  constexpr int T_BYTES = kBmmRC * kBmmWT * ES;
  constexpr int UNITS = T_BYTES / 16 / kBmmThreads;      // per thread and tile: 1 | 2
  constexpr int O_STRIDE = kBmmWT * ES + 16, O_BYTES = kBmmWT * O_STRIDE;
  constexpr int SMEM = 2 * T_BYTES > O_BYTES ? 2 * T_BYTES : O_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  __shared__ float colsum[4][kBmmWT];
  char* Js = smem;
  char* Gs = smem + T_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n32 = lane & 31, hf = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int n0 = (blockIdx.x % p.n_tiles) * kBmmWT;
  const int kt = (blockIdx.x / p.n_tiles) % p.k_tiles, k0 = kt * kBmmWT;
  const int b = blockIdx.x / (p.n_tiles * p.k_tiles);
  int64_t s, e;
  bmm_user_rows(p.offsets, b, p.is64, p.total_rows, &s, &e);
  const bool sum_cols = kt == 0 && p.db != nullptr;     // uniform over the workgroup

  u32x4 rj[UNITS], rg[UNITS];
  auto load_chunk = [&](int64_t r0) {
#pragma unroll
    for (int q = 0; q < UNITS; ++q) {
      const int i = tid + q * kBmmThreads, u = i % UPR;
      const int64_t r = r0 + i / UPR;
      rj[q] = u32x4{0, 0, 0, 0};
      rg[q] = u32x4{0, 0, 0, 0};
      if (r < e && k0 + u * EPU < p.k) rj[q] = gload16(p.a + (r * p.a_rs + k0 + u * EPU) * ES);
      if (r < e && n0 + u * EPU < p.n) rg[q] = gload16(p.g + (r * p.g_rs + n0 + u * EPU) * ES);
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float bsum = 0.f;
  const int sc = tid & 63, sq = tid >> 6;               // column sums: column sc, rows 8 sq .. 8 sq + 7 of every chunk

  if (s < e) load_chunk(s);
  for (int64_t r0 = s; r0 < e; r0 += kBmmRC) {
#pragma unroll
    for (int q = 0; q < UNITS; ++q) {
      const int i = tid + q * kBmmThreads;
      *LDS_PTR(u32x4, Js + tile_off<UPR>(i / UPR, i % UPR)) = rj[q];
      *LDS_PTR(u32x4, Gs + tile_off<UPR>(i / UPR, i % UPR)) = rg[q];
    }
    __syncthreads();
    if (r0 + kBmmRC < e) load_chunk(r0 + kBmmRC);
#pragma unroll
    for (int ks = 0; ks < kBmmRC / 16; ++ks) {
      const int ra = ks * 16 + 8 * hf;                   // slot (hf, j) of both operands carries row ra + j
      const Frag af = lds_col_frag<T, UPR>(Js, ra, ra + 4, wm * 32, lane);    // jagged^T[k][row]
      const Frag bf = lds_col_frag<T, UPR>(Gs, ra, ra + 4, wn * 32, lane);    // d_out[row][n]
      acc = Elem<T>::mma(af, bf, acc);
    }
    if (sum_cols) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        bsum += to_f32(*LDS_PTR(const T, Gs + tile_off<UPR>(sq * 8 + j, sc / EPU) + (sc % EPU) * ES));
    }
    __syncthreads();
  }

  if (sum_cols) {
    colsum[sq][sc] = bsum;
    __syncthreads();
    if (tid < kBmmWT && n0 + tid < p.n)
      p.db[(int64_t)b * p.db_bs + n0 + tid] = ((colsum[0][tid] + colsum[1][tid]) + colsum[2][tid]) + colsum[3][tid];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf;
    *LDS_PTR(T, smem + row * O_STRIDE + (wn * 32 + n32) * ES) = bmm_round<T>(acc[r]);
  }
  __syncthreads();
  constexpr int UPO = kBmmWT / EPU;
  char* o_base = p.dd + (int64_t)b * p.dd_bs * ES;
  for (int i = tid; i < kBmmWT * UPO; i += kBmmThreads) {
    const int r = i / UPO, nn = n0 + (i % UPO) * EPU;
    if (k0 + r < p.k && nn < p.n)
      gstore16(o_base + ((int64_t)(k0 + r) * p.dd_ks + nn) * ES, *LDS_PTR(const u32x4, smem + r * O_STRIDE + (i % UPO) * 16));
  }
}

template <typename T>
static int launch_fwd_t(const BmmFwdArgs& a, bool bt, int64_t blocks, hipStream_t st) {
  if (bt) hipLaunchKernelGGL((jagged_bmm_fwd_kernel<T, true>), dim3((unsigned)blocks), dim3(kBmmThreads), 0, st, a);
  else hipLaunchKernelGGL((jagged_bmm_fwd_kernel<T, false>), dim3((unsigned)blocks), dim3(kBmmThreads), 0, st, a);
  return check_launch("jagged_dense_bmm_fwd");
}

size_t jagged_bmm_workspace_bytes(int batch) { return ((size_t)(batch > 0 ? batch : 0) + 1) * sizeof(int32_t); }

int launch_jagged_bmm_fwd(const void* jagged, int64_t a_rs, const void* dense, int64_t d_bs, int64_t d_ks, int64_t d_ns,
                          const float* bias, int64_t bias_bs, void* out, int64_t o_rs, const void* offsets,
                          int64_t total_rows, int batch, int k, int n, void* workspace, int dtype, int index_dtype,
                          hipStream_t st) {
  BmmFwdArgs a;
  a.a = (const char*)jagged; a.dense = (const char*)dense; a.bias = bias; a.out = (char*)out; a.offsets = offsets;
  a.tile_off = (const int32_t*)workspace;
  a.a_rs = a_rs; a.d_bs = d_bs; a.d_ks = d_ks; a.d_ns = d_ns; a.bias_bs = bias_bs; a.o_rs = o_rs; a.total_rows = total_rows;
  a.batch = batch; a.k = k; a.n = n; a.n_tiles = (n + kBmmTN - 1) / kBmmTN; a.is64 = index_dtype == HSTU_INDEX_I64;
  const int64_t row_tiles = (total_rows + kBmmTM - 1) / kBmmTM + batch;   // >= sum over users of ceil(len / 64)
  const int64_t blocks = row_tiles * a.n_tiles;
  if (blocks > 0x7fffffffLL) return set_error(HSTU_EUNSUPPORTED, "jagged_dense_bmm_fwd: %lld work items exceed the grid limit", (long long)blocks);
  hipLaunchKernelGGL(jagged_bmm_tiles_kernel, dim3(1), dim3(1024), 0, st, offsets, (int32_t*)workspace, batch, a.is64, total_rows);
  if (int err = check_launch("jagged_dense_bmm_fwd(tiles)")) return err;
  const bool bt = d_ns != 1;
  switch (dtype) {
    case HSTU_DTYPE_BF16: return launch_fwd_t<bf16_t>(a, bt, blocks, st);
    case HSTU_DTYPE_F16: return launch_fwd_t<f16_t>(a, bt, blocks, st);
    default: return launch_fwd_t<float>(a, bt, blocks, st);
  }
}

int launch_jagged_bmm_wgrad(const void* jagged, int64_t a_rs, const void* d_out, int64_t g_rs, void* d_dense, int64_t dd_bs,
                            int64_t dd_ks, float* d_bias, int64_t db_bs, const void* offsets, int64_t total_rows, int batch,
                            int k, int n, int dtype, int index_dtype, hipStream_t st) {
  BmmWgradArgs a;
  a.a = (const char*)jagged; a.g = (const char*)d_out; a.dd = (char*)d_dense; a.db = d_bias; a.offsets = offsets;
  a.a_rs = a_rs; a.g_rs = g_rs; a.dd_bs = dd_bs; a.dd_ks = dd_ks; a.db_bs = db_bs; a.total_rows = total_rows;
  a.batch = batch; a.k = k; a.n = n; a.k_tiles = (k + kBmmWT - 1) / kBmmWT; a.n_tiles = (n + kBmmWT - 1) / kBmmWT;
  a.is64 = index_dtype == HSTU_INDEX_I64;
  const int64_t blocks = (int64_t)batch * a.k_tiles * a.n_tiles;
  if (blocks > 0x7fffffffLL) return set_error(HSTU_EUNSUPPORTED, "jagged_dense_bmm_wgrad: %lld work items exceed the grid limit", (long long)blocks);
  const dim3 grid((unsigned)blocks), block(kBmmThreads);
  switch (dtype) {
    case HSTU_DTYPE_BF16: hipLaunchKernelGGL(jagged_bmm_wgrad_kernel<bf16_t>, grid, block, 0, st, a); break;
    case HSTU_DTYPE_F16: hipLaunchKernelGGL(jagged_bmm_wgrad_kernel<f16_t>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(jagged_bmm_wgrad_kernel<float>, grid, block, 0, st, a); break;
  }
  return check_launch("jagged_dense_bmm_wgrad");
}

}  // namespace hstu
