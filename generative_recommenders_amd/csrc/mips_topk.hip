// Fused maximum-inner-product top-k for gfx950: the k best items of a table for every query row, without the (B, X)
// score matrix.
//
//   scores[b, x] = <queries[b], items[x]>   (fp32 accumulation)        out = the k largest per row, sorted
//
// Reference semantics: research/rails/indexing/mips_top_k.py:68-81 (torch.mm + torch.topk), with a FIXED order on top:
// score descending, then item index ascending; -0.0 and +0.0 are one score.  torch.topk leaves ties unspecified.
//
// One order, one key.  Every (score, index) pair becomes the 64-bit word
//     C = order_key(score) << 32 | ~index            order_key: the usual monotone map of fp32 bits to uint32
// so "score descending, index ascending" is "C descending", and all C of a row are distinct.  The k best items of a row
// are exactly the items with C >= T, T the k-th largest C.  T is found by a radix select, most significant byte first:
// eight passes (four over the score key, four over the index), each of which RECOMPUTES the score tiles with MFMA and
// counts, per row, the byte under inspection of the items that still match the digits fixed so far.  A ninth pass emits
// the items with C >= T -- exactly k per row -- and one workgroup per row sorts them.  The launch sequence is fixed (no
// host sync, nothing depends on device data) and every count is an integer, so the result is bit-identical run to run.
//
// Score tiles (mips_topk_score_kernel).  A workgroup owns 64 query rows and a contiguous range of 128-item tiles.  Both
// operands go through LDS in chunks of 128 bytes per row (16-byte coalesced reads, the next chunk's loads in flight while
// the MFMAs of the current one run), the layout and MFMA slots of jagged_bmm.hip.  The select passes keep a [64][256]
// uint32 histogram in LDS (64 KiB) and flush its non-zero bins with integer global atomics; lanes of a half wave share a
// query row, and the ones that agree with the half's first lane on the bin are counted by one LDS atomic (the first pass
// looks at sign and exponent: nearly every score of a row is in the same bin).
//
// Workspace: per row 256 bins, the digits fixed so far, the count still wanted, the emit cursor and k candidates --
// O(B (bins + k)), independent of the table size.  Nothing of size B x X exists anywhere.
//
// LDS: select 88.5 KiB, emit 24.5 KiB, sort 32 KiB; every word that is read has been written (rows and items outside
// the problem are zero-filled, the histogram is cleared, the sort pads with 0).  Nothing is read outside
// [0, B) x dim / [0, X) x dim or written outside the outputs and the workspace.
#include "capi_internal.h"
#include "hstu_common.cuh"

namespace hstu {

constexpr int kTkThreads = 256;
constexpr int kTkTM = 64;        // query rows of a workgroup
constexpr int kTkTN = 128;       // items of a score tile
constexpr int kTkBins = 256;     // one byte of the key per pass
constexpr int kTkPasses = 8;
constexpr int kTkMaxK = 4096;    // the sort's LDS: 4096 x 8 bytes
constexpr int kTkTileBytes = (kTkTM + kTkTN) * 128;
constexpr int kTkStateOff = kTkTileBytes;                         // 64 x uint64: the rows' digits / threshold
constexpr int kTkHistOff = kTkStateOff + kTkTM * 8;
constexpr int kTkSmemEmit = kTkHistOff;
constexpr int kTkSmemSelect = kTkHistOff + kTkTM * kTkBins * 4;

struct TopkArgs {
  const char* q;          // (B, dim), row stride q_rs elements
  const char* items;      // (X, dim), row stride i_rs elements
  uint32_t* hist;         // (B, 256): the current pass; cleared by the scan that reads it
  uint64_t* prefix;       // (B): digits fixed so far, after the last pass the threshold T
  uint32_t* remain;       // (B): how many items with the digits fixed so far are still wanted
  uint32_t* cursor;       // (B): candidates emitted
  uint64_t* cand;         // (B, k)
  int64_t q_rs, i_rs;
  int32_t batch, num_items, dim, k, pass, tiles_per_wg;
};

// monotone fp32 -> uint32 (larger score, larger key); both zeros map to the key of +0.0
HSTU_DEV uint32_t topk_key(float s) {
  uint32_t b = __builtin_bit_cast(uint32_t, s);
  if ((b << 1) == 0) b = 0;
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
HSTU_DEV float topk_score(uint32_t key) {
  return __builtin_bit_cast(float, (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

template <typename T> HSTU_DEV T topk_round(float x);
template <> HSTU_DEV float topk_round<float>(float x) { return x; }
template <> HSTU_DEV bf16_t topk_round<bf16_t>(float x) {
  return __builtin_bit_cast(bf16_t, (uint16_t)(Elem<bf16_t>::pk2(x, 0.f) & 0xffffu));
}
template <> HSTU_DEV f16_t topk_round<f16_t>(float x) {
  return __builtin_bit_cast(f16_t, (uint16_t)(Elem<f16_t>::pk2(x, 0.f) & 0xffffu));
}

__global__ __launch_bounds__(kTkThreads) void mips_topk_init_kernel(const TopkArgs p) {
  const int64_t i = (int64_t)blockIdx.x * kTkThreads + threadIdx.x;
  if (i < (int64_t)p.batch * kTkBins) p.hist[i] = 0;
  if (i < p.batch) {
    p.prefix[i] = 0;
    p.remain[i] = (uint32_t)p.k;
    p.cursor[i] = 0;
  }
}

// EMIT == false: pass p.pass of the radix select;  EMIT == true: append the items with C >= T to the candidates
template <typename T, bool EMIT>
__global__ __launch_bounds__(kTkThreads) void mips_topk_score_kernel(const TopkArgs p) {
  typedef typename Elem<T>::Frag Frag;
  constexpr int ES = Elem<T>::kBytes, EPU = 16 / ES;
  constexpr int KC = 128 / ES;                          // k per chunk
  constexpr int A_BYTES = kTkTM * 128;
  constexpr int A_UNITS = kTkTM * 8 / kTkThreads, B_UNITS = kTkTN * 8 / kTkThreads;   // per thread: 2, 4
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* As = smem;
  char* Bs = smem + A_BYTES;
  char* state = smem + kTkStateOff;
  char* hist = smem + kTkHistOff;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n32 = lane & 31, hf = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int row0 = blockIdx.x * kTkTM;
  const int rows = min(kTkTM, p.batch - row0);
  const int n_tiles = (p.num_items + kTkTN - 1) / kTkTN;
  const int t_begin = blockIdx.y * p.tiles_per_wg, t_end = min(t_begin + p.tiles_per_wg, n_tiles);

  if (tid < kTkTM) *LDS_PTR(uint64_t, state + 8 * tid) = tid < rows ? p.prefix[row0 + tid] : 0;
  if constexpr (!EMIT) {
    for (int i = tid; i < kTkTM * kTkBins / 4; i += kTkThreads) *LDS_PTR(u32x4, hist + 16 * i) = u32x4{0, 0, 0, 0};
  }
  const int shift = 8 * (kTkPasses - 1 - p.pass);       // select: the byte of C this pass counts
  const char* a_base = p.q + (int64_t)row0 * p.q_rs * ES;

  for (int t = t_begin; t < t_end; ++t) {
    const int n0 = t * kTkTN;
    u32x4 ra[A_UNITS], rb[B_UNITS];
    auto load_chunk = [&](int k0) {
#pragma unroll
      for (int q = 0; q < A_UNITS; ++q) {
        const int i = tid + q * kTkThreads, r = i >> 3, kk = k0 + (i & 7) * EPU;
        ra[q] = u32x4{0, 0, 0, 0};
        if (r < rows && kk < p.dim) ra[q] = gload16(a_base + ((int64_t)r * p.q_rs + kk) * ES);
      }
#pragma unroll
      for (int q = 0; q < B_UNITS; ++q) {
        const int i = tid + q * kTkThreads, nn = n0 + (i >> 3), kk = k0 + (i & 7) * EPU;
        rb[q] = u32x4{0, 0, 0, 0};
        if (nn < p.num_items && kk < p.dim) rb[q] = gload16(p.items + ((int64_t)nn * p.i_rs + kk) * ES);
      }
    };

    f32x16 acc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    load_chunk(0);
    for (int k0 = 0; k0 < p.dim; k0 += KC) {
#pragma unroll
      for (int q = 0; q < A_UNITS; ++q) {
        const int i = tid + q * kTkThreads;
        *LDS_PTR(u32x4, As + tile_off<8>(i >> 3, i & 7)) = ra[q];
      }
#pragma unroll
      for (int q = 0; q < B_UNITS; ++q) {
        const int i = tid + q * kTkThreads;
        *LDS_PTR(u32x4, Bs + tile_off<8>(i >> 3, i & 7)) = rb[q];
      }
      __syncthreads();                                   // (the first one also covers the state / histogram setup)
      if (k0 + KC < p.dim) load_chunk(k0 + KC);
#pragma unroll
      for (int ks = 0; ks < KC / 16; ++ks) {
        const int e0 = ks * 16 + 8 * hf;                 // slot (hf, j) of both operands carries k = e0 + j
        const Frag af = lds_row_frag<T, 8>(As, wm * 32 + n32, e0);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const Frag bf = lds_row_frag<T, 8>(Bs, wn * 64 + c * 32 + n32, e0);
          acc[c] = Elem<T>::mma(af, bf, acc[c]);
        }
      }
      __syncthreads();
    }

    // epilogue: acc[c][r] = score of query row wm * 32 + (r & 3) + 8 (r >> 2) + 4 hf and item n0 + wn * 64 + c * 32 + n32
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf;
      const uint64_t pre = *LDS_PTR(const uint64_t, state + 8 * row);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int item = n0 + wn * 64 + c * 32 + n32;
        const uint64_t cw = ((uint64_t)topk_key(acc[c][r]) << 32) | (uint32_t)~item;
        const bool in = row < rows && item < p.num_items;
        if constexpr (EMIT) {
          if (in && cw >= pre) {
            const uint32_t pos = atomicAdd(&p.cursor[row0 + row], 1u);
            if (pos < (uint32_t)p.k) p.cand[(int64_t)(row0 + row) * p.k + pos] = cw;
          }
        } else {
          // still a candidate: the digits above this pass's byte equal the ones fixed so far
          const bool live = in && (p.pass == 0 || (cw >> (shift + 8)) == (pre >> (shift + 8)));
          const int bin = live ? (int)((cw >> shift) & 255) : -1;
          const int lead = __shfl(bin, lane & 32, 64);   // the bin of this half wave's (= this row's) first lane
          const bool same = live && bin == lead;
          const uint64_t agree = __builtin_amdgcn_ballot_w64(same);
          const uint32_t cnt = __builtin_popcount((uint32_t)(agree >> (lane & 32)));
          // (n32 == 0: lead == bin, cnt counts this lane too)
          if (live && (n32 == 0 || !same))
            __hip_atomic_fetch_add(LDS_PTR(uint32_t, hist + 4 * (row * kTkBins + bin)), n32 == 0 ? cnt : 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
  }

  if constexpr (!EMIT) {
    __syncthreads();
    for (int i = tid; i < rows * kTkBins; i += kTkThreads) {
      const uint32_t v = *LDS_PTR(const uint32_t, hist + 4 * i);
      if (v) atomicAdd(&p.hist[(int64_t)row0 * kTkBins + i], v);
    }
  }
}

// one workgroup per row, one thread per bin: fix the next digit, clear the bins for the next pass
__global__ __launch_bounds__(kTkBins) void mips_topk_scan_kernel(const TopkArgs p) {
  __shared__ uint32_t h[kTkBins];
  const int row = blockIdx.x, tid = threadIdx.x;
  uint32_t* g = p.hist + (int64_t)row * kTkBins;
  h[tid] = g[tid];
  g[tid] = 0;
  __syncthreads();
  if (tid == 0) {
    const uint32_t want = p.remain[row];
    uint32_t above = 0;
    int bin = kTkBins - 1;
    for (; bin > 0; --bin) {                             // the largest bin with (items in bins >= bin) >= want
      if (above + h[bin] >= want) break;
      above += h[bin];
    }
    p.prefix[row] |= (uint64_t)bin << (8 * (kTkPasses - 1 - p.pass));
    p.remain[row] = want - above;
  }
}

// one workgroup per row: bitonic sort of the candidates (descending C), then scores and indices
template <typename T>
__global__ __launch_bounds__(kTkThreads) void mips_topk_sort_kernel(const TopkArgs p, T* out_scores, int32_t* out_indices) {
  __shared__ uint64_t s[kTkMaxK];
  const int row = blockIdx.x, tid = threadIdx.x;
  int n = 1;
  while (n < p.k) n <<= 1;
  const int have = (int)min(p.cursor[row], (uint32_t)p.k);
  for (int i = tid; i < n; i += kTkThreads) s[i] = i < have ? p.cand[(int64_t)row * p.k + i] : 0;   // 0 sorts behind every C
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (n >> 1); i += kTkThreads) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const uint64_t a = s[lo], b = s[hi];
        if ((a < b) == desc) { s[lo] = b; s[hi] = a; }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < p.k; i += kTkThreads) {
    const uint64_t c = s[i];
    out_scores[(int64_t)row * p.k + i] = topk_round<T>(topk_score((uint32_t)(c >> 32)));
    out_indices[(int64_t)row * p.k + i] = (int32_t)~(uint32_t)c;
  }
}

static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// deliberately a function of (batch, k) only: nothing in the workspace grows with the table
size_t mips_topk_workspace_bytes(int batch, int k) {
  const size_t b = batch > 0 ? (size_t)batch : 0, kk = k > 0 ? (size_t)k : 0;
  return align16(b * kTkBins * 4) + align16(b * 8) + 2 * align16(b * 4) + align16(b * kk * 8);
}

template <typename T>
static int launch_topk_t(TopkArgs a, void* out_scores, int32_t* out_indices, hipStream_t st) {
  auto select = mips_topk_score_kernel<T, false>;
  auto emit = mips_topk_score_kernel<T, true>;
  hipError_t e = hipFuncSetAttribute((const void*)select, hipFuncAttributeMaxDynamicSharedMemorySize, kTkSmemSelect);
  if (e != hipSuccess) return set_error(HSTU_ELAUNCH, "hstu_mips_topk: cannot reserve %d bytes of LDS: %s", kTkSmemSelect, hipGetErrorString(e));
  const int q_tiles = (a.batch + kTkTM - 1) / kTkTM, n_tiles = (a.num_items + kTkTN - 1) / kTkTN;
  // item ranges: about four workgroups per CU in all; the query tiles of one range are neighbours in launch order and
  // read the same items at about the same time
  int splits = 4 * cu_count() / q_tiles;
  splits = splits < 1 ? 1 : (splits > n_tiles ? n_tiles : splits);
  a.tiles_per_wg = (n_tiles + splits - 1) / splits;
  splits = (n_tiles + a.tiles_per_wg - 1) / a.tiles_per_wg;
  if (splits > 65535) return set_error(HSTU_EUNSUPPORTED, "hstu_mips_topk: %d item ranges exceed the grid limit", splits);
  const dim3 grid((unsigned)q_tiles, (unsigned)splits), block(kTkThreads);
  const unsigned init_blocks = (unsigned)(((int64_t)a.batch * kTkBins + kTkThreads - 1) / kTkThreads);
  hipLaunchKernelGGL(mips_topk_init_kernel, dim3(init_blocks), block, 0, st, a);
  if (int err = check_launch("hstu_mips_topk(init)")) return err;
  for (int pass = 0; pass < kTkPasses; ++pass) {
    a.pass = pass;
    hipLaunchKernelGGL(select, grid, block, kTkSmemSelect, st, a);
    if (int err = check_launch("hstu_mips_topk(select)")) return err;
    hipLaunchKernelGGL(mips_topk_scan_kernel, dim3((unsigned)a.batch), dim3(kTkBins), 0, st, a);
    if (int err = check_launch("hstu_mips_topk(scan)")) return err;
  }
  hipLaunchKernelGGL(emit, grid, block, kTkSmemEmit, st, a);
  if (int err = check_launch("hstu_mips_topk(emit)")) return err;
  hipLaunchKernelGGL(mips_topk_sort_kernel<T>, dim3((unsigned)a.batch), block, 0, st, a, (T*)out_scores, out_indices);
  return check_launch("hstu_mips_topk(sort)");
}

int launch_mips_topk(const void* queries, int64_t q_rs, const void* items, int64_t i_rs, void* out_scores, int32_t* out_indices,
                     void* workspace, int batch, int num_items, int dim, int k, int dtype, hipStream_t st) {
  TopkArgs a;
  char* ws = (char*)workspace;
  const size_t b = (size_t)batch;
  a.q = (const char*)queries; a.items = (const char*)items; a.q_rs = q_rs; a.i_rs = i_rs;
  a.hist = (uint32_t*)ws; ws += align16(b * kTkBins * 4);
  a.prefix = (uint64_t*)ws; ws += align16(b * 8);
  a.remain = (uint32_t*)ws; ws += align16(b * 4);
  a.cursor = (uint32_t*)ws; ws += align16(b * 4);
  a.cand = (uint64_t*)ws;
  a.batch = batch; a.num_items = num_items; a.dim = dim; a.k = k; a.pass = 0; a.tiles_per_wg = 1;
  switch (dtype) {
    case HSTU_DTYPE_BF16: return launch_topk_t<bf16_t>(a, out_scores, out_indices, st);
    case HSTU_DTYPE_F16: return launch_topk_t<f16_t>(a, out_scores, out_indices, st);
    default: return launch_topk_t<float>(a, out_scores, out_indices, st);
  }
}

}  // namespace hstu
