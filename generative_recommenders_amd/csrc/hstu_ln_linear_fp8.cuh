// y = (q(LayerNorm(x)) . q(W)^T) x_scale w_scale + b: the UVQK projection with row-wise e4m3 operands (gfx950).
//   The reference's switch fp8_in_addmm_fwd (ops/cpp/cuda_hstu_preprocess_and_attention.py:75-95,231-245): its LayerNorm
//   quantizes its output row by row and the GEMM is a row-wise-scaled fp8 GEMM; both kernels are outside the open tree.
//
// Arithmetic (the contract; tests/fp8_linear_ref.py restates it):
//   nx[r,:]    = LayerNorm(x[r,:]) ln_w + ln_b                   fp32, not rounded to the I/O type
//   x_scale[r] = max_k |nx[r,k]| / 448   (1 for a zero row)       fp32, IEEE division
//   xq[r,k]    = e4m3_rne(clamp(nx[r,k] / x_scale[r], +-448))     OCP e4m3fn, IEEE division
//   y[r,n]     = (sum_k xq[r,k] wq[n,k]) x_scale[r] w_scale[n] + bias[n]      fp32 accumulation, one rounding
// (wq, w_scale): the (n, k) weight quantized by the same rule (hstu_quantize_rows_fp8_kernel below).
//
// The arrangement is hstu_ln_linear.cuh's: a wave keeps 32 complete rows in registers -- as e4m3 they take 64 instead of
// 128 -- a workgroup of 8 waves walks the weight, 32 output columns (32 x 512 bytes = 16 KiB) at a time, through a ring of
// LDS tiles filled by LDS-DMA, and the product is formed transposed (W is the MFMA's A operand).  The MFMA is
// v_mfma_f32_32x32x64_f8f6f4: 8 per 32 x 32 tile.  Lane (m, h) supplies, for K step s, bytes [64 s + 32 h, +32) of row m of
// BOTH operands; whatever order the instruction gives the 64 k of a step inside the two lane halves, it is the same for A
// and B, so the sum is over all 64.  A row's amax needs the lane's own 256 values and one exchange between the halves.
//
// One step of the tile loop: barrier (every wave's pieces of tile i have landed, tile i - 1 is dead) -- the stores of the
// tile packed a step ago -- the requests for tile i + 2 into the dead slot -- 8 MFMAs -- scales, bias, packing -- wait until
// only those two requests are in flight (vmcnt counts in issue order, so tile i + 1 has landed).
//
// Work distribution, row statistics (but see the centred pass's threshold), the output's path through the wave's LDS
// staging: as in hstu_ln_linear.cuh.
#pragma once
#include "hstu_ln_linear.cuh"

namespace hstu {

constexpr int kL8K = 512;
constexpr int kL8Waves = 8;
constexpr int kL8Threads = 64 * kL8Waves;
constexpr int kL8BlockRows = 32 * kL8Waves;
constexpr int kL8Steps = kL8K / 64;             // MFMAs per 32 x 32 output tile
constexpr int kL8TileBytes = 32 * kL8K;         // 16 KiB
constexpr int kL8Stages = 3;
constexpr int kL8RingBytes = kL8Stages * kL8TileBytes;
constexpr int kL8MaxN = 4096;
constexpr int kL8StageBytes = 2048;             // per wave: 32 rows x 64 bytes of y on their way out
constexpr float kE4m3Max = 448.0f;

typedef int i32x8 __attribute__((ext_vector_type(8)));

// The MFMA's own block scales: 0 emits the unscaled v_mfma_f32_32x32x64_f8f6f4, 127 (E8M0 of 2^0) the _scale_ form with both
// scales 1 -- the same arithmetic (the row-wise scales are applied in the epilogue).  tools/bench_ln_linear.py --fp8 on a
// variant library (tools/build_variant.sh) compares them: DESIGN.md 4.4.
#ifndef L8_MFMA_SCALE
#define L8_MFMA_SCALE 0
#endif

struct LnLinearFp8Args {
  const void* x;              // LN: (rows, 512) 16-bit, leading dimension ldx; else the e4m3 codes, rows x 512 bytes
  const void* ln_w; const void* ln_b;
  const float* x_scale_in;    // without the LayerNorm
  const void* wq; const float* w_scale; const void* bias;
  void* y; void* xq; float* x_scale; float* mean; float* rstd;
  int64_t rows, ldx, ldy;
  int64_t units;              // row blocks x column tiles
  int n, n_tiles;
  float eps;
};

static inline int l8_smem_bytes(int n) { return kL8RingBytes + 2 * kL8K * 4 + 2 * n * 4 + kL8Waves * kL8StageBytes; }   // ring, LN tables, bias + w_scale, staging

HSTU_DEV float l8_scale_of(float amax) { return amax > 0.f ? amax / kE4m3Max : 1.0f; }
HSTU_DEV float l8_scaled(float v, float scale) {
  const float q = v / scale;      // (correctly rounded: hipcc's default fp32 division)
  return fminf(fmaxf(q, -kE4m3Max), kE4m3Max);
}
HSTU_DEV uint32_t l8_pack4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}

// The 32 rows of the calling wave as e4m3 operand fragments: xq[s] = bytes [64 s + 32 h, +32) of row `lane & 31`
// (h = lane >> 5); returns the row's scale.  Rows past the end repeat the last row and are never stored.
template <typename T, bool LN>
HSTU_DEV float l8_load_rows(const LnLinearFp8Args& g, int64_t row0, const float* gam, const float* bet, int lane, i32x8 (&xq)[kL8Steps]) {
  const int m = lane & 31, h = lane >> 5;
  const int64_t row = row0 + m;
  const bool ok = row < g.rows;
  const int64_t crow = ok ? row : g.rows - 1;
  if constexpr (!LN) {
    const char* xp = (const char*)g.x + crow * kL8K + 32 * h;
#pragma unroll
    for (int s = 0; s < kL8Steps; ++s) {
      const u32x4 a = gload16(xp + 64 * s), b = gload16(xp + 64 * s + 16);
      xq[s] = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
    }
    return g.x_scale_in[crow];
  } else {
    using DT = LnlDot<T>;
    // raw[4 s + i]: elements [64 s + 32 h + 8 i, +8) of the row
    u32x4 raw[4 * kL8Steps];
    const char* xp = (const char*)g.x + (crow * g.ldx + 32 * h) * 2;
#pragma unroll
    for (int s = 0; s < kL8Steps; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) raw[4 * s + i] = gload16(xp + 128 * s + 16 * i);
    float sm = 0.f, sq = 0.f;
#pragma unroll
    for (int r = 0; r < 4 * kL8Steps; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sm = DT::dot(raw[r][j], DT::kOnes, sm);
        sq = DT::dot(raw[r][j], raw[r][j], sq);
      }
    sm += __shfl_xor(sm, 32);
    sq += __shfl_xor(sq, 32);
    const float mean = sm * (1.0f / kL8K);
    const float ex2 = sq * (1.0f / kL8K);
    float var = ex2 - mean * mean;
    // The one-pass variance loses a factor E[x^2] / var of the sums' ~3e-7 relative rounding; the e4m3 codes and x_scale want
    // rstd to 2e-6, so the wave takes the centred form as soon as a row's mean exceeds its sigma (the 16-bit kernel, whose
    // rounding of normed_x hides more, waits for 8 sigma).  Also for NaN.
    // The branch is the wave's, the choice the row's: a row's bits may not depend on its neighbours.
    const bool centred = !(ex2 <= 2.f * var);
    if (__builtin_amdgcn_ballot_w64(centred) != 0) {
      float c = 0.f;
#pragma unroll
      for (int r = 0; r < 4 * kL8Steps; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d0 = DT::lo(raw[r][j]) - mean, d1 = DT::hi(raw[r][j]) - mean;
          c += d0 * d0;
          c += d1 * d1;
        }
        if (r % 4 == 3) __builtin_amdgcn_sched_barrier(0);
      }
      c += __shfl_xor(c, 32);
      if (centred) var = c * (1.0f / kL8K);
#pragma unroll
      for (int r = 0; r < 4 * kL8Steps; ++r) asm volatile("" : "+v"(raw[r]));   // or the unpacked values are kept for the passes below
    }
    const float rstd = 1.0f / sqrtf(var + g.eps);
    const float nmr = -mean * rstd;
    if (ok && h == 0) {
      if (g.mean) g.mean[row] = mean;
      if (g.rstd) g.rstd[row] = rstd;
    }
    // the eight normalised values of raw[r], in fp32
    auto normed8 = [&](int r, float (&v)[8]) {
      const int e0 = 64 * (r >> 2) + 32 * h + 8 * (r & 3);
      const f32x4 g0 = *LDS_PTR(const f32x4, gam + e0), g1 = *LDS_PTR(const f32x4, gam + e0 + 4);
      const f32x4 b0 = *LDS_PTR(const f32x4, bet + e0), b1 = *LDS_PTR(const f32x4, bet + e0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float ga = j < 2 ? g0[2 * j] : g1[2 * j - 4], gb = j < 2 ? g0[2 * j + 1] : g1[2 * j - 3];
        const float ba = j < 2 ? b0[2 * j] : b1[2 * j - 4], bb = j < 2 ? b0[2 * j + 1] : b1[2 * j - 3];
        const float t0 = __builtin_fmaf(DT::lo(raw[r][j]), rstd, nmr), t1 = __builtin_fmaf(DT::hi(raw[r][j]), rstd, nmr);
        v[2 * j] = __builtin_fmaf(t0, ga, ba);
        v[2 * j + 1] = __builtin_fmaf(t1, gb, bb);
      }
    };
    float amax = 0.f;
#pragma unroll
    for (int r = 0; r < 4 * kL8Steps; ++r) {
      float v[8];
      normed8(r, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
      asm volatile("" : "+v"(amax));
      __builtin_amdgcn_sched_barrier(0);   // or the scheduler hoists all the table reads
    }
    amax = fmaxf(amax, __shfl_xor(amax, 32));
    const float scale = l8_scale_of(amax);
#pragma unroll
    for (int r = 0; r < 4 * kL8Steps; ++r) asm volatile("" : "+v"(raw[r]));   // or the 256 values of the pass above are kept (spilled) for the one below
#pragma unroll
    for (int r = 0; r < 4 * kL8Steps; ++r) {
      float v[8];
      normed8(r, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = l8_scaled(v[j], scale);
      xq[r >> 2][2 * (r & 3)] = (int)l8_pack4(v[0], v[1], v[2], v[3]);
      xq[r >> 2][2 * (r & 3) + 1] = (int)l8_pack4(v[4], v[5], v[6], v[7]);
      asm volatile("" : "+v"(xq[r >> 2][2 * (r & 3)]), "+v"(xq[r >> 2][2 * (r & 3) + 1]));   // converted HERE: the 16-bit words die as the codes appear
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ok) {
      if (g.xq) {
        char* qp = (char*)g.xq + row * kL8K + 32 * h;
#pragma unroll
        for (int s = 0; s < kL8Steps; ++s) {
          gstore16(qp + 64 * s, u32x4{(uint32_t)xq[s][0], (uint32_t)xq[s][1], (uint32_t)xq[s][2], (uint32_t)xq[s][3]});
          gstore16(qp + 64 * s + 16, u32x4{(uint32_t)xq[s][4], (uint32_t)xq[s][5], (uint32_t)xq[s][6], (uint32_t)xq[s][7]});
        }
      }
      if (g.x_scale && h == 0) g.x_scale[row] = scale;
    }
    return scale;
  }
}

// unit u (16 bytes) of row r of a ring tile sits in slot u ^ (r & 15) of its 512-byte row: the 16 lanes of a ds_read_b128
// group (16 consecutive rows, one unit column) then hit 16 different 16-byte slots of the 256-byte bank window
HSTU_DEV uint32_t l8_tile_off(int r, int u) { return (uint32_t)(r * kL8K + ((u ^ (r & 15)) << 4)); }

template <typename T, bool LN>
__global__ __launch_bounds__(kL8Threads) __attribute__((amdgpu_waves_per_eu(2, 2)))
void hstu_lnl_fp8_fwd_kernel(const LnLinearFp8Args g) {
  extern __shared__ __attribute__((aligned(1024))) char l8_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 31, h = lane >> 5;
  char* ring = l8_smem;
  float* gam = (float*)(l8_smem + kL8RingBytes);
  float* bet = gam + kL8K;
  float* bia = bet + kL8K;
  float* wsc = bia + g.n;
  if constexpr (LN) {
    for (int i = tid; i < kL8K; i += kL8Threads) {
      gam[i] = (float)((const T*)g.ln_w)[i];
      bet[i] = (float)((const T*)g.ln_b)[i];
    }
  }
  for (int i = tid; i < g.n; i += kL8Threads) {
    bia[i] = g.bias ? (float)((const T*)g.bias)[i] : 0.f;
    wsc[i] = g.w_scale[i];
  }

  const int64_t u0 = g.units * blockIdx.x / gridDim.x, u1 = g.units * (blockIdx.x + 1) / gridDim.x;
  const int nsteps = (int)(u1 - u0);
  if (nsteps <= 0) return;
  int64_t blk = u0 / g.n_tiles;
  int tile = (int)(u0 - blk * g.n_tiles);

  // the wave's share of a tile's DMA: two 1 KiB instructions, each two 512-byte rows (4 wave + 2 j + (lane >> 5)); the lane
  // that fills physical unit `lane & 31` of row r fetches logical unit (lane & 31) ^ (r & 15)
  uint32_t uo[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = 4 * wave + 2 * j + h;
    uo[j] = (uint32_t)(r * kL8K + (((lane & 31) ^ (r & 15)) << 4));
  }
  const uint32_t ring0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)ring);
  int it = tile, islot = 0, issued = 0;
  auto issue = [&]() {
    const char* base = (const char*)g.wq + (int64_t)it * kL8TileBytes;
#pragma unroll
    for (int j = 0; j < 2; ++j) lnl_dma16(uo[j], base, ring0 + islot * kL8TileBytes + (2 * wave + j) * 1024);
    it = it + 1 == g.n_tiles ? 0 : it + 1;
    islot = islot + 1 == kL8Stages ? 0 : islot + 1;
    ++issued;
  };
  for (int i = 0; i < kL8Stages - 1 && i < nsteps; ++i) issue();
  __syncthreads();   // gam / bet / bia / wsc

  char* stage = (char*)(wsc + g.n) + wave * kL8StageBytes;
  i32x8 xq[kL8Steps];
  float xs = 1.0f;
  LnlPacked pk;
  char* pk_dst = nullptr;
  bool have_pk = false;
  bool ok_lo = false, ok_hi = false;
  char* row_dst = nullptr;
  auto store_packed = [&]() {
    if (ok_lo) gstore16_nt(pk_dst, pk.lo);
    if (ok_hi) gstore16_nt(pk_dst + 16 * g.ldy * 2, pk.hi);
  };

  // the wave's pieces of the first tile (requested first; vmcnt counts in issue order)
  if (nsteps > 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  int cslot = 0;
  bool need_rows = true;
  for (int i = 0; i < nsteps; ++i) {
    if (need_rows) {
      if (have_pk) { store_packed(); have_pk = false; }
      const int64_t row0 = blk * kL8BlockRows + wave * 32;
      xs = l8_load_rows<T, LN>(g, row0, gam, bet, lane, xq);
      const int64_t row = row0 + (lane >> 2);      // the lane's rows at store time: row, row + 16
      ok_lo = row < g.rows;
      ok_hi = row + 16 < g.rows;
      row_dst = (char*)g.y + row * g.ldy * 2 + 16 * (lane & 3);
      // said to the compiler as an instruction it counts: or every step of the tile loop waits for "the rows' loads" with
      // vmcnt(0), and with them for the ring's requests
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
      need_rows = false;
    }
    lds_barrier();       // tile i is in the ring (every wave waited for its pieces); nobody reads tile i - 1 any more
    if (have_pk) store_packed();
    const bool do_issue = issued < nsteps;
    if (do_issue) issue();

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const uint32_t tb = ring0 + cslot * kL8TileBytes;
    // all 16 fragment reads of the tile go out at once (64 registers); the MFMAs follow them with counted waits
    i32x8 wf[kL8Steps];
#pragma unroll
    for (int s = 0; s < kL8Steps; ++s) {
      const u32x4 a0 = *LDS_PTR(const u32x4, (uintptr_t)(tb + l8_tile_off(m, 4 * s + 2 * h)));
      const u32x4 a1 = *LDS_PTR(const u32x4, (uintptr_t)(tb + l8_tile_off(m, 4 * s + 2 * h + 1)));
      wf[s] = i32x8{(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < kL8Steps; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[s], xq[s], acc, 0, 0, 0, L8_MFMA_SCALE, 0, L8_MFMA_SCALE);
    // register r of lane (m, h): column (r & 3) + 8 (r >> 2) + 4 h of the tile, row m of the wave
    {
      const float* bt = bia + tile * 32 + 4 * h;
      const float* st = wsc + tile * 32 + 4 * h;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 b4 = *LDS_PTR(const f32x4, bt + 8 * j);
        const f32x4 s4 = *LDS_PTR(const f32x4, st + 8 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * j + e] = __builtin_fmaf(acc[4 * j + e] * xs, s4[e], b4[e]);
      }
    }
    pk = lnl_pack_tile<T>(acc, stage, lane);
    pk_dst = row_dst + tile * 64;
    have_pk = true;
    // behind tile i + 1's requests there are only this step's two (the stores went out before them)
    if (do_issue) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    cslot = cslot + 1 == kL8Stages ? 0 : cslot + 1;
    if (++tile == g.n_tiles) { tile = 0; ++blk; need_rows = true; }
  }
  if (have_pk) store_packed();
}

template <typename T>
static int launch_ln_linear_fp8(const LnLinearFp8Args& g, hipStream_t st) {
  const int smem = l8_smem_bytes(g.n);
  auto kern = g.ln_w ? hstu_lnl_fp8_fwd_kernel<T, true> : hstu_lnl_fp8_fwd_kernel<T, false>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  if (e != hipSuccess) return set_error(HSTU_ELAUNCH, "ln_linear_fp8_fwd: cannot reserve %d bytes of LDS: %s", smem, hipGetErrorString(e));
  const int n_cu = cu_count();
  const int grid = (int)(g.units < n_cu ? g.units : n_cu);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kL8Threads), smem, st, g);
  return check_launch("ln_linear_fp8_fwd");
}

template <typename T>
HSTU_DEV void l8_load16(const char* p, float (&f)[16]) {
  if constexpr (sizeof(T) == 2) {
    typedef T t8 __attribute__((ext_vector_type(8)));
    const t8 a = __builtin_bit_cast(t8, gload16(p)), b = __builtin_bit_cast(t8, gload16(p + 16));
#pragma unroll
    for (int j = 0; j < 8; ++j) { f[j] = (float)a[j]; f[8 + j] = (float)b[j]; }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 a = __builtin_bit_cast(f32x4, gload16(p + 16 * q));
#pragma unroll
      for (int j = 0; j < 4; ++j) f[4 * q + j] = a[j];
    }
  }
}

// Row-wise e4m3 quantizer: one wave per row, k a multiple of 16 up to 4096.  Lane l holds elements [16 (l + 64 i), +16),
// i < 4, as fp32 between the amax and the conversion: the row is read once.
constexpr int kQ8Threads = 256;
constexpr int kQ8MaxK = 4096;
template <typename T>
__global__ __launch_bounds__(kQ8Threads) void hstu_quantize_rows_fp8_kernel(const char* src, int64_t ld, int64_t rows, int k,
                                                                            uint8_t* dst, float* scale) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kQ8Threads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const char* sp = src + row * ld * (int64_t)sizeof(T);
  const int chunks = k >> 4;
  float v[4][16];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      l8_load16<T>(sp + (int64_t)c * 16 * sizeof(T), v[i]);
#pragma unroll
      for (int j = 0; j < 16; ++j) amax = fmaxf(amax, fabsf(v[i][j]));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  const float s = l8_scale_of(amax);
  if (lane == 0) scale[row] = s;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = l8_pack4(l8_scaled(v[i][4 * j], s), l8_scaled(v[i][4 * j + 1], s), l8_scaled(v[i][4 * j + 2], s), l8_scaled(v[i][4 * j + 3], s));
      gstore16(dst + row * k + (int64_t)c * 16, o);
    }
  }
}

}  // namespace hstu
