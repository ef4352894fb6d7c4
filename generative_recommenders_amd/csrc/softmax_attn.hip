// Jagged causal softmax attention for gfx950, forward and backward (the SASRec baseline's attention, include/hstu_hip.h).
//
// Structure.  One wavefront (a 64-thread workgroup) owns a 32-row tile of one (user, head) and walks the
// tiles it meets; every score product is formed TRANSPOSED, so that the lane owns the row whose statistics it needs:
//   forward, dQ kernel:  S^T[key][query] = K Q^T     C layout: lane (n32, hf) holds 16 keys of query n32
//   dK / dV kernel:      S[query][key]   = Q K^T     lane (n32, hf) holds 16 queries of key n32
// The 16 values a lane holds are, in this order, exactly the contraction slots (hf, j) of the next product's B operand
// (rows 16 s + 4 hf + j and 16 s + 8 + 4 hf + j - 4 for step s), so P / dS go from the accumulator through one pack8 into the
// next MFMA without touching LDS, and the running maximum / sum / lse / delta of a row are lane-local (one shuffle across
// the two halves).  The other operand of those products is a tile read ACROSS its rows (lds_col_frag), which is what LDS is
// used for: the forward stages V, the dQ kernel K, the dK / dV kernel Q and dO -- 32 x D elements each.  Operands contracted
// along the head dim come straight from global memory as 16-byte row pieces (gload16), zero-filled past the user's length
// and past the real head dim.
//   forward:  online softmax in the base-2 domain, t = s (scale log2 e): m = running max, l = running sum of exp2(t - m)
//             of the UN-dropped scores, P~ = exp2(t - m) rounded once to the I/O dtype in front of P V, O = acc keep_scale / l
//             rounded once, lse = (m + log2 l) ln 2.
//   backward: P = exp2(t - lse log2 e) recomputed; delta = rowsum(dO o O) by the dQ kernel (first launch) into `delta`, read
//             by the dK / dV kernel (second launch); dS = P (dP keep - delta) rounded once; dV = (P keep)^T dO.  Every output
//             row is written by one wavefront: no float atomics.
// Dropout: element index e = (r H + h) max_seq_len + j (r global query row, j key position in its user), drop_hash.cuh.
#include "capi_internal.h"
#include "drop_hash.cuh"
#include "hstu_common.cuh"

namespace hstu {
namespace {

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;

struct SmDrop {
  uint32_t thr;   // 0 = no dropout
  float scale;
  uint32_t s0, s1;
};

// position inside a 32-row tile of accumulator register r of half hf (C layout of the 32x32 MFMA)
HSTU_DEV int acc_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

// elements [e0, e0 + 8) of a row as a fragment, zero when the row is past the user's length or the piece past the head dim
template <typename T> HSTU_DEV typename Elem<T>::Frag gload_frag(const T* row, int e0, int d, bool ok) {
  typename Elem<T>::Frag f;
  const u32x4 z = {0u, 0u, 0u, 0u};
  if constexpr (Elem<T>::kBytes == 2) {
    const u32x4 x = (ok && e0 < d) ? gload16(row + e0) : z;
    f.v = __builtin_bit_cast(typename Elem<T>::vec8, x);
  } else {
    const u32x4 x0 = (ok && e0 < d) ? gload16(row + e0) : z;
    const u32x4 x1 = (ok && e0 + 4 < d) ? gload16(row + e0 + 4) : z;
    const f32x4 a = __builtin_bit_cast(f32x4, x0), b = __builtin_bit_cast(f32x4, x1);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  }
  return f;
}

// rows [r0, r0 + 32) of one head -> a swizzled [32][D] LDS tile; rows >= len and columns >= d are zero
template <typename T, int D>
HSTU_DEV void stage_tile(char* tile, const T* base, int64_t row_stride, int r0, int len, int d, int lane) {
  constexpr int EPU = 16 / (int)sizeof(T), UPR = D / EPU;
  const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 32 * UPR / 64; ++i) {
    const int u = lane + 64 * i, row = u / UPR, unit = u % UPR;
    const bool ok = (r0 + row < len) && (unit * EPU < d);
    const u32x4 x = ok ? gload16(base + (int64_t)(r0 + row) * row_stride + unit * EPU) : z;
    *LDS_PTR(u32x4, tile + tile_off<UPR>(row, unit)) = x;
  }
}

// four consecutive elements d0 .. d0 + 3 of an output row
template <typename T> HSTU_DEV void store4(T* p, float a, float b, float c, float e) {
  if constexpr (Elem<T>::kBytes == 2) {
    const u32x2 w = {Elem<T>::pk2(a, b), Elem<T>::pk2(c, e)};
    *GLOBAL_PTR(u32x2, p) = w;
  } else {
    const f32x4 w = {a, b, c, e};
    gstore16(p, __builtin_bit_cast(u32x4, w));
  }
}

// acc^T[blk] (C layout: row = d, col = the lane's output row) * mul -> contiguous (rows, H, d) output row `dst`
template <typename T, int NB> HSTU_DEV void store_row_t(T* dst, const f32x16* acc, float mul, int d, int hf) {
#pragma unroll
  for (int blk = 0; blk < NB; ++blk)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = 32 * blk + 8 * g + 4 * hf;
      if (d0 < d) store4<T>(dst + d0, acc[blk][4 * g] * mul, acc[blk][4 * g + 1] * mul, acc[blk][4 * g + 2] * mul, acc[blk][4 * g + 3] * mul);
    }
}

// keep factor (0 or the survivor scale) of element (query row base e_row, key position j)
HSTU_DEV float keep_factor(const SmDrop& dc, uint64_t e_row, int j) {
  return drop_r16(e_row + (uint64_t)j, dc.s0, dc.s1) >= dc.thr ? dc.scale : 0.f;
}

struct Problem {
  int b, h, tile, len;
  int64_t start;
};
// workgroup -> (user, head, tile); the longest tiles of a user first.  false: nothing to do.
HSTU_DEV bool decode_problem(const SoftmaxAttnArgs& a, Problem& p) {
  const int tiles = (a.max_seq_len + 31) >> 5;
  const int64_t w = blockIdx.x;
  p.tile = tiles - 1 - (int)(w % tiles);
  const int64_t bh = w / tiles;
  p.h = (int)(bh % a.heads);
  p.b = (int)(bh / a.heads);
  p.start = load_index(a.offsets, p.b, a.index_dtype);
  const int64_t len = load_index(a.offsets, p.b + 1, a.index_dtype) - p.start;
  p.len = (int)(len < a.max_seq_len ? len : a.max_seq_len);
  return p.tile * 32 < p.len;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ forward
template <typename T, int D>
__global__ __launch_bounds__(64) void hstu_softmax_attn_fwd_kernel(const SoftmaxAttnArgs a, const SmDrop dc) {
  constexpr int NS = D / 16, NB = D / 32, UPR = D * (int)sizeof(T) / 16;
  __shared__ __attribute__((aligned(16))) char vt[32 * D * sizeof(T)];
  Problem pr;
  if (!decode_problem(a, pr)) return;
  const int lane = threadIdx.x, n32 = lane & 31, hf = lane >> 5;
  const int d = a.head_dim, H = a.heads;
  const int qi = pr.tile * 32 + n32;
  const bool q_ok = qi < pr.len;
  const int64_t qrow = pr.start + qi;
  const T* kbase = (const T*)a.k + pr.start * a.k_rs + (int64_t)pr.h * a.k_hs;
  const T* vbase = (const T*)a.v + pr.start * a.v_rs + (int64_t)pr.h * a.v_hs;

  typename Elem<T>::Frag qf[NS];
  {
    const T* qp = (const T*)a.q + qrow * a.q_rs + (int64_t)pr.h * a.q_hs;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = gload_frag<T>(qp, 16 * s + 8 * hf, d, q_ok);
  }
  const float c = a.scale * kLog2e;
  const uint64_t e_row = ((uint64_t)qrow * (uint64_t)H + (uint64_t)pr.h) * (uint64_t)a.max_seq_len;
  float m = -INFINITY, l = 0.f;
  f32x16 acc[NB];
#pragma unroll
  for (int blk = 0; blk < NB; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[blk][r] = 0.f;

  for (int kt = 0; kt <= pr.tile; ++kt) {
    const int k0 = kt * 32;
    stage_tile<T, D>(vt, vbase, a.v_rs, k0, pr.len, d, lane);
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
    {
      const bool k_ok = k0 + n32 < pr.len;
      const T* kp = kbase + (int64_t)(k0 + n32) * a.k_rs;
#pragma unroll
      for (int s = 0; s < NS; ++s) st = Elem<T>::mma(gload_frag<T>(kp, 16 * s + 8 * hf, d, k_ok), qf[s], st);
    }
    float t[16], mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, hf);
      t[r] = key <= qi ? st[r] * c : -INFINITY;
      mx = fmaxf(mx, t[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx);          // finite from the first tile on: key 0 is visible to every row
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    m = m_new;
    l *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      t[r] = __builtin_amdgcn_exp2f(t[r] - m_new);
      l += t[r];
    }
    if (dc.thr) {
#pragma unroll
      for (int r = 0; r < 16; ++r) t[r] = keep_factor(dc, e_row, k0 + acc_row(r, hf)) != 0.f ? t[r] : 0.f;
    }
    typename Elem<T>::Frag pf[2] = {Elem<T>::pack8(t), Elem<T>::pack8(t + 8)};
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[blk][r] *= alpha;
    __syncthreads();
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        acc[blk] = Elem<T>::mma(lds_col_frag<T, UPR>(vt, 16 * s + 4 * hf, 16 * s + 8 + 4 * hf, 32 * blk, lane), pf[s], acc[blk]);
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);
  if (q_ok) {
    const float inv = (dc.thr ? dc.scale : 1.f) / l;
    store_row_t<T, NB>((T*)a.out + (qrow * H + pr.h) * (int64_t)d, acc, inv, d, hf);
    if (hf == 0) ((float*)a.lse)[qrow * H + pr.h] = (m + __builtin_amdgcn_logf(l)) * kLn2;
  }
}

// ------------------------------------------------------------------------------------------------------------ backward: dQ
template <typename T, int D>
__global__ __launch_bounds__(64) void hstu_softmax_attn_bwd_dq_kernel(const SoftmaxAttnArgs a, const SmDrop dc) {
  constexpr int NS = D / 16, NB = D / 32, UPR = D * (int)sizeof(T) / 16;
  __shared__ __attribute__((aligned(16))) char ktile[32 * D * sizeof(T)];
  Problem pr;
  if (!decode_problem(a, pr)) return;
  const int lane = threadIdx.x, n32 = lane & 31, hf = lane >> 5;
  const int d = a.head_dim, H = a.heads;
  const int qi = pr.tile * 32 + n32;
  const bool q_ok = qi < pr.len;
  const int64_t qrow = pr.start + qi;
  const T* kbase = (const T*)a.k + pr.start * a.k_rs + (int64_t)pr.h * a.k_hs;
  const T* vbase = (const T*)a.v + pr.start * a.v_rs + (int64_t)pr.h * a.v_hs;

  typename Elem<T>::Frag qf[NS], gf[NS];
  float delta = 0.f;
  {
    const T* qp = (const T*)a.q + qrow * a.q_rs + (int64_t)pr.h * a.q_hs;
    const T* gp = (const T*)a.dout + (qrow * H + pr.h) * (int64_t)d;
    const T* op = (const T*)a.out + (qrow * H + pr.h) * (int64_t)d;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      qf[s] = gload_frag<T>(qp, 16 * s + 8 * hf, d, q_ok);
      gf[s] = gload_frag<T>(gp, 16 * s + 8 * hf, d, q_ok);
      const typename Elem<T>::Frag of = gload_frag<T>(op, 16 * s + 8 * hf, d, q_ok);
#pragma unroll
      for (int j = 0; j < 8; ++j) delta += (float)gf[s].v[j] * (float)of.v[j];
    }
  }
  delta += __shfl_xor(delta, 32, 64);
  const float lse2 = q_ok ? a.lse[qrow * H + pr.h] * kLog2e : 0.f;
  if (q_ok && hf == 0) a.delta[qrow * H + pr.h] = delta;
  const float c = a.scale * kLog2e;
  const uint64_t e_row = ((uint64_t)qrow * (uint64_t)H + (uint64_t)pr.h) * (uint64_t)a.max_seq_len;
  f32x16 acc[NB];
#pragma unroll
  for (int blk = 0; blk < NB; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[blk][r] = 0.f;

  for (int kt = 0; kt <= pr.tile; ++kt) {
    const int k0 = kt * 32;
    stage_tile<T, D>(ktile, kbase, a.k_rs, k0, pr.len, d, lane);
    f32x16 dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) dp[r] = 0.f;
    {
      const bool k_ok = k0 + n32 < pr.len;
      const T* vp = vbase + (int64_t)(k0 + n32) * a.v_rs;
#pragma unroll
      for (int s = 0; s < NS; ++s) dp = Elem<T>::mma(gload_frag<T>(vp, 16 * s + 8 * hf, d, k_ok), gf[s], dp);
    }
    __syncthreads();
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) st = Elem<T>::mma(lds_row_frag<T, UPR>(ktile, n32, 16 * s + 8 * hf), qf[s], st);
    float ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, hf);
      const float p = (key <= qi && q_ok) ? __builtin_amdgcn_exp2f(st[r] * c - lse2) : 0.f;
      const float kf = dc.thr ? keep_factor(dc, e_row, key) : 1.f;
      ds[r] = p * (dp[r] * kf - delta);
    }
    typename Elem<T>::Frag sf[2] = {Elem<T>::pack8(ds), Elem<T>::pack8(ds + 8)};
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        acc[blk] = Elem<T>::mma(lds_col_frag<T, UPR>(ktile, 16 * s + 4 * hf, 16 * s + 8 + 4 * hf, 32 * blk, lane), sf[s], acc[blk]);
    __syncthreads();
  }
  if (q_ok) store_row_t<T, NB>((T*)a.dq + (qrow * H + pr.h) * (int64_t)d, acc, a.scale, d, hf);
}

// ------------------------------------------------------------------------------------------------------- backward: dK and dV
template <typename T, int D>
__global__ __launch_bounds__(64) void hstu_softmax_attn_bwd_dkv_kernel(const SoftmaxAttnArgs a, const SmDrop dc) {
  constexpr int NS = D / 16, NB = D / 32, UPR = D * (int)sizeof(T) / 16;
  __shared__ __attribute__((aligned(16))) char qtile[32 * D * sizeof(T)];
  __shared__ __attribute__((aligned(16))) char gtile[32 * D * sizeof(T)];
  __shared__ __attribute__((aligned(16))) float stats[64];   // lse log2 e, delta of the 32 query rows
  Problem pr;
  if (!decode_problem(a, pr)) return;
  const int lane = threadIdx.x, n32 = lane & 31, hf = lane >> 5;
  const int d = a.head_dim, H = a.heads;
  const int kj = pr.tile * 32 + n32;
  const bool k_ok = kj < pr.len;
  const int64_t krow = pr.start + kj;
  const T* qbase = (const T*)a.q + pr.start * a.q_rs + (int64_t)pr.h * a.q_hs;
  const T* gbase = (const T*)a.dout + (pr.start * H + pr.h) * (int64_t)d;
  const int64_t g_rs = (int64_t)H * d;

  typename Elem<T>::Frag kf_[NS], vf[NS];
  {
    const T* kp = (const T*)a.k + krow * a.k_rs + (int64_t)pr.h * a.k_hs;
    const T* vp = (const T*)a.v + krow * a.v_rs + (int64_t)pr.h * a.v_hs;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      kf_[s] = gload_frag<T>(kp, 16 * s + 8 * hf, d, k_ok);
      vf[s] = gload_frag<T>(vp, 16 * s + 8 * hf, d, k_ok);
    }
  }
  const float c = a.scale * kLog2e;
  f32x16 dk[NB], dv[NB];
#pragma unroll
  for (int blk = 0; blk < NB; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[blk][r] = 0.f; dv[blk][r] = 0.f; }

  const int last = (pr.len - 1) >> 5;
  for (int qt = pr.tile; qt <= last; ++qt) {
    const int q0 = qt * 32;
    stage_tile<T, D>(qtile, qbase, a.q_rs, q0, pr.len, d, lane);
    stage_tile<T, D>(gtile, gbase, g_rs, q0, pr.len, d, lane);
    {
      const bool ok = q0 + n32 < pr.len;
      const int64_t idx = (pr.start + q0 + n32) * H + pr.h;
      stats[lane] = ok ? (hf ? a.delta[idx] : a.lse[idx] * kLog2e) : 0.f;
    }
    __syncthreads();
    f32x16 st, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      st = Elem<T>::mma(lds_row_frag<T, UPR>(qtile, n32, 16 * s + 8 * hf), kf_[s], st);
      dp = Elem<T>::mma(lds_row_frag<T, UPR>(gtile, n32, 16 * s + 8 * hf), vf[s], dp);
    }
    float pd[16], ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qloc = acc_row(r, hf), qi = q0 + qloc;
      const float lse2 = stats[qloc], delta = stats[32 + qloc];
      const float p = (kj <= qi && qi < pr.len) ? __builtin_amdgcn_exp2f(st[r] * c - lse2) : 0.f;
      float kf = 1.f;
      if (dc.thr) {
        const uint64_t e_row = ((uint64_t)(pr.start + qi) * (uint64_t)H + (uint64_t)pr.h) * (uint64_t)a.max_seq_len;
        kf = keep_factor(dc, e_row, kj);
      }
      pd[r] = p * kf;
      ds[r] = p * (dp[r] * kf - delta);
    }
    typename Elem<T>::Frag pf[2] = {Elem<T>::pack8(pd), Elem<T>::pack8(pd + 8)};
    typename Elem<T>::Frag sf[2] = {Elem<T>::pack8(ds), Elem<T>::pack8(ds + 8)};
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        dv[blk] = Elem<T>::mma(lds_col_frag<T, UPR>(gtile, 16 * s + 4 * hf, 16 * s + 8 + 4 * hf, 32 * blk, lane), pf[s], dv[blk]);
        dk[blk] = Elem<T>::mma(lds_col_frag<T, UPR>(qtile, 16 * s + 4 * hf, 16 * s + 8 + 4 * hf, 32 * blk, lane), sf[s], dk[blk]);
      }
    __syncthreads();
  }
  if (k_ok) {
    store_row_t<T, NB>((T*)a.dk + (krow * H + pr.h) * (int64_t)d, dk, a.scale, d, hf);
    store_row_t<T, NB>((T*)a.dv + (krow * H + pr.h) * (int64_t)d, dv, 1.f, d, hf);
  }
}

// ------------------------------------------------------------------------------------------------------------------ launchers
namespace {
SmDrop make_sm_drop(const SoftmaxAttnArgs& a) {
  SmDrop dc;
  dc.thr = drop_threshold(a.dropout_p);
  dc.scale = drop_scale(dc.thr);
  dc.s0 = (uint32_t)a.seed;
  dc.s1 = (uint32_t)(a.seed >> 32);
  return dc;
}

int grid_of(const SoftmaxAttnArgs& a, const char* who, unsigned* grid) {
  const int64_t n = (int64_t)a.batch * a.heads * ((a.max_seq_len + 31) >> 5);
  if (n > 0x7fffffffLL) return set_error(HSTU_EUNSUPPORTED, "%s: batch x heads x tiles = %lld workgroups exceed the grid limit", who, (long long)n);
  *grid = (unsigned)n;
  return HSTU_OK;
}

template <typename T, int D> int fwd_t(const SoftmaxAttnArgs& a, unsigned grid, hipStream_t st) {
  hipLaunchKernelGGL((hstu_softmax_attn_fwd_kernel<T, D>), dim3(grid), dim3(64), 0, st, a, make_sm_drop(a));
  return check_launch("hstu_softmax_attn_fwd");
}
template <typename T, int D> int bwd_t(const SoftmaxAttnArgs& a, unsigned grid, hipStream_t st) {
  const SmDrop dc = make_sm_drop(a);
  hipLaunchKernelGGL((hstu_softmax_attn_bwd_dq_kernel<T, D>), dim3(grid), dim3(64), 0, st, a, dc);   // writes delta
  if (int e = check_launch("hstu_softmax_attn_bwd (dQ)")) return e;
  hipLaunchKernelGGL((hstu_softmax_attn_bwd_dkv_kernel<T, D>), dim3(grid), dim3(64), 0, st, a, dc);  // reads delta
  return check_launch("hstu_softmax_attn_bwd (dK, dV)");
}
template <typename T> int fwd_d(const SoftmaxAttnArgs& a, unsigned grid, hipStream_t st) {
  return softmax_attn_head_dim(a.head_dim) == 32 ? fwd_t<T, 32>(a, grid, st) : fwd_t<T, 64>(a, grid, st);
}
template <typename T> int bwd_d(const SoftmaxAttnArgs& a, unsigned grid, hipStream_t st) {
  return softmax_attn_head_dim(a.head_dim) == 32 ? bwd_t<T, 32>(a, grid, st) : bwd_t<T, 64>(a, grid, st);
}
}  // namespace

int launch_softmax_attn_fwd(const SoftmaxAttnArgs& a, hipStream_t st) {
  unsigned grid = 0;
  if (int e = grid_of(a, "hstu_softmax_attn_fwd", &grid)) return e;
  switch (a.dtype) {
    case HSTU_DTYPE_BF16: return fwd_d<bf16_t>(a, grid, st);
    case HSTU_DTYPE_F16: return fwd_d<f16_t>(a, grid, st);
    default: return fwd_d<float>(a, grid, st);
  }
}

int launch_softmax_attn_bwd(const SoftmaxAttnArgs& a, hipStream_t st) {
  unsigned grid = 0;
  if (int e = grid_of(a, "hstu_softmax_attn_bwd", &grid)) return e;
  switch (a.dtype) {
    case HSTU_DTYPE_BF16: return bwd_d<bf16_t>(a, grid, st);
    case HSTU_DTYPE_F16: return bwd_d<f16_t>(a, grid, st);
    default: return bwd_d<float>(a, grid, st);
  }
}

}  // namespace hstu
