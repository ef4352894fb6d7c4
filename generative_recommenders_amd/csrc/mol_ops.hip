// Mixture-of-Logits scores for gfx950: every (query, item) pair of a batch against a shared item table, with the
// (B, X, L) logits and the (B, X, H) hidden layer of the gating MLP living in registers and LDS only.
//
//   l[n P_X + m] = <qc[b, n, :], xc[x, m, :]> / temperature                       L = P_Q P_X
//   t            = W2 silu(W1 l + b1) + b2            (H > 0)       |  W l + b     (H == 0)
//   g            = gq[b] * gi[x] + t
//   w            = g sigmoid(g)   (glu_silu)   |  g sigmoid(layer_norm(g))   (glu_silu_ln: no affine, eps 1e-5)
//   out[b, x]    = sum_j softmax(w)_j l_j
//
// Reference semantics: research/rails/similarities/mol/similarity_fn.py:35-49 (combiner), :151-204 (gating), :363-387
// (logits, "bxnm" order) in eval mode with a shared table.
//
// A workgroup (4 waves) owns 4 queries and walks 32-item tiles; a wave owns the 4 x 8 = 32 pairs of its 8 items, so
// nothing but the weights is shared between waves.  Per tile a wave
//   1. forms the logits with MFMA straight from global memory: rows (b, n) of qc viewed as (B P_Q, D) against rows
//      (x, m) of xc viewed as (X P_X, D) -- both are plain row-major matrices and a fragment is 8 consecutive
//      elements of a row -- and scatters the 32 x 32 result tiles to its [32 pairs][L] fp32 tile in LDS through two
//      small offset tables (no division in the loop);
//   2. runs the MLP transposed, pairs as the MFMA column: hidden^T = W1 l^T per 32 hidden units, bias + SiLU on the
//      accumulator, which IS the B operand of t^T += W2 hidden^T (the accumulator's row order is matched by
//      permuting W2's columns when they are staged), so the hidden layer never leaves registers;
//   3. gates, normalises and reduces: a pair's L values sit in the two lanes n32 and n32 + 32.
// fp32 operands go through v_mfma_f32_32x32x2_f32; 16-bit operands are rounded to their dtype where an MFMA reads them
// (the logits feeding W1, the hidden layer feeding W2), everything else is fp32.  No atomics: bit-identical run to run.
//
// LDS: two offset tables (3 KiB), b1 / b2 as fp32, the waves' logit tiles, the workgroup's rows of gq and the waves' rows
// of gi in their dtype (gi is requested before the logits and lands in LDS after them), and the weights, zero-padded to L' = 32 or
// 64 columns and H' = a multiple of 32 rows.  Weights that do not fit (fp32 with L > 32 and H > 192) are staged in
// chunks of hidden units per tile.  Every word that is read has been written: the logit tiles are cleared once (the
// scatter rewrites columns < L of every pair each tile, columns >= L stay zero) and the weights are staged padded.
// Nothing outside qc / xc / gq / gi / the weights is read, nothing outside out[0, B) x [0, X) is written.
#include "capi_internal.h"
#include "hstu_common.cuh"

namespace hstu {

constexpr int kMolThreads = 256;
constexpr int kMolQB = 4;            // queries of a workgroup
constexpr int kMolXW = 8;            // items of a wave
constexpr int kMolXB = 32;           // items of a workgroup tile
constexpr int kMolRowTab = 256;      // >= 4 P_Q rounded up to 32
constexpr int kMolMaxQueries = 4 << 20;  // queries of one launch (2^20 workgroups in x: a grid of 2^32 threads is the runtime's limit)
constexpr int kMolColTab = 512;      // >= 8 P_X rounded up to 32
constexpr int kMolFixedBytes = (kMolRowTab + kMolColTab) * 4 + kMolMaxHidden * 4 + kMolMaxLogits * 4;

struct MolArgs {
  const char *qc, *xc, *gq, *gi;      // (B, P_Q, D), (X, P_X, D), (B, L), (X, L)
  const char *w1, *b1, *w2, *b2;      // H > 0: (H, L), (H), (L, H), (L);  H == 0: w1 = W (L, L), b2 = b (L)
  float* out;                         // (B, X)
  float inv_temp;
  int32_t B, X, PQ, PX, D, H, L, ln;
  int32_t hc, n_chunks;               // hidden units staged at a time
  int32_t tiles_per_wg;
};

template <typename T> HSTU_DEV typename Elem<T>::Frag mol_lds_frag(const char* row, int e0) {
  typename Elem<T>::Frag f;
  if constexpr (Elem<T>::kBytes == 2) {
    f.v = __builtin_bit_cast(typename Elem<T>::vec8, *LDS_PTR(const u32x4, row + 2 * e0));
  } else {
    const f32x4 a = *LDS_PTR(const f32x4, row + 4 * e0), b = *LDS_PTR(const f32x4, row + 4 * e0 + 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  }
  return f;
}

// 8 consecutive elements of a global row, or zeros
template <typename T> HSTU_DEV typename Elem<T>::Frag mol_global_frag(const char* p, bool ok) {
  typename Elem<T>::Frag f;
  if constexpr (Elem<T>::kBytes == 2) {
    u32x4 x = {0, 0, 0, 0};
    if (ok) x = gload16(p);
    f.v = __builtin_bit_cast(typename Elem<T>::vec8, x);
  } else {
    u32x4 x0 = {0, 0, 0, 0}, x1 = {0, 0, 0, 0};
    if (ok) { x0 = gload16(p); x1 = gload16(p + 16); }
    const f32x4 a = __builtin_bit_cast(f32x4, x0), b = __builtin_bit_cast(f32x4, x1);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  }
  return f;
}

// 4 consecutive elements of an LDS row as fp32
template <typename T> HSTU_DEV f32x4 mol_lds4(const char* p) {
  if constexpr (Elem<T>::kBytes == 2) {
    typedef T vec4 __attribute__((ext_vector_type(4)));
    const vec4 v = __builtin_bit_cast(vec4, *LDS_PTR(const u32x2, p));
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  } else {
    return *LDS_PTR(const f32x4, p);
  }
}

// accumulator register r of a 32x32 MFMA holds row (r & 3) + 8 (r >> 2) + 4 hf: four consecutive rows per r >> 2
HSTU_DEV int mol_row4(int q, int hf) { return 8 * q + 4 * hf; }

template <typename T, int LT>
__global__ __launch_bounds__(kMolThreads) void hstu_mol_scores_kernel(const MolArgs p) {
  typedef typename Elem<T>::Frag Frag;
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  constexpr int ES = Elem<T>::kBytes;
  constexpr int LP = 32 * LT;                 // padded L
  constexpr int LDL = LP * 4 + 16;            // bytes of a logit row (fp32) ...
  constexpr int LD1 = LP * ES + 16;           // ... and of a W1 row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* rowtab = smem;
  char* coltab = rowtab + kMolRowTab * 4;
  char* b1s = coltab + kMolColTab * 4;
  char* b2s = b1s + kMolMaxHidden * 4;
  char* lg_all = b2s + kMolMaxLogits * 4;
  char* gqs = lg_all + 4 * 32 * LDL;          // [4 queries][LP] in T, zero-padded: the workgroup's rows of gq
  char* gis_all = gqs + kMolQB * LP * ES;     // per wave [8 items][LP] in T: the tile's rows of gi
  char* w1s = gis_all + 4 * kMolXW * LP * ES;
  const int rows1 = p.H > 0 ? p.hc : LP;
  char* w2s = w1s + rows1 * LD1;
  const int ld2 = p.hc * ES + 16;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n32 = lane & 31, hf = lane >> 5;
  char* lg = lg_all + wave * 32 * LDL;
  char* gis = gis_all + wave * kMolXW * LP * ES;
  const int R = kMolQB * p.PQ, C = kMolXW * p.PX;
  const int RT = (R + 31) >> 5, CT = (C + 31) >> 5;
  const int64_t b0 = (int64_t)blockIdx.x * kMolQB;
  const int hp = (p.H + 31) & ~31;

  // byte offset of (pair, logit) in a wave's tile = rowtab[(b, n)] + coltab[(x, m)]; pair = 8 b + x
  for (int i = tid; i < kMolRowTab; i += kMolThreads) {
    int v = -1;
    if (i < R) { const int bq = i / p.PQ, n = i - bq * p.PQ; v = bq * kMolXW * LDL + n * p.PX * 4; }
    *LDS_PTR(int, rowtab + 4 * i) = v;
  }
  for (int i = tid; i < kMolColTab; i += kMolThreads) {
    int v = -1;
    if (i < C) { const int xi = i / p.PX, m = i - xi * p.PX; v = xi * LDL + m * 4; }
    *LDS_PTR(int, coltab + 4 * i) = v;
  }
  for (int i = tid; i < kMolMaxHidden; i += kMolThreads)
    *LDS_PTR(float, b1s + 4 * i) = i < p.H ? to_f32(GLOBAL_PTR(const T, p.b1)[i]) : 0.f;
  for (int i = tid; i < kMolMaxLogits; i += kMolThreads)
    *LDS_PTR(float, b2s + 4 * i) = i < p.L ? to_f32(GLOBAL_PTR(const T, p.b2)[i]) : 0.f;
  for (int i = lane; i < 32 * LDL / 16; i += 64) *LDS_PTR(u32x4, lg + 16 * i) = u32x4{0, 0, 0, 0};
  for (int i = tid; i < kMolQB * LP; i += kMolThreads) {
    const int64_t b = b0 + i / LP;
    const int l = i % LP;
    *LDS_PTR(T, gqs + ES * i) = (b < p.B && l < p.L) ? GLOBAL_PTR(const T, p.gq)[b * p.L + l] : (T)0.f;
  }

  // weights of hidden units [c hc, (c + 1) hc), zero-padded; W2's columns permuted inside every 16 (bits 2 and 3 of
  // the unit swapped) so that slot (hf, j) of an A fragment is the unit accumulator register j of GEMM 1 holds
  auto stage_weights = [&](int c) {
    const T zero = (T)0.f;
    if (p.H > 0) {
      const int h0 = c * p.hc;
      for (int i = tid; i < p.hc * LP; i += kMolThreads) {
        const int hl = i / LP, l = i % LP, h = h0 + hl;
        T v = zero;
        if (h < p.H && l < p.L) v = GLOBAL_PTR(const T, p.w1)[(int64_t)h * p.L + l];
        *LDS_PTR(T, w1s + hl * LD1 + l * ES) = v;
      }
      for (int l = tid >> 5; l < LP; l += kMolThreads / 32) {
        for (int hl = tid & 31; hl < p.hc; hl += 32) {
          const int h = h0 + hl, pos = (hl & ~12) | ((hl & 4) << 1) | ((hl & 8) >> 1);
          T v = zero;
          if (h < p.H && l < p.L) v = GLOBAL_PTR(const T, p.w2)[(int64_t)l * p.H + h];
          *LDS_PTR(T, w2s + l * ld2 + pos * ES) = v;
        }
      }
    } else {
      for (int i = tid; i < LP * LP; i += kMolThreads) {
        const int lo = i / LP, li = i % LP;
        T v = zero;
        if (lo < p.L && li < p.L) v = GLOBAL_PTR(const T, p.w1)[(int64_t)lo * p.L + li];
        *LDS_PTR(T, w1s + lo * LD1 + li * ES) = v;
      }
    }
  };
  if (p.n_chunks == 1) stage_weights(0);
  __syncthreads();

  const int64_t n_tiles = ((int64_t)p.X + kMolXB - 1) / kMolXB;
  const int64_t t_begin = (int64_t)blockIdx.y * p.tiles_per_wg;
  const int64_t t_end = min(t_begin + (int64_t)p.tiles_per_wg, n_tiles);
  const int64_t q_rows = (int64_t)p.B * p.PQ, x_rows = (int64_t)p.X * p.PX;

  for (int64_t t = t_begin; t < t_end; ++t) {
    const int64_t x0 = t * kMolXB + wave * kMolXW;

    // the tile's rows of gi: requested now, written to LDS after the logits (unconditional loads: an element outside
    // the problem reads gi[0] and is replaced by zero)
    T giv[4 * LT];
#pragma unroll
    for (int j = 0; j < 4 * LT; ++j) {
      const int i = lane + 64 * j, l = i % LP;
      const int64_t x = x0 + i / LP;
      const bool ok = x < p.X && l < p.L;
      const T v = GLOBAL_PTR(const T, p.gi)[ok ? x * p.L + l : 0];
      giv[j] = ok ? v : (T)0.f;
    }

    // ---- 1. logits -> lg[pair][l]
    for (int ct = 0; ct < CT; ++ct) {
      const int col = 32 * ct + n32;
      const int64_t gcol = x0 * p.PX + col;
      const bool col_ok = col < C && gcol < x_rows;
      const char* xrow = p.xc + gcol * p.D * ES;
      const int coff = *LDS_PTR(const int, coltab + 4 * col);
      for (int rt = 0; rt < RT; ++rt) {
        const int row = 32 * rt + n32;
        const int64_t grow = b0 * p.PQ + row;
        const bool row_ok = row < R && grow < q_rows;
        const char* qrow = p.qc + grow * p.D * ES;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < p.D; k0 += 64) {           // four chunks of 16 requested together
          Frag af[4], bf[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int kk = k0 + 16 * j + 8 * hf;
            af[j] = mol_global_frag<T>(qrow + kk * ES, row_ok && kk < p.D);
            bf[j] = mol_global_frag<T>(xrow + kk * ES, col_ok && kk < p.D);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (k0 + 16 * j < p.D) acc = Elem<T>::mma(af[j], bf[j], acc);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const i32x4 ro = *LDS_PTR(const i32x4, rowtab + 4 * (32 * rt + mol_row4(q, hf)));
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (ro[i] >= 0 && coff >= 0) *LDS_PTR(float, lg + ro[i] + coff) = acc[4 * q + i] * p.inv_temp;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4 * LT; ++j) *LDS_PTR(T, gis + ES * (lane + 64 * j)) = giv[j];
    __syncthreads();

    // ---- 2. t^T = W2 silu(W1 l^T + b1) + b2, pairs as columns
    Frag lb[2 * LT];
#pragma unroll
    for (int ks = 0; ks < 2 * LT; ++ks) {
      float v[8];
      const f32x4 a = *LDS_PTR(const f32x4, lg + n32 * LDL + 4 * (16 * ks + 8 * hf));
      const f32x4 b = *LDS_PTR(const f32x4, lg + n32 * LDL + 4 * (16 * ks + 8 * hf) + 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
      lb[ks] = Elem<T>::pack8(v);
    }
    f32x16 tacc[LT];
#pragma unroll
    for (int lt = 0; lt < LT; ++lt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 bb = *LDS_PTR(const f32x4, b2s + 4 * (32 * lt + mol_row4(q, hf)));
#pragma unroll
        for (int i = 0; i < 4; ++i) tacc[lt][4 * q + i] = bb[i];
      }

    if (p.H > 0) {
      for (int c = 0; c < p.n_chunks; ++c) {
        if (p.n_chunks > 1) {
          __syncthreads();
          stage_weights(c);
          __syncthreads();
        }
        const int h0 = c * p.hc, hn = min(p.hc, hp - h0);
        for (int hb = 0; hb < hn; hb += 32) {
          f32x16 acc;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 bb = *LDS_PTR(const f32x4, b1s + 4 * (h0 + hb + mol_row4(q, hf)));
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[4 * q + i] = bb[i];
          }
#pragma unroll
          for (int ks = 0; ks < 2 * LT; ++ks)
            if (16 * ks < p.L) acc = Elem<T>::mma(mol_lds_frag<T>(w1s + (hb + n32) * LD1, 16 * ks + 8 * hf), lb[ks], acc);
          float hv[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) hv[r] = acc[r] * fast_sigmoid(acc[r]);
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            const Frag hfrag = Elem<T>::pack8(hv + 8 * f);
#pragma unroll
            for (int lt = 0; lt < LT; ++lt)
              tacc[lt] = Elem<T>::mma(mol_lds_frag<T>(w2s + (32 * lt + n32) * ld2, hb + 16 * f + 8 * hf), hfrag, tacc[lt]);
          }
        }
      }
    } else {
#pragma unroll
      for (int lt = 0; lt < LT; ++lt)
#pragma unroll
        for (int ks = 0; ks < 2 * LT; ++ks)
          if (16 * ks < p.L)
            tacc[lt] = Elem<T>::mma(mol_lds_frag<T>(w1s + (32 * lt + n32) * LD1, 16 * ks + 8 * hf), lb[ks], tacc[lt]);
    }

    // ---- 3. gate, softmax, weighted sum: lane (n32, hf) holds logits 32 lt + 8 q + 4 hf + i of pair n32
    const int64_t b = b0 + (n32 >> 3), x = x0 + (n32 & 7);
    const bool pair_ok = b < p.B && x < p.X;
    const char* gq_row = gqs + (n32 >> 3) * LP * ES;
    const char* gi_row = gis + (n32 & 7) * LP * ES;
    float g[16 * LT], lv[16 * LT];
    float sum = 0.f;
#pragma unroll
    for (int lt = 0; lt < LT; ++lt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int l0 = 32 * lt + mol_row4(q, hf);
        const f32x4 lq = *LDS_PTR(const f32x4, lg + n32 * LDL + 4 * l0);
        const f32x4 gqv = mol_lds4<T>(gq_row + ES * l0), gxv = mol_lds4<T>(gi_row + ES * l0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = 16 * lt + 4 * q + i;
          lv[e] = lq[i];
          g[e] = l0 + i < p.L ? gqv[i] * gxv[i] + tacc[lt][4 * q + i] : 0.f;
          sum += g[e];
        }
      }
    float mean = 0.f, rstd = 1.f;
    if (p.ln) {
      sum += __shfl_xor(sum, 32, 64);
      mean = sum / (float)p.L;
      float var = 0.f;
#pragma unroll
      for (int lt = 0; lt < LT; ++lt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int l = 32 * lt + (r & 3) + mol_row4(r >> 2, hf);
          const float d = g[16 * lt + r] - mean;
          var += l < p.L ? d * d : 0.f;
        }
      var += __shfl_xor(var, 32, 64);
      rstd = 1.0f / sqrtf(var / (float)p.L + 1e-5f);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int lt = 0; lt < LT; ++lt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int l = 32 * lt + (r & 3) + mol_row4(r >> 2, hf), e = 16 * lt + r;
        const float arg = p.ln ? (g[e] - mean) * rstd : g[e];
        g[e] = l < p.L ? g[e] * fast_sigmoid(arg) : -INFINITY;
        mx = fmaxf(mx, g[e]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float den = 0.f, num = 0.f;
#pragma unroll
    for (int e = 0; e < 16 * LT; ++e) {
      const float pe = __builtin_amdgcn_exp2f((g[e] - mx) * 1.44269504088896340736f);   // exp2(-inf) = 0: padding
      den += pe;
      num += pe * lv[e];
    }
    den += __shfl_xor(den, 32, 64);
    num += __shfl_xor(num, 32, 64);
    if (pair_ok && hf == 0) p.out[b * p.X + x] = num / den;
  }
}

// hidden units staged at a time: all of them when the weights fit next to the logit tiles, else the largest multiple of 32
static int mol_chunk(int lp, int hp, int es, int* smem) {
  const int fixed = kMolFixedBytes + 4 * 32 * (lp * 4 + 16) + (kMolQB + 4 * kMolXW) * lp * es;
  if (hp == 0) {
    *smem = fixed + lp * (lp * es + 16);
    return 0;
  }
  int hc = hp;
  for (; hc > 32; hc -= 32)
    if (fixed + hc * (lp * es + 16) + lp * (hc * es + 16) <= kLdsBudget) break;
  *smem = fixed + hc * (lp * es + 16) + lp * (hc * es + 16);
  return hc;
}

template <typename T, int LT>
static int launch_mol_t(MolArgs a, hipStream_t st) {
  auto kern = hstu_mol_scores_kernel<T, LT>;
  int smem = 0;
  const int hp = (a.H + 31) & ~31;
  a.hc = mol_chunk(32 * LT, hp, Elem<T>::kBytes, &smem);
  a.n_chunks = a.hc > 0 ? (hp + a.hc - 1) / a.hc : 1;
  if (smem > kLdsBudget) return set_error(HSTU_EUNSUPPORTED, "hstu_mol_scores: %d bytes of LDS exceed the budget", smem);
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  if (e != hipSuccess) return set_error(HSTU_ELAUNCH, "hstu_mol_scores: cannot reserve %d bytes of LDS: %s", smem, hipGetErrorString(e));
  // larger batches: one launch per kMolMaxQueries queries (the operands of a query are rows of qc, gq and out)
  const int64_t batch = a.B, n_tiles = ((int64_t)a.X + kMolXB - 1) / kMolXB;
  const int es = Elem<T>::kBytes;
  for (int64_t q0 = 0; q0 < batch; q0 += kMolMaxQueries) {
    MolArgs c = a;
    c.B = (int32_t)(batch - q0 < kMolMaxQueries ? batch - q0 : kMolMaxQueries);
    c.qc = a.qc + q0 * a.PQ * a.D * es;
    c.gq = a.gq + q0 * a.L * es;
    c.out = a.out + q0 * a.X;
    const int64_t q_groups = ((int64_t)c.B + kMolQB - 1) / kMolQB;
    // item ranges: about eight workgroups per CU in all, so that a workgroup amortises staging the weights
    int64_t splits = 8 * (int64_t)cu_count() / q_groups;
    splits = splits < 1 ? 1 : (splits > n_tiles ? n_tiles : splits);
    if (splits > 65535) splits = 65535;
    const int64_t per = (n_tiles + splits - 1) / splits;
    splits = (n_tiles + per - 1) / per;
    c.tiles_per_wg = (int32_t)per;
    hipLaunchKernelGGL(kern, dim3((unsigned)q_groups, (unsigned)splits), dim3(kMolThreads), smem, st, c);
    if (int err = check_launch("hstu_mol_scores")) return err;
  }
  return HSTU_OK;
}

int launch_mol_scores(const void* qc, const void* xc, const void* gq, const void* gi, const void* w1, const void* b1, const void* w2,
                      const void* b2, float* out, int batch, int num_items, int pq, int px, int dim, int hidden, float inv_temperature,
                      int layer_norm, int dtype, hipStream_t st) {
  MolArgs a;
  a.qc = (const char*)qc; a.xc = (const char*)xc; a.gq = (const char*)gq; a.gi = (const char*)gi;
  a.w1 = (const char*)w1; a.b1 = (const char*)b1; a.w2 = (const char*)w2; a.b2 = (const char*)b2;
  a.out = out; a.inv_temp = inv_temperature;
  a.B = batch; a.X = num_items; a.PQ = pq; a.PX = px; a.D = dim; a.H = hidden; a.L = pq * px; a.ln = layer_norm;
  a.hc = 0; a.n_chunks = 1; a.tiles_per_wg = 1;
  const bool wide = a.L > 32;
  switch (dtype) {
    case HSTU_DTYPE_BF16: return wide ? launch_mol_t<bf16_t, 2>(a, st) : launch_mol_t<bf16_t, 1>(a, st);
    case HSTU_DTYPE_F16: return wide ? launch_mol_t<f16_t, 2>(a, st) : launch_mol_t<f16_t, 1>(a, st);
    default: return wide ? launch_mol_t<float, 2>(a, st) : launch_mol_t<float, 1>(a, st);
  }
}

}  // namespace hstu
