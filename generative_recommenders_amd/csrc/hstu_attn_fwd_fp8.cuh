// fp8 (OCP e4m3fn) HSTU attention forward for gfx950: q / k / v read as e4m3 from HBM, bf16 output.
//
//   O[i,:] = sum_j silu(alpha qd kd <q_i,k_j>) * scale * M[i,j] * vd * v_j        (per user b, head h; qd = q_descale[b,h], ...)
//
// The e4m3 forward of hstu::hstu_mha_fwd (ops/cpp/hstu_attention/flash_common.cpp:222-305, 448-536: (B, H) fp32 descales,
// bf16 output).  Unlike the reference's kernels, which load the descales and never use them, the descales are APPLIED:
// alpha qd kd is the score multiplier of the (user, head), scale vd multiplies the fp32 accumulator before the bf16 store.
//
// Same mapping and schedule as the 16-bit forward (hstu_attn_fwd.cuh: one workgroup = (user, head, 128 query rows), the query
// index on the lane axis, S^T = K Q^T and O^T += V^T P^T on 32x32x16 MFMAs, K/V tiles of 32 keys through an LDS ring), except:
//  * S^T = K Q^T runs on the e4m3 MFMA (v_mfma_f32_32x32x16_fp8_fp8: the bf16 rate, fp32 accumulation of exact products):
//    K stays e4m3 in LDS, Q stays e4m3 in registers (8 bytes per fragment).  As for the 16-bit MFMA, slot (hf, j) of A is
//    paired with slot (hf, j) of B, so both operands only have to agree on which element a slot carries.
//  * V is widened exactly to bf16 (every e4m3 value is a bf16 value) on its way into LDS, and O^T += V^T P^T is the bf16
//    kernel's: P is rounded to bf16 as on the bf16 path (the reference's Hopper kernel rounds P to e4m3 instead).
//  * The K/V tiles come through REGISTERS, a step ahead: every thread loads one 16-byte unit (16 e4m3 values) of the K and of
//    the V tile.
// Bytes from HBM: 1 per q / k / v element, 2 per output element.
#pragma once
#include "hstu_attn_fwd.cuh"

namespace hstu {

template <int D>
struct Fp8FwdCfg {
  static constexpr int UPR8 = D / 16;                  // 16-byte units of an e4m3 row (global memory)
  static constexpr int UPR = D * 2 / 16;               // 16-byte units of a bf16 row (LDS)
  static constexpr int NU = (32 * UPR8 + kFwdThreads - 1) / kFwdThreads;   // staged units per thread and tensor
  static constexpr int KT = 32 * D;                    // bytes of a 32-row e4m3 K tile
  static constexpr int VT = 32 * D * 2;                // bytes of a 32-row V tile widened to bf16
  static constexpr int STAGE = KT + VT;
  static constexpr int NS = 2;                         // tile t computed while tile t+1 waits in registers
  static constexpr int SMEM = NS * STAGE > 4 * VT ? NS * STAGE : 4 * VT;   // (the epilogue parks one [32][D] bf16 tile per wave)
  static constexpr int KG = D / 16;                    // 16-wide contraction groups of QK^T
  static constexpr int DB = D / 32;                    // 32-wide output blocks
};

// 16 e4m3 values -> 16 bf16 values (two 16-byte units), exact; element order is kept (bytes 0,1 / 2,3 of word w are
// elements 4w, 4w+1 / 4w+2, 4w+3)
HSTU_DEV void fp8x16_to_bf16(const u32x4 x, u32x4& lo, u32x4& hi) {
  uint32_t o[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    o[2 * w] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)x[w], 1.0f, false));
    o[2 * w + 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)x[w], 1.0f, true));
  }
  lo = u32x4{o[0], o[1], o[2], o[3]};
  hi = u32x4{o[4], o[5], o[6], o[7]};
}

// Cooperative global -> register load of one [32][D] e4m3 tile: unconditional loads on clamped (valid) addresses, so the
// registers are not consumed before fp8_tile_lds_write (see tile_gload).  Zero fill happens at write time.
template <int D>
HSTU_DEV void fp8_tile_gload(u32x4 (&reg)[Fp8FwdCfg<D>::NU], const char* base, int64_t row_stride_bytes, int row0, int len,
                             int real_d, int tid) {
  constexpr int UPR8 = Fp8FwdCfg<D>::UPR8;
#pragma unroll
  for (int t = 0; t < Fp8FwdCfg<D>::NU; ++t) {
    const int u = min(tid + t * kFwdThreads, 32 * UPR8 - 1);
    const int row = min(row0 + u / UPR8, len - 1);
    const int unit = ((u % UPR8) * 16 < real_d) ? (u % UPR8) : 0;
    reg[t] = gload16(base + (int64_t)row * row_stride_bytes + unit * 16);
  }
}

// ... and register -> LDS: K as it is (e4m3 rows, swizzled 16-byte units), rows past `len` and columns past the real head dim
// as zeros
template <int D>
HSTU_DEV void fp8_tile_lds_write_raw(const u32x4 (&reg)[Fp8FwdCfg<D>::NU], char* tile, int row0, int len, int real_d, int tid) {
  constexpr int UPR8 = Fp8FwdCfg<D>::UPR8;
#pragma unroll
  for (int t = 0; t < Fp8FwdCfg<D>::NU; ++t) {
    const int u = tid + t * kFwdThreads;
    if (u < 32 * UPR8) {
      const int row = u / UPR8, unit = u % UPR8;
      const bool ok = (row0 + row < len) & (unit * 16 < real_d);
      const u32x4 z = {0u, 0u, 0u, 0u};
      *LDS_PTR(u32x4, tile + tile_off<UPR8>(row, unit)) = ok ? reg[t] : z;
    }
  }
}

// ... V widened to bf16, into the swizzled row-major layout the 16-bit fragment readers expect
template <int D>
HSTU_DEV void fp8_tile_lds_write(const u32x4 (&reg)[Fp8FwdCfg<D>::NU], char* tile, int row0, int len, int real_d, int tid) {
  constexpr int UPR8 = Fp8FwdCfg<D>::UPR8, UPR = Fp8FwdCfg<D>::UPR;
#pragma unroll
  for (int t = 0; t < Fp8FwdCfg<D>::NU; ++t) {
    const int u = tid + t * kFwdThreads;
    if (u < 32 * UPR8) {
      const int row = u / UPR8, unit = u % UPR8;
      const bool ok = (row0 + row < len) & (unit * 16 < real_d);
      const u32x4 z = {0u, 0u, 0u, 0u};
      u32x4 lo, hi;
      fp8x16_to_bf16(ok ? reg[t] : z, lo, hi);
      *LDS_PTR(u32x4, tile + tile_off<UPR>(row, 2 * unit)) = lo;
      *LDS_PTR(u32x4, tile + tile_off<UPR>(row, 2 * unit + 1)) = hi;
    }
  }
}

HSTU_DEV float fp8_descale_at(const float* d, int64_t sb, int64_t sh, int b, int h) {
  return d ? *GLOBAL_PTR(const float, d + (int64_t)b * sb + (int64_t)h * sh) : 1.0f;
}

template <int D>
__global__ __launch_bounds__(kFwdThreads, HSTU_FWD_MIN_WAVES) void hstu_attn_fwd_fp8_kernel(const HstuAttnParams p, const HstuFp8Descale ds,
                                                                                          int nqb) {
  using C = Fp8FwdCfg<D>;
  using E = Elem<bf16_t>;
  using Frag = E::Frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n32 = lane & 31, hf = lane >> 5;

  // ---- work decode: as the 16-bit forward (8 (user, head) pairs per dispatch group, heavier query blocks first)
  const int bid = blockIdx.x;
  const int grp = bid / (8 * nqb), rem = bid % (8 * nqb);
  const int qb = nqb - 1 - rem / 8;
  const int uh = grp * 8 + (rem & 7);
  if (uh >= p.batch * p.heads) return;
  const int b = user_of_slot(p, uh / p.heads), hd = uh % p.heads;

  const int64_t off0 = load_index(p.seq_offsets, b, p.offsets_dtype);
  const int len = (int)(load_index(p.seq_offsets, b + 1, p.offsets_dtype) - off0);
  const int nq_rows = p.delta_q > 0 ? min(p.delta_q, len) : len;
  const int i_shift = p.delta_q > 0 ? len - nq_rows : 0;
  const int64_t q_base = p.delta_q > 0 ? (int64_t)b * p.delta_q + (p.delta_q - nq_rows) : off0;
  const int q0 = qb * kFwdRowsPerBlock;
  if (q0 >= nq_rows) return;

  const MaskCtx mc = make_mask_ctx(p, b, len);
  // the descales of this (user, head): alpha qd kd multiplies S, scale vd the accumulator
  const float alpha = p.alpha * fp8_descale_at(ds.q, ds.q_batch_stride, ds.q_head_stride, b, hd) *
                      fp8_descale_at(ds.k, ds.k_batch_stride, ds.k_head_stride, b, hd);
  const float out_mul = attn_scale_of(p) * fp8_descale_at(ds.v, ds.v_batch_stride, ds.v_head_stride, b, hd);

  const int na_blk = (min(kFwdRowsPerBlock, nq_rows - q0) + 31) >> 5;
  const int vw = ((qb & 1) && wave < na_blk) ? na_blk - 1 - wave : wave;
  const int r0 = q0 + 32 * vw;
  const bool wave_active = r0 < nq_rows;
  const int my_row = r0 + n32;
  const bool row_ok = my_row < nq_rows;
  const int qi = my_row + i_shift;
  const int qi_id = mc.id_of(qi);

  const int i_first = q0 + i_shift;
  const int i_last = min(q0 + kFwdRowsPerBlock, nq_rows) - 1 + i_shift;
  const bool ctx_rows = mc.ctx > 0 && i_first < mc.ctx;
  const int kv_hi = ctx_rows ? len : min(len, i_last + 1);
  int kv_lo = 0;
  if (mc.win > 0 && mc.full == 0 && !ctx_rows) {
    const int x = mc.id_of(i_first) - mc.win;
    const int pos = x <= 0 ? 0 : (mc.ctx > 0 ? x + mc.ctx - 1 : x);
    kv_lo = (pos >> 5) << 5;
  }
  const int ntiles = (kv_hi - kv_lo + 31) >> 5;

  // ---- Q fragment (B operand of S^T = K Q^T, e4m3): lane (n32, hf) holds elements hf D/2 + 8 kg .. +8 of its row, i.e. D/32
  // 16-byte units of one half row; fragment kg is half kg % 2 of unit kg / 2
  u32x4 qraw[C::KG / 2];
  {
    const int ld_row = min(my_row, nq_rows - 1);
    const char* qrow = (const char*)p.q + (q_base + ld_row) * p.q_row_stride + (int64_t)hd * p.q_head_stride;
#pragma unroll
    for (int i = 0; i < C::KG / 2; ++i) {
      const int e0 = hf * (D / 2) + 16 * i;
      qraw[i] = gload16(qrow + (e0 < p.dqk ? e0 : 0));
    }
#pragma unroll
    for (int i = 0; i < C::KG / 2; ++i) {
      const int e0 = hf * (D / 2) + 16 * i;
      const u32x4 z = {0u, 0u, 0u, 0u};
      qraw[i] = (row_ok && e0 < p.dqk) ? qraw[i] : z;
    }
  }
  const char* kbase = (const char*)p.k + off0 * p.k_row_stride + (int64_t)hd * p.k_head_stride;
  const char* vbase = (const char*)p.v + off0 * p.v_row_stride + (int64_t)hd * p.v_head_stride;

  f32x16 oacc[C::DB];
#pragma unroll
  for (int d = 0; d < C::DB; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;

  const float aabs = fabsf(alpha);
  const bool wave_plain = mc.simple || (mc.has_targets && mc.win == 0 && mc.ctx == 0 && i_shift == 0 && r0 + 32 <= min(len, mc.max_id));
  const bool diag_fast = wave_plain && i_shift == 0 && kv_lo == 0 && aabs > 1e-20f && aabs < 1e6f;

  // ---- K/V: tile 0 converted into slot 0, tile 1 in registers
  u32x4 kreg[C::NU], vreg[C::NU];
  if (ntiles > 0) {
    fp8_tile_gload<D>(kreg, kbase, p.k_row_stride, kv_lo, len, p.dqk, tid);
    fp8_tile_gload<D>(vreg, vbase, p.v_row_stride, kv_lo, len, p.dv, tid);
    fp8_tile_lds_write_raw<D>(kreg, smem, kv_lo, len, p.dqk, tid);
    fp8_tile_lds_write<D>(vreg, smem + C::KT, kv_lo, len, p.dv, tid);
    if (ntiles > 1) {
      fp8_tile_gload<D>(kreg, kbase, p.k_row_stride, kv_lo + 32, len, p.dqk, tid);
      fp8_tile_gload<D>(vreg, vbase, p.v_row_stride, kv_lo + 32, len, p.dv, tid);
    }
  }

  for (int t = 0; t < ntiles; ++t) {
    const int slot = t & 1;
    const int j0 = kv_lo + (t << 5);
    __syncthreads();   // tile t is in slot t % 2 for every wave; every wave is done with tile t - 1 (slot (t + 1) % 2 is free)
    const int i0w = r0 + i_shift;
    bool tile_act, tile_full;
    if (wave_plain) {
      tile_act = i0w < len && j0 <= min(i0w + 31, len - 1);
      tile_full = j0 + 32 <= i0w;
    } else {
      tile_act = mc.pair_may_be_active(i0w, 32, j0, 32);
      tile_full = tile_act && mc.pair_fully_valid(i0w, 32, j0, 32);
    }
    if (wave_active && tile_act) {
      const char* Kt = smem + slot * C::STAGE;
      const char* Vt = Kt + C::KT;
      // mode (wave-uniform), as in the 16-bit forward: 0 no mask, 1 plain causal by compares, 2 general mask algebra, 3 targets /
      // window by integer arithmetic, 4 plain causal with tile-aligned rows (the diagonal tile's mask put into S itself)
      const int mode = tile_full ? 0 : (wave_plain ? (diag_fast ? 4 : 1) : (mc.ctx == 0 ? 3 : 2));
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int kg = 0; kg < C::KG; ++kg) {
        const int e0 = hf * (D / 2) + kg * 8;
        const u32x2 a = *LDS_PTR(const u32x2, Kt + tile_off<C::UPR8>(n32, e0 >> 4) + (e0 & 15));
        const u32x4& qu = qraw[kg >> 1];
        const u32x2 b = (kg & 1) ? u32x2{qu[2], qu[3]} : u32x2{qu[0], qu[1]};
        s = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(__builtin_bit_cast(long, a), __builtin_bit_cast(long, b), s, 0, 0, 0);
      }
      if (mode == 4) {
        const float neg = alpha < 0.f ? 1e30f : -1e30f;
        const int x = n32 - 4 * hf;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = ((r & 3) + 8 * (r >> 2) > x) ? neg : s[r];
      }
      Frag pb[2];
#pragma unroll
      for (int h8 = 0; h8 < 2; ++h8) {
        float pv[8];
        const f32x2 a2 = {alpha, alpha};
        const f32x2 c2 = {-1.44269504088896340736f * alpha, -1.44269504088896340736f * alpha};
        const f32x2 one2 = {1.f, 1.f};
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const f32x2 sv = {s[8 * h8 + j], s[8 * h8 + j + 1]};
          const f32x2 x = sv * a2, tt = sv * c2;
          const f32x2 e = {__builtin_amdgcn_exp2f(tt[0]), __builtin_amdgcn_exp2f(tt[1])};
          const f32x2 dn = e + one2;
          const f32x2 sg = {__builtin_amdgcn_rcpf(dn[0]), __builtin_amdgcn_rcpf(dn[1])};
          const f32x2 pr = x * sg;
          pv[j] = pr[0];
          pv[j + 1] = pr[1];
        }
        if (mode == 1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int r = 8 * h8 + j;
            const int key = j0 + (r & 3) + 8 * (r >> 2) + 4 * hf;
            pv[j] = (row_ok & (key < len) & (key <= qi)) ? pv[j] : 0.f;
          }
        } else if (mode == 2) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int r = 8 * h8 + j;
            const int key = j0 + (r & 3) + 8 * (r >> 2) + 4 * hf;
            const bool ok = row_ok & (key < len) & mc.valid_ids(qi, key, qi_id, mc.id_of(key));
            pv[j] = ok ? pv[j] : 0.f;
          }
        } else if (mode == 3) {
          const int i_eff = row_ok ? qi : -1;
          const int idi = mc.has_targets ? min(i_eff, mc.max_id) : i_eff;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int r = 8 * h8 + j;
            const int key = j0 + (r & 3) + 8 * (r >> 2) + 4 * hf;
            const int idj = mc.has_targets ? min(key, mc.max_id) : key;
            const int keep = mc.keep_bits_row(i_eff, idi, key, idj) & ((key - len) >> 31);
            pv[j] = __builtin_bit_cast(float, __builtin_bit_cast(int, pv[j]) & keep);
          }
        }
        pb[h8] = E::pack8(pv);
      }
#pragma unroll
      for (int d = 0; d < C::DB; ++d) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          Frag a = lds_col_frag<bf16_t, C::UPR>(Vt, 16 * ks + 4 * hf, 16 * ks + 8 + 4 * hf, 32 * d, lane);
          oacc[d] = E::mma(a, pb[ks], oacc[d]);
        }
      }
    }
    // tile t + 1 (in registers since step t - 1) -> the free slot; tile t + 2 requested
    if (t + 1 < ntiles) {
      char* st = smem + (slot ^ 1) * C::STAGE;
      fp8_tile_lds_write_raw<D>(kreg, st, j0 + 32, len, p.dqk, tid);
      fp8_tile_lds_write<D>(vreg, st + C::KT, j0 + 32, len, p.dv, tid);
      if (t + 2 < ntiles) {
        fp8_tile_gload<D>(kreg, kbase, p.k_row_stride, j0 + 64, len, p.dqk, tid);
        fp8_tile_gload<D>(vreg, vbase, p.v_row_stride, j0 + 64, len, p.dv, tid);
      }
    }
  }

  // ---- epilogue: O^T accumulators x scale vd -> bf16 rows.  Full-width heads through LDS (each wave parks its [32][D] tile in
  // the dead ring and stores whole 16-byte units), narrower real heads lane by lane
  if (p.dv == D) {
    __syncthreads();   // every wave is done with the ring
    char* tile = smem + wave * C::VT;
    if (wave_active) {
#pragma unroll
      for (int d = 0; d < C::DB; ++d)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          u32x2 v = {E::pk2(oacc[d][4 * rq] * out_mul, oacc[d][4 * rq + 1] * out_mul),
                     E::pk2(oacc[d][4 * rq + 2] * out_mul, oacc[d][4 * rq + 3] * out_mul)};
          *LDS_PTR(u32x2, tile + tile_off<C::UPR>(n32, 4 * d + rq) + 8 * hf) = v;
        }
      char* obase = (char*)p.out + ((q_base + r0) * p.o_row_stride + (int64_t)hd * p.o_head_stride) * 2;
      const int rows_valid = nq_rows - r0;
#pragma unroll
      for (int i = 0; i < 32 * C::UPR / 64; ++i) {
        const int idx = i * 64 + lane;
        const int row = idx / C::UPR, unit = idx % C::UPR;
        const u32x4 v = *LDS_PTR(const u32x4, tile + tile_off<C::UPR>(row, unit));
        if (row < rows_valid) gstore16_nt(obase + (int64_t)row * p.o_row_stride * 2 + unit * 16, v);
      }
    }
    return;
  }
  if (row_ok) {
    char* orow = (char*)p.out + ((q_base + my_row) * p.o_row_stride + (int64_t)hd * p.o_head_stride) * 2;
#pragma unroll
    for (int d = 0; d < C::DB; ++d) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int d0 = 32 * d + 8 * rq + 4 * hf;
        if (d0 < p.dv)
          store4<bf16_t>(orow, d0, oacc[d][4 * rq] * out_mul, oacc[d][4 * rq + 1] * out_mul, oacc[d][4 * rq + 2] * out_mul,
                         oacc[d][4 * rq + 3] * out_mul);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Jagged per-(user, head) e4m3 quantizer: one workgroup per (user, head), two passes over the user's rows of that head.
//   descale[b,h] = amax / 448 (1 when amax == 0),  x8 = e4m3(clamp(x / descale, -448, 448))     (IEEE division, RNE)
// ---------------------------------------------------------------------------
constexpr int kQuantThreads = 256;

template <typename T>
HSTU_DEV void load8_as_f32(const char* p, float (&f)[8]) {
  if constexpr (sizeof(T) == 2) {
    const u32x4 x = gload16(p);
    typedef T t8 __attribute__((ext_vector_type(8)));
    const t8 h = __builtin_bit_cast(t8, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)h[j];
  } else {
    const f32x4 a = __builtin_bit_cast(f32x4, gload16(p)), b = __builtin_bit_cast(f32x4, gload16(p + 16));
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[4 + j] = b[j]; }
  }
}

HSTU_DEV float fp8_quant_clamped(float x, float descale) {
  const float y = x / descale;   // (correctly rounded: hipcc's default fp32 division)
  return fminf(fmaxf(y, -448.0f), 448.0f);
}

// VEC: rows 16-byte aligned and dim a multiple of 8 (8 elements per thread and step); otherwise one element per step
template <typename T, bool VEC>
__global__ __launch_bounds__(kQuantThreads) void hstu_jagged_quantize_fp8_kernel(const char* x, int64_t x_row_stride, int64_t x_head_stride,
                                                                               uint8_t* x8, float* descale, const void* seq_offsets,
                                                                               int offsets_dtype, int heads, int dim) {
  __shared__ float red[kQuantThreads / 64];
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int64_t off0 = load_index(seq_offsets, b, offsets_dtype);
  const int64_t len = load_index(seq_offsets, b + 1, offsets_dtype) - off0;
  const int tid = threadIdx.x;
  constexpr int EB = sizeof(T);
  constexpr int STEP = VEC ? 8 : 1;
  const int upr = dim / STEP;
  const int64_t n = len * upr;
  auto src = [&](int64_t u) {
    const int64_t r = u / upr;
    const int c = (int)(u - r * upr) * STEP;
    return x + ((off0 + r) * x_row_stride + (int64_t)h * x_head_stride + c) * EB;
  };
  auto dst = [&](int64_t u) {
    const int64_t r = u / upr;
    const int c = (int)(u - r * upr) * STEP;
    return x8 + ((off0 + r) * heads + h) * (int64_t)dim + c;
  };
  // pass 1: amax
  float amax = 0.f;
  for (int64_t u = tid; u < n; u += kQuantThreads) {
    if constexpr (VEC) {
      float f[8];
      load8_as_f32<T>(src(u), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
    } else {
      amax = fmaxf(amax, fabsf((float)*(const T*)src(u)));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = amax;
  __syncthreads();
  amax = red[0];
#pragma unroll
  for (int w = 1; w < kQuantThreads / 64; ++w) amax = fmaxf(amax, red[w]);
  const float d = amax > 0.f ? amax / 448.0f : 1.0f;
  if (tid == 0) descale[(int64_t)b * heads + h] = d;
  // pass 2: scaled, clamped, rounded to e4m3 (round to nearest even)
  for (int64_t u = tid; u < n; u += kQuantThreads) {
    if constexpr (VEC) {
      float f[8];
      load8_as_f32<T>(src(u), f);
      int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_quant_clamped(f[0], d), fp8_quant_clamped(f[1], d), 0, false);
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_quant_clamped(f[2], d), fp8_quant_clamped(f[3], d), w0, true);
      int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_quant_clamped(f[4], d), fp8_quant_clamped(f[5], d), 0, false);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_quant_clamped(f[6], d), fp8_quant_clamped(f[7], d), w1, true);
      *GLOBAL_PTR(u32x2, dst(u)) = u32x2{(uint32_t)w0, (uint32_t)w1};
    } else {
      const float y = fp8_quant_clamped((float)*(const T*)src(u), d);
      *dst(u) = (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(y, 0.f, 0, false) & 0xff);
    }
  }
}

}  // namespace hstu
