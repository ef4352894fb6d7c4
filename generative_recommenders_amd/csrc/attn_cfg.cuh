// Sizes of the attention kernels' configurations: workgroup shapes and LDS layouts as functions of the element size and
// the (padded) head dims.  The kernels (hstu_attn_*.cuh) and the host-side dispatch plan (attn_misc.hip) both read them
// here; nothing else restates them.
#pragma once
#include "hstu_common.cuh"

namespace hstu {

// ---- forward (hstu_attn_fwd.cuh) ----
constexpr int kFwdThreads = 256;
constexpr int kFwdRowsPerBlock = 128;

template <typename T, int DQK, int DV>
struct FwdCfg {
  static constexpr int EB = Elem<T>::kBytes;
  static constexpr int EPU = 16 / EB;            // elements per 16-byte unit
  static constexpr int UPR_K = DQK * EB / 16;    // units per K row
  static constexpr int UPR_V = DV * EB / 16;
  static constexpr int KT = 32 * DQK * EB;       // bytes of a 32-row K tile
  static constexpr int VT = 32 * DV * EB;
  static constexpr int STAGE = KT + VT;
  static constexpr int KG = DQK / 16;            // 16-wide contraction groups of QK^T
  static constexpr int DB = DV / 32;             // 32-wide output blocks
  static constexpr int NKU = (32 * UPR_K + kFwdThreads - 1) / kFwdThreads;  // staged units / thread
  static constexpr int NVU = (32 * UPR_V + kFwdThreads - 1) / kFwdThreads;
  // K/V ring filled by LDS-DMA.  Counted vmcnt waits need every wave to issue the same number of
  // DMA instructions per tile (whole multiples of the 4 waves); otherwise depth 2 with full drains.
  static constexpr int NCH_K = 32 * UPR_K / 64, NCH_V = 32 * UPR_V / 64;
  static constexpr bool COUNTED = (NCH_K % 4 == 0) && (NCH_V % 4 == 0);
  static constexpr int PER_TILE = NCH_K / 4 + NCH_V / 4;      // DMA instructions per wave per tile
  static constexpr int NS = (COUNTED && STAGE <= 16384) ? 3 : 2;  // ring depth (= tiles in flight + 1)
  static constexpr int SMEM = NS * STAGE;
};

// ---- general backward (hstu_attn_bwd.cuh) ----
constexpr int kBwdThreads = 512;
constexpr int kBwdWaves = 8;

template <typename T, int DQK, int DV>
struct BwdCfg {
  static constexpr int EB = Elem<T>::kBytes;
  static constexpr int EPU = 16 / EB;
  static constexpr int UPR_K = DQK * EB / 16;
  static constexpr int UPR_V = DV * EB / 16;
  static constexpr int KT = 32 * DQK * EB;
  static constexpr int VT = 32 * DV * EB;
  static constexpr int PAIR = KT + VT;            // K+V tile, also Q+dO stage
  static constexpr int DSROW = (EB == 2) ? 72 : 144;  // padded [key][32 q] row of the dS buffer
  static constexpr int DSBUF = 32 * DSROW;
  static constexpr int KGQ = DQK / 16;
  static constexpr int KGV = DV / 16;
  static constexpr int DBQ = DQK / 32;
  static constexpr int DBV = DV / 32;
  static constexpr int NQU = (32 * UPR_K + kBwdThreads - 1) / kBwdThreads;
  static constexpr int NOU = (32 * UPR_V + kBwdThreads - 1) / kBwdThreads;
  static constexpr int smem_bytes(int nw, int extra = 0) { return nw * PAIR + PAIR + 2 * nw * DSBUF + extra; }
  // at most 7 key tiles per block: the 8th wave never owns a tile, so every step has a
  // helper wave for the dQ GEMM of the previous step
  static constexpr int max_tiles(int lds_budget) {
    int nw = (lds_budget - PAIR) / (PAIR + 2 * DSBUF);
    return nw > kBwdWaves - 1 ? kBwdWaves - 1 : nw;
  }
};

// ---- folded backward (hstu_attn_bwd_fold.cuh) ----
template <typename T, int DQK, int DV>
struct FoldCfg {
  using B = BwdCfg<T, DQK, DV>;
  static constexpr int DSB = 32 * 64;                    // [32 keys][32 q] 16-bit tile, 64-byte rows
  static constexpr int kMaxTiles = kBwdWaves - 1;
  // all kMaxTiles K/V slots are always allocated (the dQ GEMM reads every slot, used or not)
  static constexpr int smem_bytes() { return (kMaxTiles + 2) * B::PAIR + kBwdWaves * DSB; }
};

// ---- four-wave backward, head dim 64 (hstu_attn_bwd_quad.cuh) ----
constexpr int kQuadWaves = 4;
constexpr int kQuadThreads = 256;

template <typename T, int D>
struct QuadCfg {
  using B = BwdCfg<T, D, D>;
  static constexpr int DSB = 32 * 64;                 // [32 keys][32 q] 16-bit dS' tile
  static constexpr int kMaxTiles = 7;
  // 7 K/V pairs + one Q/dO stage + 7 dS' tiles
  static constexpr int smem_bytes() { return kMaxTiles * B::PAIR + B::PAIR + kMaxTiles * DSB; }
};

// ---- two-kernel backward for long sequences (hstu_attn_bwd_long.cuh) ----
#ifndef LONG_NW
#define LONG_NW 7
#endif
#ifndef LONG_STAGES
#define LONG_STAGES 3
#endif
constexpr int kLongNW = LONG_NW;            // key tiles (owner waves) per block of the dK / dV kernel
constexpr int kLongStages = LONG_STAGES;    // its Q / dO ring
static_assert(kLongNW <= kBwdWaves && kLongStages >= 2 && (kLongNW + kLongStages) * 16 <= 160, "LDS");

template <typename T, int D>
struct LongCfg {
  using B = BwdCfg<T, D, D>;
  static constexpr int smem_dkv() { return (kLongNW + kLongStages) * B::PAIR; }
};

// ---- short sequences, one wave per problem (hstu_attn_solo.cuh) ----
constexpr int kSoloWaves = 4;
constexpr int kSoloThreads = 256;
constexpr int kSoloD = 32;          // instantiated head dim (16-bit: 64-byte rows, 2 KiB tiles)
constexpr int kSoloMaxLen = 64;
constexpr int kSoloBucketBytes = 3 * 1024;   // a user's time buckets as bytes (solo_bucket_bytes)
// workgroups per SIMD of the backward launch that takes the problems of <= 32 rows only (hstu_attn_bwd_solo_kernel, TPT = 1)
#ifndef SOLO_BWD_SHORT_WAVES
#define SOLO_BWD_SHORT_WAVES 4
#endif

template <typename T>
struct SoloCfg {
  static constexpr int TILE = 32 * kSoloD * Elem<T>::kBytes;      // 2048
  static constexpr int UPR = kSoloD * Elem<T>::kBytes / 16;        // 4
  // per wave: K, V, Q (2 tiles each; forward: 12 KiB -> 3 workgroups per CU) + dO and 2 dS' tiles (backward: 20 KiB)
  static constexpr int bwd_slice(int tpt = 2) { return tpt * (4 * TILE + 32 * 64); }
  static constexpr int fwd_slice(int tpt = 2) { return 3 * tpt * TILE; }   // the output tile is parked over the query tile it came from
};

}  // namespace hstu
