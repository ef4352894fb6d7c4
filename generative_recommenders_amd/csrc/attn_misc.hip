// The attention dispatch plan (capi_internal.h: AttnPlan) and what reads it without launching an attention kernel: the
// kernel names, the backward's workspace size, the reduction of the bias-gradient partial rows.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "attn_cfg.cuh"
#include "attn_dma_addr.h"
#include "capi_internal.h"
namespace hstu {
namespace {

// The A/B switches of the dispatch, each read once.  A switch that is "0" turns its schedule off (the general kernel, or
// one launch instead of two, runs instead); HSTU_ATTN_PRECISE=1 turns the precise forward on; HSTU_BWD_NW caps the key
// tiles per block of the general backward.
struct Env {
  bool fold = on("HSTU_BWD_FOLD"), long_bwd = on("HSTU_BWD_LONG"), solo = on("HSTU_SOLO"), solo_bias = on("HSTU_SOLO_BIAS"),
       quad = on("HSTU_BWD_QUAD"), bias_fold = on("HSTU_BIAS_FOLD"), bias_head_loop = on("HSTU_BIAS_HEAD_LOOP"),
       solo_split = on("HSTU_SOLO_SPLIT"), solo_bias_split = on("HSTU_SOLO_BIAS_SPLIT");
  bool precise = [] { const char* e = getenv("HSTU_ATTN_PRECISE"); return e && e[0] == '1'; }();
  int bwd_nw = [] { const char* e = getenv("HSTU_BWD_NW"); return e ? atoi(e) : 0; }();
  static bool on(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
};
const Env& env() {
  static const Env e;
  return e;
}

// LDS sizes of the instantiation for an element size and padded head dims, read from the kernels' own configurations
struct DimCfg {
  int fwd_smem;                          // FwdCfg::SMEM: the K/V ring
  int (*bwd_max_tiles)(int lds_budget);  // BwdCfg
  int (*bwd_smem)(int nw, int extra);
  int fold_smem, quad_smem, long_dkv_smem;   // dqk == dv only
};
template <typename T, int A, int V>
constexpr DimCfg dim_cfg_of() {
  DimCfg c{FwdCfg<T, A, V>::SMEM, &BwdCfg<T, A, V>::max_tiles, &BwdCfg<T, A, V>::smem_bytes, 0, 0, 0};
  if constexpr (A == V) {
    c.fold_smem = FoldCfg<T, A, A>::smem_bytes();
    c.quad_smem = QuadCfg<T, A>::smem_bytes();
    c.long_dkv_smem = LongCfg<T, A>::smem_dkv();
  }
  return c;
}
#define ROW(T, A) {dim_cfg_of<T, A, 32>(), dim_cfg_of<T, A, 64>(), dim_cfg_of<T, A, 128>()}
constexpr DimCfg kDimCfg[2][3][3] = {{ROW(bf16_t, 32), ROW(bf16_t, 64), ROW(bf16_t, 128)}, {ROW(float, 32), ROW(float, 64), ROW(float, 128)}};
#undef ROW
static_assert(Elem<bf16_t>::kBytes == Elem<f16_t>::kBytes, "bf16 and f16 share their sizes");
const DimCfg& dim_cfg(const HstuAttnParams& p, int a, int v) { return kDimCfg[p.dtype == HSTU_DTYPE_F32][a / 64][v / 64]; }
using Solo = SoloCfg<bf16_t>;             // (16-bit I/O only)
static_assert(QuadCfg<bf16_t, 64>::smem_bytes() <= 80 * 1024, "two workgroups per CU");

int tiles_of(int rows) { return (rows + 31) / 32; }

// The kernels that start a masked element's S accumulator at -1e30 (hstu_attn_bwd_fold.cuh, fold_pair) need alpha * 1e30
// to stay finite and alpha * 1.44e30 to overflow exp2; alpha == 0 is fine (every product with a masked element is then
// multiplied by alpha = 0 or by silu(0) = 0 anyway)
bool alpha_in_mask_range(float alpha) {
  const float aa = alpha < 0.f ? -alpha : alpha;
  return aa == 0.f || (aa > 1e-20f && aa < 1e6f);
}

// The folded schedule needs: 16-bit I/O, no bias, no contextual rows, one key block of <= 7 tiles, and head
// dims equal to an instantiated size (its LDS-DMA staging cannot zero-pad).
bool attn_bwd_fold_applicable(const HstuAttnParams& p) {
  if (!env().fold || p.dtype == HSTU_DTYPE_F32 || p.pos_w || p.contextual_seq_len > 0) return false;
  if (p.dqk != p.dv || (p.dqk != 128 && p.dqk != 64)) return false;
  return alpha_in_mask_range(p.alpha) && tiles_of(p.max_seq_len) <= 7;
}

// The two-kernel backward for long sequences (hstu_attn_bwd_long.cuh): longer than the folded schedule takes -- or
// contextual rows, which it does not take at any length
bool attn_bwd_long_applicable(const HstuAttnParams& p) {
  if (!env().long_bwd || p.dtype == HSTU_DTYPE_F32 || p.pos_w || p.delta_q != 0) return false;
  if (p.dqk != p.dv || (p.dqk != 128 && p.dqk != 64)) return false;
  return alpha_in_mask_range(p.alpha) && (tiles_of(p.max_seq_len) > 7 || (p.contextual_seq_len > 0 && p.max_seq_len > 64));
}

// short sequences (max_seq_len <= 64, head dims <= 32, 16-bit I/O): one wave per (user, head) (hstu_attn_solo.cuh)
bool attn_solo_applicable(const HstuAttnParams& p, bool backward) {
  if (!env().solo || p.dtype == HSTU_DTYPE_F32 || p.pos_w || p.delta_q != 0) return false;
  if (p.max_seq_len > kSoloMaxLen || p.dqk > kSoloD || p.dv > kSoloD) return false;
  return !(backward && p.contextual_seq_len > 0) && alpha_in_mask_range(p.alpha);
}

// Time buckets are few and lopsided (most pairs of a user fall in the top three or four): the lanes of a wave mostly
// add to the SAME histogram entry and the LDS atomics serialise.  Every lane group therefore gets its own copy of
// the time-bucket histogram (entry b of copy c at b * copies + c: the lanes of a wave that share a bucket hit
// consecutive words), as many copies as fit without costing a key tile; the copies are summed at the flush.
int hist_bytes(const HstuAttnParams& p, int copies) { return ((2 * p.max_seq_len + (p.num_buckets + 1) * copies) * 4 + 15) / 16 * 16; }
// ... behind `fixed` bytes of everything else: 32, 8 or 1 copies, whichever fits first
bool fit_hist(const HstuAttnParams& p, int fixed, AttnLaunch* l) {
  for (int c : {32, 8, 1}) {
    const int hist = hist_bytes(p, c);
    if (fixed + hist > kLdsBudget) continue;
    if (l) l->ts_copies = c, l->hist = hist, l->smem = fixed + hist;
    return true;
  }
  return false;
}
// LDS of a short-sequence research backward launch: four slices, histograms, tables (double-buffered: hstu_attn_solo.cuh),
// two sets of bucket bytes
bool solo_bias_bwd_lds(const HstuAttnParams& p, int tpt, AttnLaunch* l) {
  return fit_hist(p, kSoloWaves * Solo::bwd_slice(tpt) + 2 * bias_table_bytes(p.max_seq_len, p.num_buckets) + 2 * (tpt == 1 ? 1024 : kSoloBucketBytes), l);
}
int solo_bias_fwd_smem(const HstuAttnParams& p) {
  return kSoloWaves * (Solo::fwd_slice(2) + bias_table_bytes(p.max_seq_len, p.num_buckets) + kSoloBucketBytes);
}

// research path at the short-sequence shapes (Amazon-Books: N = 61, 4 heads of 16): relative bias inside the one-wave-per-
// (user, head) kernels.  16-bit I/O, max_seq_len <= 64, head dims <= 32, <= 255 time buckets (bucket bytes), no contextual
// rows, no delta
bool attn_solo_bias_applicable(const HstuAttnParams& p, bool backward) {
  if (!env().solo_bias || !p.pos_w || p.dtype == HSTU_DTYPE_F32 || p.delta_q != 0 || p.contextual_seq_len > 0) return false;
  if (p.max_seq_len > kSoloMaxLen || p.dqk > kSoloD || p.dv > kSoloD || p.num_buckets > 255) return false;
  if (!alpha_in_mask_range(p.alpha)) return false;
  if (p.max_seq_len + 32 + 3 > kSoloThreads) return false;      // (a thread per timestamp entry)
  return backward ? solo_bias_bwd_lds(p, 2, nullptr) : solo_bias_fwd_smem(p) <= kLdsBudget;
}

// research-path backward on the folded schedule: head dim 64, 16-bit I/O, the whole sequence in 7 tiles, position AND
// time tables.  LDS behind the folded kernel's own: histograms, tables, one bucket byte per element of the causal
// triangle of 7 tiles
bool attn_bwd_fold_bias_applicable(const HstuAttnParams& p, AttnLaunch* l) {
  if (!env().bias_fold || !p.pos_w || !p.ts_w || !p.timestamps) return false;
  if (p.dtype == HSTU_DTYPE_F32 || p.contextual_seq_len > 0 || p.dqk != 64 || p.dv != 64) return false;
  if (p.num_buckets > 255 || tiles_of(p.max_seq_len) > 7 || !alpha_in_mask_range(p.alpha)) return false;
  return fit_hist(p, FoldCfg<bf16_t, 64, 64>::smem_bytes() + bias_table_bytes(p.max_seq_len, p.num_buckets) + 28 * 1024, l);
}

// research-path forward, short sequences: does one workgroup per (user, query block) walk the heads with the time
// buckets of its tile pairs as bytes in LDS (hstu_attn_fwd.cuh, HEADS instantiation)?  *cache = those bytes
bool attn_fwd_head_loop_applicable(const HstuAttnParams& p, int ring_bytes, int tables, int nqb, int* cache_out) {
  const int tmax = tiles_of(p.max_seq_len);
  // 1 KiB per key tile and wave: wave w of query block qb keeps 4 qb + w + 1 tiles.  The LARGEST block counts -- not
  // always the last one: at 129..160 rows the last block has one wave with rows (5 tiles) and the first four (1 + 2 + 3 + 4)
  int cache = 0;
  for (int qb = 0; qb < nqb; ++qb) {
    int c = 0;
    for (int w = 0; w < 4; ++w)
      if (4 * qb + w < tmax) c += (4 * qb + w + 1) * 1024;
    if (c > cache) cache = c;
  }
  *cache_out = cache;
  return p.pos_w && p.dtype != HSTU_DTYPE_F32 && p.heads > 1 && p.delta_q == 0 && tmax <= 7 && p.ts_w && p.timestamps &&
         p.num_buckets <= 255 && p.contextual_seq_len == 0 && ring_bytes + tables + cache <= 52 * 1024 && env().bias_head_loop;
}

// key tiles per block of the general backward with `extra_lds` bytes of LDS taken by something else
int bwd_tiles(const DimCfg& dc, int dqk_padded, int max_seq_len, int extra_lds) {
  int nw = dc.bwd_max_tiles(kLdsBudget - extra_lds);
  const int need = tiles_of(max_seq_len);
  if (need <= nw) return need < 1 ? 1 : need;        // one key block: no dq accumulation, no scratch
  // several key blocks: the helpers' fp32 dq partials go through a per-wave LDS scratch tile (kDqScratchBytes)
  nw = dc.bwd_max_tiles(kLdsBudget - extra_lds - kDqScratchBytes);
  // Away from the diagonal every key tile of the block is active in every step: nw owner waves run one pair each while the
  // 8 - nw others run the dQ GEMM of the previous query tile, dealt in whole 32-feature blocks (at most DQK/32 helpers
  // have work).  With the block as large as the LDS allows the owners wait for them most of every step (cycle trace,
  // N = 1024, 128-wide heads, 5 tiles: owners 6 K cycles, helpers 12.5 K), and a sequence that does not divide into
  // such blocks ends in a block of one or two tiles whose workgroup is mostly idle waves.  Measured (tools/long_bwd.py
  // with HSTU_BWD_NW = 3..7 at N = 256 .. 8192): at most 6 tiles per block at head dim 64 (N = 8192: 13.0 -> 10.2 ms),
  // 5 at 32 (N = 1024: 5.7 -> 4.0 ms), and the tiles spread EVENLY over the fewest blocks that takes (16 tiles at head
  // dim 128 = 4 x 4 instead of 5 + 5 + 5 + 1: 11.8 -> 9.0 ms).  Dealing single (feature block, key tile) contractions
  // to the helpers instead -- every one busy -- was measured too and is slower: each partial sum pays the LDS transpose
  // and 16 atomic instructions of its own.
  const int cap = dqk_padded >= 128 ? 5 : (dqk_padded >= 64 ? 6 : 5);
  if (nw > cap) nw = cap;
  if (nw < 1) nw = 1;
  const int blocks = (need + nw - 1) / nw;
  nw = (need + blocks - 1) / blocks;
  if (env().bwd_nw > 0 && env().bwd_nw < nw) nw = env().bwd_nw;
  return nw < 1 ? 1 : nw;
}

// LDS bytes of the research-path bias state of a general backward workgroup (histograms with *ts_copies privatised
// copies of the time-bucket histogram + the staged tables); 0 without bias
int bwd_bias_lds(const HstuAttnParams& p, const DimCfg& dc, int dqk_padded, int* ts_copies) {
  *ts_copies = 1;
  if (!p.pos_w) return 0;
  auto bytes = [&](int nc) { return hist_bytes(p, nc) + bias_table_bytes(p.max_seq_len, p.num_buckets); };
  const int base = bwd_tiles(dc, dqk_padded, p.max_seq_len, bytes(1));
  for (int c : {32, 8})
    if (bwd_tiles(dc, dqk_padded, p.max_seq_len, bytes(c)) == base) { *ts_copies = c; break; }
  return bytes(*ts_copies);
}

int refuse(AttnPlan& pl, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(pl.msg, sizeof(pl.msg), fmt, ap);
  va_end(ap);
  return pl.err = code;
}

// as many workgroups as fit a CU (LDS) walk the problems, four at a time
int solo_grid(int total, int per_cu, int n_cu) {
  const int wgs = (total + kSoloWaves - 1) / kSoloWaves;
  return wgs < per_cu * n_cu ? wgs : per_cu * n_cu;
}

// the bias-gradient part of the workspace behind `off` bytes: the launches' partial rows, then the chunk sums of the
// two-stage reduce (chunks ~ sqrt(rows): both stages are one thread per column walking its rows one after the other, and
// with a fixed 128 chunks the second stage was 128 dependent loads for the 256 .. 768 rows of the persistent kernels:
// 31 us per backward call, 12 % of the Amazon-Books research-path backward: profiles/r06_c3bias_rocprofv3_pmc.md)
constexpr int kRedChunks = 128;
void plan_partial_rows(AttnPlan& pl, const HstuAttnParams& p, size_t off, int rows, bool user_counter) {
  pl.partial_off = off;
  pl.partial_rows = rows;
  pl.partial_width = 2 * p.max_seq_len + p.num_buckets;
  const size_t bytes = (size_t)rows * pl.partial_width * sizeof(float);
  // (the user counter of the dynamic hand-out sits right behind the partial rows, in the first word of the region the
  // reduce's chunk sums take over AFTER the kernel: one memset zeroes both)
  pl.counter_off = off + bytes;
  pl.zero_bytes = bytes + (user_counter ? sizeof(int) : 0);
  pl.red_chunks = 1;
  while (pl.red_chunks * pl.red_chunks < rows && pl.red_chunks < kRedChunks) ++pl.red_chunks;
  pl.chunk_off = off + bytes;
  pl.ws_bytes = pl.chunk_off + (size_t)pl.red_chunks * pl.partial_width * sizeof(float);
}

AttnPlan new_plan(const HstuAttnParams& p, bool backward) {
  AttnPlan pl;
  memset(&pl, 0, sizeof(pl));
  pl.dtype = p.dtype;
  pl.backward = backward;
  pl.a = pad_head_dim(p.dqk), pl.v = pad_head_dim(p.dv);
  pl.bias = p.pos_w != nullptr;
  pl.contextual = p.contextual_seq_len > 0;
  pl.n_launch = 1;
  pl.n_slabs = 1;
  return pl;
}

}  // namespace

AttnPlan plan_attn_fwd(const HstuAttnParams& p) {
  AttnPlan pl = new_plan(p, false);
  AttnLaunch& l = pl.launch[0];
  if (pl.a == 0 || pl.v == 0) return refuse(pl, HSTU_EUNSUPPORTED, "hstu_attn_fwd: head dims (%d, %d) not instantiated", p.dqk, p.dv), pl;
  const int n_cu = cu_count();
  // (the short-sequence forwards stay ONE launch: splitting them by length class like the backward ones measured -1 % (plain) and +14 %
  // (bias: 168 registers for three waves per SIMD cost 19 spills) on the Amazon-Books batch -- a forward wave's time is instruction
  // issue, not latency)
  if (attn_solo_applicable(p, false)) {
    pl.sched = kSchedSolo;
    l = {2, solo_grid(p.batch * p.heads, 3, n_cu), kSoloWaves * Solo::fwd_slice(2), 0, 0, 0, 0, kSoloMaxLen, 0};
    return pl;
  }
  if (attn_solo_bias_applicable(p, false)) {      // a wave per user (its own tables and bucket bytes), at most two workgroups per CU
    pl.sched = kSchedSoloBias;
    const int smem = solo_bias_fwd_smem(p);
    const int per_cu = kLdsBudget / smem < 2 ? kLdsBudget / smem : 2;
    l = {2, solo_grid(p.batch, per_cu, n_cu), smem, 0, 0, bias_table_bytes(p.max_seq_len, p.num_buckets), 0, kSoloMaxLen, 0};
    return pl;
  }
  if (pl.bias && pl.a != pl.v)
    return refuse(pl, HSTU_EUNSUPPORTED, "hstu_attn_fwd: relative-bias attention is instantiated for dqk == dv in {32, 64, 128} (got %d, %d)", p.dqk, p.dv), pl;
  pl.sched = kSchedGeneral;
  const int ring = dim_cfg(p, pl.a, pl.v).fwd_smem;
  const int q_rows = p.delta_q > 0 ? p.delta_q : p.max_seq_len;
  pl.nqb = (q_rows + kFwdRowsPerBlock - 1) / kFwdRowsPerBlock;
  const int tables = pl.bias ? bias_table_bytes(p.max_seq_len, p.num_buckets) : 0;
  int cache = 0;
  pl.head_loop = attn_fwd_head_loop_applicable(p, ring, tables, pl.nqb, &cache);
  // the output error at the rounding floor of the I/O dtype, ~20-25 % slower (hstu_attn_fwd.cuh, PRECISE)
  pl.precise = !pl.bias && p.dtype != HSTU_DTYPE_F32 && pl.a == pl.v && (pl.a == 64 || pl.a == 128) && env().precise;
  const int groups = ((pl.head_loop ? p.batch : p.batch * p.heads) + 7) / 8;
  l.grid = groups * 8 * pl.nqb;
  l.smem = ring + tables + (pl.head_loop ? cache : 0);
  l.tables = pl.head_loop ? tables : 0;
  if (l.smem > kLdsBudget) refuse(pl, HSTU_EUNSUPPORTED, "hstu_attn_fwd: max_seq_len %d needs %d bytes of LDS for the bias tables", p.max_seq_len, l.smem);
  return pl;
}

AttnPlan plan_attn_bwd(const HstuAttnBwdParams& bp) {
  const HstuAttnParams& p = bp.fwd;
  AttnPlan pl = new_plan(p, true);
  AttnLaunch* l = pl.launch;
  if (pl.a == 0 || pl.v == 0) return refuse(pl, HSTU_EUNSUPPORTED, "hstu_attn_bwd: head dims (%d, %d) not instantiated", p.dqk, p.dv), pl;
  const DimCfg& dc = dim_cfg(p, pl.a, pl.v);
  const int n_cu = cu_count();
  const int tmax = tiles_of(p.max_seq_len);
  if (attn_solo_applicable(p, true)) {
    // two launches by length class (hstu_attn_solo.cuh): problems of 33 .. 64 rows with the full slices (two workgroups per CU), problems
    // of <= 32 rows with one tile per tensor (SOLO_BWD_SHORT_WAVES per CU); HSTU_SOLO_SPLIT=0: one launch for everything.  (The two
    // launches one after the other: putting the long class on a side stream of the device -- fork / join by events -- measured SLOWER,
    // 69 -> 83 us on the Amazon-Books batch: profiles/r06_ab_solo_length_classes.txt)
    pl.sched = kSchedSolo;
    const int total = p.batch * p.heads, lo = env().solo_split ? 32 : 0;
    pl.n_launch = 0;
    if (p.max_seq_len > lo) l[pl.n_launch++] = {2, solo_grid(total, 2, n_cu), kSoloWaves * Solo::bwd_slice(2), 0, 0, 0, lo, kSoloMaxLen, 0};
    if (lo) l[pl.n_launch++] = {1, solo_grid(total, SOLO_BWD_SHORT_WAVES, n_cu), kSoloWaves * Solo::bwd_slice(1), 0, 0, 0, 0, lo, 0};
  } else if (attn_solo_bias_applicable(p, true)) {
    // a workgroup per user at a time, its waves the heads; two launches by length class: users of 33 .. 64 rows with the full slices
    // (one workgroup per CU), users of <= 32 rows with one tile per tensor (two per CU); HSTU_SOLO_BIAS_SPLIT=0: one launch
    pl.sched = kSchedSoloBias;
    const int lo = env().solo_bias_split ? 32 : 0;
    pl.n_launch = 0;
    if (p.max_seq_len > lo) l[pl.n_launch++] = {2, 0, 0, 1, 0, 0, lo, kSoloMaxLen, 0};
    if (lo) l[pl.n_launch++] = {1, 0, 0, 1, 0, 0, 0, lo, 0};
    int rows = 0;
    for (int i = 0; i < pl.n_launch; ++i) {
      if (!solo_bias_bwd_lds(p, l[i].tpt, &l[i])) return refuse(pl, HSTU_EUNSUPPORTED, "hstu_attn_bwd(solo, bias): LDS"), pl;
      const int per_cu = (l[i].tpt == 1 && 2 * l[i].smem <= kLdsBudget) ? 2 : 1;
      l[i].grid = p.batch < per_cu * n_cu ? p.batch : per_cu * n_cu;
      l[i].tables = bias_table_bytes(p.max_seq_len, p.num_buckets);
      l[i].row0 = rows;
      rows += l[i].grid;
    }
    plan_partial_rows(pl, p, 0, rows, false);
  } else if (attn_bwd_fold_applicable(p)) {
    pl.nw = tmax;
    if (p.dqk == 64 && env().quad) {        // 4-wave workgroups, two per CU, one per problem (hstu_attn_bwd_quad.cuh)
      pl.sched = kSchedQuad;
      l[0].grid = p.batch * p.heads, l[0].smem = dc.quad_smem;
    } else {                                // one persistent workgroup per CU (never more workgroups than problems: every workgroup reads its first problem's offsets)
      pl.sched = kSchedFold;
      l[0].grid = p.batch * p.heads < n_cu ? p.batch * p.heads : n_cu, l[0].smem = dc.fold_smem;
    }
  } else if (attn_bwd_long_applicable(p)) {
    pl.sched = kSchedLong;
    const int groups = (p.batch * p.heads + 7) / 8;
    pl.nkb = (tmax + kLongNW - 1) / kLongNW;
    pl.nqb = (p.max_seq_len + kFwdRowsPerBlock - 1) / kFwdRowsPerBlock;
    pl.n_launch = 2;
    l[0].grid = groups * 8 * pl.nkb, l[0].smem = dc.long_dkv_smem;
    l[1].grid = groups * 8 * pl.nqb, l[1].smem = dc.fwd_smem;
  } else if (pl.bias && pl.a != pl.v) {
    return refuse(pl, HSTU_EUNSUPPORTED, "hstu_attn_bwd: relative-bias attention is instantiated for dqk == dv in {32, 64, 128} (got %d, %d)", p.dqk, p.dv), pl;
  } else if (attn_bwd_fold_bias_applicable(p, &l[0])) {
    pl.sched = kSchedFoldBias;
    pl.nw = tmax;
    l[0].grid = p.batch < n_cu ? p.batch : n_cu;
    l[0].tables = bias_table_bytes(p.max_seq_len, p.num_buckets);
    plan_partial_rows(pl, p, 0, l[0].grid, true);
  } else {
    pl.sched = kSchedGeneral;
    const int hist = bwd_bias_lds(p, dc, pl.a, &l[0].ts_copies);
    pl.nw = bwd_tiles(dc, pl.a, p.max_seq_len, hist);
    pl.nkb = (p.max_seq_len + 32 * pl.nw - 1) / (32 * pl.nw);
    // research-path bias with the whole sequence in one key block: one workgroup per USER walks the heads and keeps the
    // time-bucket matrix as bytes in LDS (1 KiB per tile pair of the causal triangle), see hstu_attn_bwd.cuh
    const int cache = pl.nw * (pl.nw + 1) / 2 * 1024;
    pl.head_loop = pl.bias && pl.nkb == 1 && p.heads > 1 && p.ts_w && p.timestamps && p.num_buckets <= 255 && p.contextual_seq_len == 0 &&
                   dc.bwd_smem(pl.nw, hist + cache) <= kLdsBudget && env().bias_head_loop;
    const int groups = ((pl.head_loop ? p.batch : p.batch * p.heads) + 7) / 8;
    l[0].grid = groups * 8 * pl.nkb;
    l[0].smem = dc.bwd_smem(pl.nw, hist + (pl.nkb > 1 ? kDqScratchBytes : 0) + (pl.head_loop ? cache : 0));
    l[0].hist = pl.head_loop ? hist : 0;
    // several key blocks: an fp32 dq accumulator for their atomic adds, or (deterministic) one slab per key block that block
    // kb stores into, and a second launch that converts (and sums) it: 16 bytes of dq per thread
    if (pl.nkb > 1) {
      pl.slab_bytes = ((size_t)bp.total_rows * p.heads * p.dqk * sizeof(float) + 255) / 256 * 256;
      pl.n_slabs = bp.deterministic ? pl.nkb : 1;
      const int64_t n = bp.total_rows * p.heads * (int64_t)(p.dqk / (p.dtype == HSTU_DTYPE_F32 ? 4 : 8));
      pl.n_launch = 2;
      l[1].grid = (int)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384);
    }
    pl.ws_bytes = pl.slab_bytes * pl.n_slabs;
    if (pl.bias) plan_partial_rows(pl, p, pl.ws_bytes, l[0].grid, false);
    if (l[0].smem > kLdsBudget)
      return refuse(pl, HSTU_EUNSUPPORTED, "hstu_attn_bwd: max_seq_len %d needs %d bytes of LDS for the bias histograms", p.max_seq_len, l[0].smem), pl;
  }
  // the kernels built on fold_problem_x / quad_problem: how they address their tile requests is a constant of the launch
  if (pl.sched == kSchedFold || pl.sched == kSchedQuad || pl.sched == kSchedFoldBias) {
    const int64_t eb = dtype_bytes(p.dtype);
    pl.dma_fast = attn_bwd_dma_fast(p.q_row_stride * eb, p.k_row_stride * eb, p.v_row_stride * eb, bp.do_row_stride * eb, 32 * (int64_t)pl.nw);
  }
  if (pl.bias && bp.deterministic)
    refuse(pl, HSTU_EUNSUPPORTED, "hstu_attn_bwd: deterministic = 1 is not available with the relative bias (the table gradients are "
                                  "histograms of float atomics)");
  return pl;
}

// Profiler name of the instantiation a plan launches (the launch tests compare it with the kernel names rocprofv3 reports)
int attn_kernel_name(const AttnPlan& pl, char* buf, size_t len) {
  if (!buf || len == 0) return HSTU_EINVAL;
  if (pl.sched == kSchedNone) { buf[0] = 0; return set_error(pl.err, "%s", pl.msg); }
  const char* dt = pl.dtype == HSTU_DTYPE_BF16 ? "bf16" : (pl.dtype == HSTU_DTYPE_F16 ? "f16" : "f32");
  const char* dir = pl.backward ? "bwd" : "fwd";
  switch (pl.sched) {
    case kSchedSolo: snprintf(buf, len, "hstu_attn_%s_solo_kernel<%s>", dir, dt); break;
    case kSchedSoloBias: snprintf(buf, len, "hstu_attn_%s_solo_bias_kernel<%s>", dir, dt); break;
    case kSchedQuad: snprintf(buf, len, "hstu_attn_bwd_quad_kernel<%s,%d>", dt, pl.a); break;
    case kSchedFold: snprintf(buf, len, "hstu_attn_bwd_fold_kernel<%s,%d,%d>", dt, pl.a, pl.v); break;
    case kSchedLong: snprintf(buf, len, "hstu_attn_bwd_dkv_kernel<%s,%d>+hstu_attn_bwd_dq_kernel<%s,%d>", dt, pl.a, dt, pl.a); break;
    case kSchedFoldBias: snprintf(buf, len, "hstu_attn_bwd_fold_bias_kernel<%s,64>", dt); break;
    default: {
      const char* variant = pl.bias ? ",bias" : "";
      if (!pl.backward && pl.head_loop) variant = ",bias,heads";
      if (pl.precise) variant = ",precise";
      snprintf(buf, len, "hstu_attn_%s_kernel<%s,%d,%d%s>", dir, dt, pl.a, pl.v, variant);
    }
  }
  return HSTU_OK;
}

// column sums of the (rows, width) partial matrix in two fixed-order stages (deterministic across launches):
// stage 1, grid (column blocks, chunks): every workgroup sums its contiguous chunk of rows for 64 columns into
// row `chunk` of the plan's chunk-sum rows; stage 2: one thread per column sums the chunk rows.  (One thread per column
// over ALL rows -- the first version -- took 3.6 ms for the 32768 partial rows of an 8192-user batch: 9 waves on the
// whole chip.)

__global__ void bias_grad_reduce_stage1(const float* partial, int rows, int width, int chunks, float* chunk_sums) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= width) return;
  const int per = (rows + chunks - 1) / chunks;
  const int r0 = blockIdx.y * per, r1 = min(r0 + per, rows);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int r = r0;
  for (; r + 3 < r1; r += 4) {
    s0 += partial[(int64_t)r * width + c];
    s1 += partial[(int64_t)(r + 1) * width + c];
    s2 += partial[(int64_t)(r + 2) * width + c];
    s3 += partial[(int64_t)(r + 3) * width + c];
  }
  for (; r < r1; ++r) s0 += partial[(int64_t)r * width + c];
  chunk_sums[(int64_t)blockIdx.y * width + c] = (s0 + s1) + (s2 + s3);
}

__global__ void bias_grad_reduce_stage2(const float* chunk_sums, int chunks, int width, int npos, float* dpos_w, float* dts_w) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= width) return;
  // (four independent partial sums: the loads of a column are 4 deep in flight instead of one after the other)
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int r = 0;
  for (; r + 3 < chunks; r += 4) {
    s0 += chunk_sums[(int64_t)r * width + c];
    s1 += chunk_sums[(int64_t)(r + 1) * width + c];
    s2 += chunk_sums[(int64_t)(r + 2) * width + c];
    s3 += chunk_sums[(int64_t)(r + 3) * width + c];
  }
  for (; r < chunks; ++r) s0 += chunk_sums[(int64_t)r * width + c];
  const float s = (s0 + s1) + (s2 + s3);
  if (c < npos) dpos_w[c] = s;
  else if (dts_w) dts_w[c - npos] = s;
}

int launch_bias_grad_reduce(const AttnPlan& pl, void* workspace, int npos, float* dpos_w, float* dts_w, hipStream_t st) {
  const float* partial = (const float*)((char*)workspace + pl.partial_off);
  float* chunk_sums = (float*)((char*)workspace + pl.chunk_off);
  const int width = pl.partial_width, chunks = pl.red_chunks;
  hipLaunchKernelGGL(bias_grad_reduce_stage1, dim3((width + 63) / 64, chunks), dim3(64), 0, st, partial, pl.partial_rows, width, chunks, chunk_sums);
  if (int e = check_launch("hstu_attn_bwd(bias gradient reduce 1)")) return e;
  hipLaunchKernelGGL(bias_grad_reduce_stage2, dim3((width + 63) / 64), dim3(64), 0, st, chunk_sums, chunks, width, npos, dpos_w, dts_w);
  return check_launch("hstu_attn_bwd(bias gradient reduce 2)");
}

}  // namespace hstu
