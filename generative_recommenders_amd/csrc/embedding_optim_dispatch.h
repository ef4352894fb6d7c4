// Everything the host decides for the in-backward embedding optimizers and the coalesce (embedding_optim.hip): the chunk
// size, the row class, the two workspace layouts, the grids and their cap, the combine kernel's LDS bytes and every entry
// point's widest row.  Host-only, plain C++ with no HIP in it, and every function a pure function of its arguments -- the
// sort's temporary bytes are a parameter, the unit passes what rocprim asks for.  tests/test_embedding_optim_dispatch_host.py
// compiles this header alone and sweeps it; the unit instantiates exactly the classes reachable() names.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hstu {
namespace embedding_optim {

constexpr int kOptWaves = 4;           // waves per workgroup of the chunk kernel, a chunk each
constexpr int kChunkLarge = 128;       // sorted rows per wave of the chunk kernel: two coalesced loads of the (id, row) pairs
constexpr int kChunkSmall = 32;        // below kSmallBatch ids: four times the waves, a quarter of the groups each walks
constexpr int64_t kSmallBatch = 262144;
constexpr int kSmallChunkMaxDim = 512; // four times the partial sums of a quarter of the widest row: the same workspace
constexpr int kCombineWaves = 8;       // waves that share one cut segment's partial sums
constexpr int kOptMaxPieces = 4;       // 16-byte pieces per lane and dout row: rows of up to 4 KiB
constexpr int kOptMaxDim = 2048;       // 4 KiB of bf16 / fp16: the widest partial sum (8 KiB of fp32)
constexpr int kOptMaxBlocks = 8192;    // grid-stride above this
constexpr int kScanThreads = 256;      // the coalesce's rank scan: threads per tile ...
constexpr int kScanItems = 8;          // ... consecutive positions per thread: two 16-byte stores of ranks
constexpr int kScanTile = kScanThreads * kScanItems;
constexpr int kTileScanThreads = 1024;
static_assert(kChunkLarge / kChunkSmall * kSmallChunkMaxDim <= kOptMaxDim, "the small chunks' partial sums must fit the workspace");

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int64_t capped(int64_t blocks) { return blocks < kOptMaxBlocks ? blocks : kOptMaxBlocks; }

// The widest gradient row an entry point takes: 4 KiB (kOptMaxPieces pieces per lane), or for fp32 rows -- the coalesced lists
// of tables of up to kOptMaxDim columns -- 8 KiB where the entry point takes those (wide_fp32: the coalesced Adagrad entry,
// the 16-bit Adagrad, SGD and Adam; not the fp32 Adagrad entry and not the coalesce itself): dim <= kOptMaxDim either way
constexpr int max_row_bytes(int elem_bytes, bool wide_fp32) {
  return wide_fp32 && elem_bytes == 4 ? kOptMaxDim * (int)sizeof(float) : kOptMaxPieces * 64 * 16;
}

// Small chunks for small batches, where the partial sums (packed at the row's own width) still fit the room laid out for the
// large ones: 2 * ceil(n / 32) * dim <= 2 * 4 * ceil(n / 128) * (kOptMaxDim / 4) for dim <= kSmallChunkMaxDim.
constexpr int chunk_of(int64_t n, int dim) { return n < kSmallBatch && dim <= kSmallChunkMaxDim ? kChunkSmall : kChunkLarge; }

// np: 16-byte pieces per lane and gradient row; u: gradient rows in flight per wave -- eight for rows of up to 1 KiB (the
// reference's dim 256 in any dtype), fewer for wider rows: each comes with a table row of twice (16-bit dout) or once its size
// in registers (the coalesce keeps them: the groups do not change the order of a sum, and one rule is one thing less to test).
// Eight pieces: coalesced fp32 rows of tables wider than 1024 columns, 8 KiB, which only an applying sink takes.
struct RowClass {
  int np, u;
};
constexpr RowClass row_class(int elem_bytes, int dim, bool applies) {
  const int row_bytes = dim * elem_bytes;
  if (row_bytes <= 1024) return {1, 8};
  if (row_bytes <= 2048) return {2, 4};
  if (elem_bytes == 4 && applies && row_bytes > 4096) return {8, 2};
  return {4, elem_bytes == 2 ? 2 : 4};
}

// every value row_class takes: the unit's template switch walks this list
constexpr RowClass kRowClasses[] = {{1, 8}, {2, 4}, {4, 2}, {4, 4}, {8, 2}};

// whether some legal (dim, n) lands in the class: what the unit compiles, no more and no less
constexpr bool reachable(int elem_bytes, int np, int u, int chunk, bool applies) {
  if (chunk != kChunkSmall && chunk != kChunkLarge) return false;
  const int vec = 16 / elem_bytes;
  for (int dim = vec; dim * elem_bytes <= max_row_bytes(elem_bytes, applies); dim += vec) {
    const RowClass c = row_class(elem_bytes, dim, applies);
    if (c.np == np && c.u == u && (chunk == kChunkLarge || chunk_of(0, dim) == kChunkSmall)) return true;
  }
  return false;
}
// ... and every legal row's class is on the list, so a reachable class cannot go uncompiled
constexpr bool row_classes_listed() {
  for (int elem_bytes = 2; elem_bytes <= 4; elem_bytes += 2)
    for (int applies = 0; applies < 2; ++applies)
      for (int dim = 16 / elem_bytes; dim * elem_bytes <= max_row_bytes(elem_bytes, applies); dim += 16 / elem_bytes) {
        const RowClass c = row_class(elem_bytes, dim, applies);
        bool listed = false;
        for (const RowClass& k : kRowClasses) listed = listed || (k.np == c.np && k.u == c.u);
        if (!listed) return false;
      }
  return true;
}
static_assert(row_classes_listed(), "row_class returned a class that kRowClasses does not list");

// One launch of the chunk and combine kernels (and, for the coalesce, of the scan kernels in front of them)
struct Plan {
  int np, u, chunk;
  int64_t chunks;
  int chunk_grid;
  int combine_grid;    // 0: one chunk, nothing can leave it -- no combine kernel
  size_t combine_lds;  // (kCombineWaves - 1) rows of dim floats: at most 56 KiB
  int64_t scan_tiles;
  int scan_grid;
};
constexpr Plan plan(int elem_bytes, int dim, int64_t n, bool applies) {
  const RowClass c = row_class(elem_bytes, dim, applies);
  Plan p{};
  p.np = c.np;
  p.u = c.u;
  p.chunk = chunk_of(n, dim);
  p.chunks = ceil_div(n, p.chunk);
  p.chunk_grid = (int)capped(ceil_div(p.chunks, kOptWaves));
  p.combine_grid = p.chunks < 2 ? 0 : (int)capped(p.chunks - 1);
  p.combine_lds = (size_t)(kCombineWaves - 1) * dim * sizeof(float);
  p.scan_tiles = ceil_div(n, kScanTile);
  p.scan_grid = (int)capped(p.scan_tiles);
  return p;
}

// sorted_idx | perm (n each) | partial sums (two per 128 positions, sized for the widest row: dim is not known here, and the
// size must not depend on it) | sort temporary
struct OptLayout {
  size_t part, partials_off, temp_off, temp_bytes, total;
};
constexpr OptLayout opt_layout(int64_t n, size_t sort_temp) {
  OptLayout l{};
  l.part = align256((size_t)n * sizeof(int32_t));
  l.partials_off = 2 * l.part;
  l.temp_off = l.partials_off + align256(2 * (size_t)ceil_div(n, kChunkLarge) * kOptMaxDim * sizeof(float));
  l.temp_bytes = n ? sort_temp : 0;
  l.total = l.temp_off + align256(l.temp_bytes);
  return l;
}
// the floats the partial sums of plan p take (two slots per chunk, packed at the row's width), and the room they have
constexpr size_t partials_bytes(const Plan& p, int dim) { return 2 * (size_t)p.chunks * dim * sizeof(float); }
constexpr size_t partials_room(const OptLayout& l) { return l.temp_off - l.partials_off; }

// the update's workspace | rank (n) | heads per scan tile
struct CoalesceLayout {
  OptLayout opt;
  size_t rank_off, tiles_off, total;
};
constexpr CoalesceLayout coalesce_layout(int64_t n, size_t sort_temp) {
  CoalesceLayout l{};
  l.opt = opt_layout(n, sort_temp);
  l.rank_off = l.opt.total;
  l.tiles_off = l.rank_off + align256((size_t)n * sizeof(int32_t));
  l.total = l.tiles_off + align256((size_t)ceil_div(n, kScanTile) * sizeof(int32_t));
  return l;
}

}  // namespace embedding_optim
}  // namespace hstu
