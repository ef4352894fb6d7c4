"""Compiles csrc/embedding_optim_dispatch.h ALONE with g++ (no HIP anywhere near it) into a small program and asks it for
the host plan of the embedding optimizers: the host tests sweep it.

A gradient dtype is named "bf16", "f16" or "f32"; `applies` is 1 for a sink that updates a table, 0 for the coalesce."""

import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")
DTYPES = {"bf16": 2, "f16": 2, "f32": 4}
CONSTS = ("opt_waves", "chunk_large", "chunk_small", "small_batch", "small_chunk_max_dim", "combine_waves", "max_pieces", "max_dim",
          "max_blocks", "scan_threads", "scan_items", "scan_tile", "tile_scan_threads")
PLAN = ("np", "u", "chunk", "chunks", "chunk_grid", "combine_grid", "combine_lds", "scan_tiles", "scan_grid", "partials_bytes",
        "partials_room")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "embedding_optim_dispatch.h"
using namespace hstu::embedding_optim;
int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "consts")) {
    printf("%d %d %d %lld %d %d %d %d %d %d %d %d %d\n", kOptWaves, kChunkLarge, kChunkSmall, (long long)kSmallBatch, kSmallChunkMaxDim,
           kCombineWaves, kOptMaxPieces, kOptMaxDim, kOptMaxBlocks, kScanThreads, kScanItems, kScanTile, kTileScanThreads);
    return 0;
  }
  if (argc >= 5 && !strcmp(argv[1], "sweep")) {      // sweep <elem bytes> <applies> <n> ..: every legal dim x every n
    const int eb = atoi(argv[2]);
    const bool applies = atoi(argv[3]) != 0;
    for (int dim = 16 / eb; dim * eb <= max_row_bytes(eb, applies); dim += 16 / eb)
      for (int i = 4; i < argc; ++i) {
        const long long n = atoll(argv[i]);
        const Plan p = plan(eb, dim, n, applies);
        printf("%d %lld %d %d %d %lld %d %d %zu %lld %d %zu %zu\n", dim, n, p.np, p.u, p.chunk, (long long)p.chunks, p.chunk_grid,
               p.combine_grid, p.combine_lds, (long long)p.scan_tiles, p.scan_grid, partials_bytes(p, dim),
               partials_room(opt_layout(n, 0)));
      }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "reachable")) {  // every class the unit compiles: <elem bytes> <applies> <np> <u> <chunk>
    for (int eb = 2; eb <= 4; eb += 2)
      for (int applies = 0; applies < 2; ++applies)
        for (const RowClass& c : kRowClasses)
          for (int chunk : {kChunkSmall, kChunkLarge})
            if (reachable(eb, c.np, c.u, chunk, applies)) printf("%d %d %d %d %d\n", eb, applies, c.np, c.u, chunk);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "layout")) {     // layout <n> <sort temporary bytes>
    const long long n = atoll(argv[2]);
    const CoalesceLayout l = coalesce_layout(n, (size_t)atoll(argv[3]));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", l.opt.part, l.opt.partials_off, l.opt.temp_off, l.opt.temp_bytes, l.opt.total, l.rank_off,
           l.tiles_off, l.total);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "rows")) {       // the widest row per (elem bytes, wide_fp32)
    printf("%d %d %d %d\n", max_row_bytes(2, false), max_row_bytes(2, true), max_row_bytes(4, false), max_row_bytes(4, true));
    return 0;
  }
  return 2;
}
"""


@functools.lru_cache(maxsize=None)
def _exe():
    d = tempfile.mkdtemp(prefix="embedding_optim_probe_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "probe.cpp"), os.path.join(d, "probe")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    return exe


def ask(*args):
    return subprocess.check_output([_exe(), *[str(a) for a in args]], text=True)


def consts():
    return dict(zip(CONSTS, (int(x) for x in ask("consts").split())))


def sweep(dtype, applies, ns):
    """(dim, n) -> dict of PLAN's fields, for every legal dim of the dtype and every n of `ns`"""
    out = {}
    for line in ask("sweep", DTYPES[dtype], int(applies), *ns).splitlines():
        v = [int(x) for x in line.split()]
        out[(v[0], v[1])] = dict(zip(PLAN, v[2:]))
    return out


def reachable():
    """the set of (elem bytes, applies, np, u, chunk) the unit compiles"""
    return {tuple(int(x) for x in line.split()) for line in ask("reachable").splitlines()}


def layout(n, sort_temp):
    names = ("part", "partials_off", "temp_off", "temp_bytes", "opt_total", "rank_off", "tiles_off", "total")
    return dict(zip(names, (int(x) for x in ask("layout", n, sort_temp).split())))


def max_row_bytes():
    """(elem bytes, wide_fp32) -> the widest row in bytes"""
    return dict(zip(((2, False), (2, True), (4, False), (4, True)), (int(x) for x in ask("rows").split())))
