"""Compiles csrc/quant_embedding_dispatch.h ALONE with g++ (no HIP anywhere near it) into a small program and asks it for
the geometry: the host tests sweep it, the GPU tests read the grid cap from it.

A `kind` names one of the header's splits: "quantize" (16 codes per lane, a row inside one wave), "gather4" (fp32 output:
4 codes per lane) and "gather2" (16-bit output: 8 codes per lane)."""

import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")
KINDS = ("quantize", "gather4", "gather2")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "quant_embedding_dispatch.h"
using namespace hstu::quant_embedding;
static Split split_of(const char* kind, int d) {
  if (!strcmp(kind, "quantize")) return quantize_split(d);
  return gather_split(d, !strcmp(kind, "gather4") ? 4 : 2);
}
int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "consts")) {
    printf("%d %d %d %d %d %d %d\n", kThreads, kWave, kMaxDim, kMaxPasses, kQuantizePiece, kGatherChunks, kBlocksPerCu);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "sweep")) {      // per dim: the scalars, then every (pass, lane) piece offset
    for (int d = 1; d <= kMaxDim; ++d) {
      const Split s = split_of(argv[2], d);
      printf("%d %d %d %d %d %d %d %d %d %d %d", d, (int)dim_ok(d), meta_offset(d), row_stride(d), row_pieces(d), s.piece, s.pieces,
             s.lanes, s.rows, s.passes, s.chunks);
      for (int p = 0; p < s.passes; ++p)
        for (int l = 0; l < s.lanes; ++l) printf(" %d", piece_offset(s, l, p));
      printf("\n");
    }
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "grid")) {       // grid <kind> <n> <dim> <cus>
    const long long n = atoll(argv[3]);
    const int d = atoi(argv[4]), cus = atoi(argv[5]);
    const Split s = split_of(argv[2], d);
    printf("%lld %d %lld %lld\n", (long long)steps(n, s), grid(n, s, cus), (long long)grid_cap(cus),
           (long long)steps_per_workgroup(n, s, cus));
    return 0;
  }
  return 2;
}
"""


@functools.lru_cache(maxsize=None)
def _exe():
    d = tempfile.mkdtemp(prefix="quant_embedding_probe_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "probe.cpp"), os.path.join(d, "probe")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    return exe


def ask(*args):
    return subprocess.check_output([_exe(), *[str(a) for a in args]], text=True)


def consts():
    names = ("threads", "wave", "max_dim", "max_passes", "quantize_piece", "gather_chunks", "blocks_per_cu")
    return dict(zip(names, (int(x) for x in ask("consts").split())))


@functools.lru_cache(maxsize=None)
def sweep(kind):
    """dim -> dict(ok, meta, stride, row_pieces, piece, pieces, lanes, rows, passes, chunks, offsets[pass][lane])"""
    out = {}
    for line in ask("sweep", kind).splitlines():
        v = [int(x) for x in line.split()]
        d, ok, meta, stride, row_pieces, piece, pieces, lanes, rows, passes, chunks = v[:11]
        offs = v[11:]
        assert len(offs) == passes * lanes
        out[d] = dict(ok=ok, meta=meta, stride=stride, row_pieces=row_pieces, piece=piece, pieces=pieces, lanes=lanes, rows=rows,
                      passes=passes, chunks=chunks, offsets=[offs[p * lanes:(p + 1) * lanes] for p in range(passes)])
    return out


def grid(kind, n, dim, cus):
    steps, g, cap, per_wg = (int(x) for x in ask("grid", kind, n, dim, cus).split())
    return dict(steps=steps, grid=g, cap=cap, steps_per_wg=per_wg)
