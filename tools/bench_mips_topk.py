#!/usr/bin/env python3
"""Fused MIPS top-k against torch.mm + torch.topk on one MI355X: one JSON object on stdout (and, with --out, in a file).

Shapes: the research configs' evaluation, B = 1024 users against the whole corpus with k' = 2500 + N0 (N0 = the width of
past_ids, which get_top_k_outputs fetches on top of MAX_K): ML-1M (X = 3,953, D = 50, N0 = 211), ML-20M (X = 131,263,
D = 256, N0 = 211), Amazon-Books (X = 695,763, D = 64, N0 = 61), each in bf16 and fp32.  Timed per point: the fused op
(hstu_mips_topk through ops._launch.mips_topk, table padded once as the module does) and, in the same process and
alternating with it round by round, the reference's composition torch.mm(queries, table^T) + torch.topk(k', sorted) -- and
the composition's mm alone.  HIP events after a pre-warm and a warm-up; rounds x iters >= 100 timed iterations per point,
the median of the rounds is reported.  The composition writes a (B, X) matrix; the fused op's workspace is reported next
to it.

    python tools/bench_mips_topk.py [--iters 20] [--rounds 5] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd import _lib as L  # noqa: E402
from generative_recommenders_amd.ops import _launch  # noqa: E402

DEV = "cuda"
SHAPES = {"ml-1m": (1024, 3953, 50, 211), "ml-20m": (1024, 131263, 256, 211), "amzn-books": (1024, 695763, 64, 61)}
DTYPES = {"bfloat16": torch.bfloat16, "float32": torch.float32}


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def run(name, B, X, D, n0, dtype_name, iters, rounds):
    dt = DTYPES[dtype_name]
    k = min(2500 + n0, X)
    gen = torch.Generator(device=DEV).manual_seed(1)
    q = torch.nn.functional.normalize(torch.randn(B, D, device=DEV, generator=gen), dim=1).to(dt)
    table = torch.nn.functional.normalize(torch.randn(X, D, device=DEV, generator=gen), dim=1).to(dt)
    dp = _launch.mips_topk_dim(D, dt)
    padded = torch.nn.functional.pad(table, (0, dp - D)).contiguous()          # once, as MIPSBruteForceTopK's constructor does
    table_t = table.t()

    fns = {
        "fused": lambda: _launch.mips_topk(q, padded, k),
        "mm_topk": lambda: torch.topk(torch.mm(q, table_t), k=k, dim=1, sorted=True, largest=True),
        "mm": lambda: torch.mm(q, table_t),
    }
    for fn in fns.values():                                                    # pre-warm (allocator, kernel load), then warm-up
        fn()
    torch.cuda.synchronize()
    for fn in fns.values():
        _events_ms(fn, 3)
    ms = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            ms[n].append(_events_ms(fn, iters))
    med = {n: statistics.median(v) for n, v in ms.items()}
    es = q.element_size()
    return {
        "shape": name, "dtype": dtype_name, "B": B, "X": X, "D": D, "k": k, "timed_iterations": iters * rounds,
        "fused_ms": round(med["fused"], 4), "mm_topk_ms": round(med["mm_topk"], 4), "mm_ms": round(med["mm"], 4),
        "fused_over_mm_topk": round(med["fused"] / med["mm_topk"], 3),
        "fused_ms_rounds": [round(v, 4) for v in ms["fused"]], "mm_topk_ms_rounds": [round(v, 4) for v in ms["mm_topk"]],
        "score_matrix_bytes": B * X * es, "fused_workspace_bytes": int(L.lib().hstu_mips_topk_workspace_bytes(B, k)),
        "table_bytes": X * dp * es,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    points = [run(n, *SHAPES[n], d, args.iters, args.rounds) for n in args.shapes.split(",") for d in DTYPES]
    result = {"tool": "bench_mips_topk", "device": torch.cuda.get_device_name(0), "points": points}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
