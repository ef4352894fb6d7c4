#!/usr/bin/env python3
"""Mixture-of-Logits scoring, fused against composite, on one MI355X: one JSON object on stdout (and, with --out, in a file).

Shapes: B = 1024 queries against the catalogue sizes of the research configs -- ML-1M (X = 3,953), ML-20M (X = 131,263),
Amazon-Books (X = 695,763) -- with an 8 x 8 x 32 MoL (L = 64 logits, D_P = 32), H = 128 hidden units in the query-item gating
MLP, in bf16 and fp32.  Timed per point, in one process and alternating round by round:

* ``fused``: ``MoLSimilarity.forward`` in eval mode under ``no_grad`` (torch projections + hstu_mol_scores);
* ``fused_op``: hstu_mol_scores alone on operands computed once -- what ``MoLBruteForceTopK`` runs per query chunk; its
  share of the MFMA peak is FLOP = B X (2 L D_P + 4 L H) over the time, against 2516.6 TFLOP/s (bf16) / 157.3 (fp32);
* ``composite``: the same module's composite path (the reference's forward in torch ops) over query chunks sized so that
  the tensors it materialises -- about (5 L + 2 H) elements per pair -- stay within ``--composite-bytes``; it cannot run
  unchunked at these sizes at all.  ``composite_pair_bytes`` is that estimate, ``composite_unchunked_bytes`` what one
  unchunked call would need, ``logits_fp32_bytes`` the (B, X, L) fp32 logit tensor alone.

HIP events after a warm-up; the median of the rounds is reported.

    python tools/bench_mol_topk.py [--iters 2] [--rounds 3] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.research.modeling.similarity_utils import create_mol_interaction_module  # noqa: E402

DEV = "cuda"
SHAPES = {"ml-1m": 3953, "ml-20m": 131263, "amzn-books": 695763}
DTYPES = {"bfloat16": torch.bfloat16, "float32": torch.float32}
PEAK_TFLOPS = {"bfloat16": 2516.6, "float32": 157.3}
B, PQ, PX, DP, H, DIM = 1024, 8, 8, 32, 128, 64


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def run(name, X, dtype_name, iters, rounds, composite_bytes):
    dt = DTYPES[dtype_name]
    torch.manual_seed(1)
    module, debug_str = create_mol_interaction_module(
        query_embedding_dim=DIM, item_embedding_dim=DIM, dot_product_dimension=DP, query_dot_product_groups=PQ,
        item_dot_product_groups=PX, temperature=0.05, query_dropout_rate=0.0, query_hidden_dim=128, item_dropout_rate=0.0,
        item_hidden_dim=128, gating_query_hidden_dim=128, gating_qi_hidden_dim=H, gating_item_hidden_dim=128,
        softmax_dropout_rate=0.0, bf16_training=False)
    module = module.to(device=DEV, dtype=dt).eval()
    queries = torch.randn(B, DIM, device=DEV).to(dt)
    items = torch.randn(1, X, DIM, device=DEV).to(dt)
    L = PQ * PX
    pair_bytes = (5 * L + 2 * H) * queries.element_size()
    chunk = max(1, min(B, composite_bytes // (pair_bytes * X)))

    with torch.no_grad():
        xc, gi = module.fused_item_operands(items, dt)

    def fused():
        with torch.no_grad():
            return module(queries, items)[0]

    def fused_op():
        with torch.no_grad():
            return module.fused_scores(queries, xc, gi)

    def composite():
        with torch.no_grad():
            for b0 in range(0, B, chunk):
                module._composite(queries[b0:b0 + chunk], items)
    fns = {"fused": fused, "fused_op": fused_op, "composite": composite}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            ms[n].append(_events_ms(fn, iters))
    med = {n: statistics.median(v) for n, v in ms.items()}
    flop = B * X * (2 * L * DP + 4 * L * H)
    return {
        "shape": name, "dtype": dtype_name, "module": debug_str, "B": B, "X": X, "timed_iterations": iters * rounds,
        "fused_ms": round(med["fused"], 3), "fused_op_ms": round(med["fused_op"], 3), "composite_ms": round(med["composite"], 3),
        "fused_over_composite": round(med["fused"] / med["composite"], 3),
        "rounds_ms": {n: [round(v, 3) for v in vs] for n, vs in ms.items()},
        "fused_op_tflops": round(flop / med["fused_op"] / 1e9, 2),
        "fused_op_share_of_mfma_peak": round(flop / med["fused_op"] / 1e9 / PEAK_TFLOPS[dtype_name], 4),
        "fused_score_bytes": B * X * 4, "composite_query_chunk": chunk, "composite_pair_bytes": pair_bytes,
        "composite_chunk_bytes": chunk * X * pair_bytes, "composite_unchunked_bytes": B * X * pair_bytes,
        "logits_fp32_bytes": B * X * L * 4,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--composite-bytes", type=int, default=8 << 30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    points = []
    for n in args.shapes.split(","):
        for d in DTYPES:
            points.append(run(n, SHAPES[n], d, args.iters, args.rounds, args.composite_bytes))
            print(json.dumps(points[-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    result = {"tool": "bench_mol_topk", "device": torch.cuda.get_device_name(0), "points": points}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
