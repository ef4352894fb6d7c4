#!/usr/bin/env python3
"""Fused jagged causal softmax attention against its composition on one MI355X: one JSON object on stdout (and, with
--out, in a file).

Shapes: the four shipped SASRec configurations with gr_output_length added, (N, H, d) = ml-1m (210, 1, 50), ml-20m
(210, 4, 64), ml-3b (510, 4, 64), amzn-books (60, 4, 16), bf16, at the configs' batch of 128 users and at 2048 users -- 128
users are a launch-scale problem on 256 CUs, so both are reported.  Lengths come from common.generate_sparse_seq_len
(sparsity 0.8), q / k / v as the module hands them over (k and v two column slices of one buffer).  Timed per point: forward,
and forward + backward, of ops.softmax_attention.jagged_causal_softmax_attention (fused HIP kernels) and of
jagged_causal_softmax_attention_composed (padded (B, H, N, N) scores through torch), in the same process and alternating
round by round, HIP events after a pre-warm and a warm-up; the median of the rounds is reported.  FLOPs and bytes are
algorithmic, from the shapes and the drawn lengths: 4 d flops per visible (query, key) pair forward (QK^T and PV), 10 d
backward (S and dP recomputed, dV, dQ, dK); bytes = q, k, v, out once forward, plus dO, dq, dk, dv backward.

    python tools/bench_sasrec_attention.py [--iters 20] [--rounds 5] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.common import generate_sparse_seq_len  # noqa: E402
from generative_recommenders_amd.ops import _launch  # noqa: E402
from generative_recommenders_amd.ops.softmax_attention import (  # noqa: E402
    jagged_causal_softmax_attention,
    jagged_causal_softmax_attention_composed,
)

DEV = "cuda"
SHAPES = {"ml-1m": (210, 1, 50), "ml-20m": (210, 4, 64), "ml-3b": (510, 4, 64), "amzn-books": (60, 4, 16)}
BATCHES = (128, 2048)


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def run(name, n, H, d, B, iters, rounds):
    torch.manual_seed(1)
    lengths = generate_sparse_seq_len(size=B, max_seq_len=n, sparsity=0.8, device=torch.device(DEV)).clamp(min=1)
    offsets = _launch.complete_cumsum(lengths)
    rows = int(offsets[-1].item())
    qbuf = torch.randn(rows, H * d, device=DEV).bfloat16().requires_grad_(True)
    kvbuf = torch.randn(rows, 2 * H * d, device=DEV).bfloat16().requires_grad_(True)
    dout = torch.randn(rows, H, d, device=DEV).bfloat16()
    q = qbuf.view(rows, H, d)
    k, v = kvbuf[:, : H * d].view(rows, H, d), kvbuf[:, H * d:].view(rows, H, d)
    assert _launch.softmax_attn_supported(q.dtype, d, n)

    def fwd(f):
        with torch.no_grad():
            return f(n, q, k, v, offsets)

    def fwd_bwd(f):
        qbuf.grad = kvbuf.grad = None
        f(n, q, k, v, offsets).backward(dout)

    fns = {
        "fused_fwd": lambda: fwd(jagged_causal_softmax_attention),
        "composed_fwd": lambda: fwd(jagged_causal_softmax_attention_composed),
        "fused_fwd_bwd": lambda: fwd_bwd(jagged_causal_softmax_attention),
        "composed_fwd_bwd": lambda: fwd_bwd(jagged_causal_softmax_attention_composed),
    }
    for fn in fns.values():                                  # pre-warm (allocator, kernel load), then warm-up
        fn()
    torch.cuda.synchronize()
    for fn in fns.values():
        _events_ms(fn, 3)
    ms = {m: [] for m in fns}
    for _ in range(rounds):
        for m, fn in fns.items():
            ms[m].append(_events_ms(fn, iters))
    med = {m: statistics.median(v_) for m, v_ in ms.items()}
    ln = lengths.to(torch.float64)
    pairs = float((ln * (ln + 1) / 2).sum().item()) * H
    flops_fwd, flops_bwd = 4.0 * d * pairs, 10.0 * d * pairs
    bytes_fwd, bytes_bwd = 4 * rows * H * d * 2, 8 * rows * H * d * 2
    return {
        "shape": name, "N": n, "H": H, "d": d, "users": B, "rows": rows, "dtype": "bfloat16", "timed_iterations": iters * rounds,
        **{m + "_ms": round(x, 4) for m, x in med.items()},
        "fwd_speedup": round(med["composed_fwd"] / med["fused_fwd"], 2),
        "fwd_bwd_speedup": round(med["composed_fwd_bwd"] / med["fused_fwd_bwd"], 2),
        "fused_fwd_ms_rounds": [round(x, 4) for x in ms["fused_fwd"]],
        "fused_fwd_bwd_ms_rounds": [round(x, 4) for x in ms["fused_fwd_bwd"]],
        "flops_fwd": flops_fwd, "flops_fwd_bwd": flops_fwd + flops_bwd, "bytes_fwd": bytes_fwd, "bytes_fwd_bwd": bytes_fwd + bytes_bwd,
        "fused_fwd_tflops": round(flops_fwd / med["fused_fwd"] * 1e-9, 2),
        "fused_fwd_bwd_tflops": round((flops_fwd + flops_bwd) / med["fused_fwd_bwd"] * 1e-9, 2),
        "fused_fwd_gbs": round(bytes_fwd / med["fused_fwd"] * 1e-6, 1),
        "composed_scores_bytes": B * H * n * n * 2,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    points = [run(s, *SHAPES[s], B, args.iters, args.rounds) for s in args.shapes.split(",") for B in BATCHES]
    result = {"tool": "bench_sasrec_attention", "device": torch.cuda.get_device_name(0), "points": points}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
