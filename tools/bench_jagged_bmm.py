#!/usr/bin/env python3
"""jagged_dense_bmm_broadcast_add on one MI355X: one JSON object on stdout (and, with --out, in a file).

Shapes: B = 1024 users, max_seq_len 200, K = 256 -> N = 512 (DLRM-v3's table dim -> transducer dim), bf16, with M-full
(every user 200 rows) and M-jag (uniform 100 .. 200) lengths, and a small-K point (K = 64) at M-full.  Timed per shape:
forward, data gradient, weight + bias gradient, and the three together through autograd -- and, in the same process and
alternating with them round by round, the composition a caller would otherwise write from this package's own ops:
jagged_to_padded_dense -> torch.bmm -> + bias -> dense_to_jagged, and its autograd backward.  HIP events after a pre-warm
and a warm-up; the median of the rounds is reported.

Bytes are algorithmic: forward (rows K + B K N + rows N) s + 4 B N (the fp32 bias), data gradient the same without the bias,
weight gradient (rows K + rows N + B K N) s + 4 B N.  At these shapes the arithmetic intensity is below the ~310 FLOP/B
ridge, so the bound is HBM (8 TB/s); the line gives GB/s and the fraction of it, and FLOP/s against 2.5 PFLOP/s.

    python tools/bench_jagged_bmm.py [--iters 20] [--rounds 5] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.ops import _launch  # noqa: E402
from generative_recommenders_amd.ops.jagged_tensors import (  # noqa: E402
    dense_to_jagged,
    jagged_dense_bmm_broadcast_add,
    jagged_to_padded_dense,
)

PEAK_HBM = 8.0e12
PEAK_FLOPS = 2.5e15
DEV = "cuda"


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def padded_composition(max_seq_len, off, jagged, dense, bias, rows):
    padded = jagged_to_padded_dense(jagged, off, max_seq_len)
    return dense_to_jagged(torch.bmm(padded, dense) + bias.unsqueeze(1), off, rows)


def run(name, B, N_len, K, N, lengths, iters, rounds):
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(lengths, 0)
    off = off.to(DEV)
    rows = int(off[-1])
    gen = torch.Generator(device=DEV).manual_seed(1)
    mk = lambda *s: (torch.rand(*s, device=DEV, generator=gen) * 2 - 1).to(torch.bfloat16)  # noqa: E731
    jagged, dense, bias = mk(rows, K).requires_grad_(), mk(B, K, N).requires_grad_(), mk(B, N).requires_grad_()
    d_out = (torch.randn(rows, N, device=DEV, generator=gen) * 0.01).to(torch.bfloat16)
    bias32 = bias.detach().float()
    jd, dd = jagged.detach(), dense.detach()

    def hip_all():
        for t in (jagged, dense, bias):
            t.grad = None
        jagged_dense_bmm_broadcast_add(N_len, off, jagged, dense, bias).backward(d_out)

    def pad_all():
        for t in (jagged, dense, bias):
            t.grad = None
        padded_composition(N_len, off, jagged, dense, bias, rows).backward(d_out)

    fns = {
        "hip_fwd": lambda: _launch.jagged_dense_bmm_fwd(jd, dd, bias32, off),
        "hip_dgrad": lambda: _launch.jagged_dense_bmm_fwd(d_out, dd.transpose(1, 2), None, off),
        "hip_wgrad": lambda: _launch.jagged_dense_bmm_wgrad(jd, d_out, off),
        "hip_fwd_bwd": hip_all,
        "padded_fwd": lambda: padded_composition(N_len, off, jd, dd, bias.detach(), rows),
        "padded_fwd_bwd": pad_all,
    }
    with torch.no_grad():
        a, b = fns["hip_fwd"](), fns["padded_fwd"]()
        diff = float((a.float() - b.float()).norm() / b.float().norm())
    for fn in fns.values():         # pre-warm (code objects, hipBLASLt's choice) and warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():   # alternating: every round times every variant once
            times[k].append(_events_ms(fn, iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    s = 2
    flop = 2.0 * rows * K * N
    bytes_ = {
        "hip_fwd": (rows * K + B * K * N + rows * N) * s + 4 * B * N,
        "hip_dgrad": (rows * N + B * K * N + rows * K) * s,
        "hip_wgrad": (rows * K + rows * N + B * K * N) * s + 4 * B * N,
    }
    bytes_["hip_fwd_bwd"] = sum(bytes_.values())
    res = {
        "shape": {"users": B, "max_seq_len": N_len, "K": K, "N": N, "rows": rows, "dtype": "bfloat16"},
        "ms": {k: round(v, 4) for k, v in med.items()},
        "ms_rounds": {k: [round(x, 4) for x in v] for k, v in times.items()},
        "hip_over_padded": {"fwd": round(med["hip_fwd"] / med["padded_fwd"], 3),
                            "fwd_bwd": round(med["hip_fwd_bwd"] / med["padded_fwd_bwd"], 3)},
        "flop_per_byte_fwd": round(flop / bytes_["hip_fwd"], 1),
        "fwd_vs_padded_rel_fro": diff,
    }
    for k, nb in bytes_.items():
        fl = flop * (3 if k == "hip_fwd_bwd" else 1)
        t = med[k] * 1e-3
        res[k] = {"bytes": nb, "GBps": round(nb / t / 1e9, 1), "frac_of_8TBps": round(nb / t / PEAK_HBM, 3),
                  "TFLOPs": round(fl / t / 1e12, 1), "frac_of_2.5PFLOPs": round(fl / t / PEAK_FLOPS, 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="M-full,M-jag,M-full-K64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    B, L = 1024, 200
    shapes = {
        "M-full": (256, 512, torch.full((B,), L)),
        "M-jag": (256, 512, torch.randint(L // 2, L + 1, (B,), generator=g)),
        "M-full-K64": (64, 512, torch.full((B,), L)),
    }
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "workloads": {}}
    for name in args.shapes.split(","):
        K, N, lengths = shapes[name]
        res["workloads"][name] = run(name, B, L, K, N, lengths, args.iters, args.rounds)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
