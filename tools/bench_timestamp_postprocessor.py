#!/usr/bin/env python3
"""TimestampLayerNormPostprocessor on one MI355X: the fused path (aligned GEMM + one row pass, ops/timestamp_layer_norm.py)
against the composition on this package's ops (hstu_time_features -> cat -> addmm with the 516-long contraction ->
layer_norm).  One JSON object on stdout, and in --out.

bf16, D = 512, the two DLRM periods, at 81,920 rows (8192 users x 10 candidates) and 204,800 rows (full embeddings).  Both
paths run in ONE process on the same inputs, timed with HIP events after a warm-up, alternating fused / composed rounds;
the median per call is reported for the forward and for forward + backward (gradients of x and of the four parameters).
Bytes are algorithmic, for the row pass alone (the two GEMMs move the same x / z0 / dz on either path): forward reads z0 and
writes y; backward reads z0 and dy and writes dz -- 2 bytes each per element; timestamps, statistics and parameters are
below 1 %.  max_abs_diff compares the two paths' outputs and x-gradients on the timed inputs.

    python tools/bench_timestamp_postprocessor.py [--iters 20] [--rounds 7] [--out profiles/timestamp_postprocessor.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.ops import _launch  # noqa: E402
from generative_recommenders_amd.ops.timestamp_layer_norm import timestamp_layer_norm, timestamp_layer_norm_composed  # noqa: E402

DEV = "cuda"
SHAPES = {"candidates_81920x512": (81920, 512), "full_204800x512": (204800, 512)}
PERIODS = [(3600, 24), (86400, 7)]


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def run(rows, dim, iters, rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    f = len(PERIODS)
    x = torch.randn(rows, dim, device=DEV, generator=g).to(torch.bfloat16).requires_grad_()
    t = torch.randint(1_600_000_000, 1_760_000_000, (rows,), device=DEV, generator=g)
    w = (torch.randn(dim, dim + 2 * f, device=DEV, generator=g) * (2.0 / (2 * dim + 2 * f)) ** 0.5).requires_grad_()
    b = (0.1 * torch.randn(dim, device=DEV, generator=g)).requires_grad_()
    lw = (1.0 + 0.1 * torch.randn(dim, device=DEV, generator=g)).requires_grad_()
    lb = (0.1 * torch.randn(dim, device=DEV, generator=g)).requires_grad_()
    pu = torch.tensor([[float(p) for p, _ in PERIODS]], device=DEV)
    upp = torch.tensor([[float(u) for _, u in PERIODS]], device=DEV)
    dy = torch.randn(rows, dim, device=DEV, generator=g).to(torch.bfloat16)
    leaves = (x, w, b, lw, lb)
    assert _launch.time_ln_supported(dim, f, x.dtype)

    def fwd(fn):
        with torch.no_grad():
            return fn(x, t, w, b, lw, lb, pu, upp, 1e-5)

    def fwd_bwd(fn):
        for p in leaves:
            p.grad = None
        fn(x, t, w, b, lw, lb, pu, upp, 1e-5).backward(dy)

    paths = {"fused": timestamp_layer_norm, "composed": timestamp_layer_norm_composed}
    outs, gx = {}, {}
    for name, fn in paths.items():       # warm-up of every shape of the timed window, and the outputs to compare
        for _ in range(3):
            outs[name] = fwd(fn)
            fwd_bwd(fn)
        gx[name] = x.grad.clone()
    times = {k: {"fwd": [], "fwd_bwd": []} for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            times[name]["fwd"].append(_events_ms(lambda: fwd(fn), iters))
            times[name]["fwd_bwd"].append(_events_ms(lambda: fwd_bwd(fn), iters))
    med = {k: {m: statistics.median(v) for m, v in d.items()} for k, d in times.items()}
    elems = rows * dim
    row_pass_bytes = {"fwd": 2 * elems * 2, "fwd_bwd": 2 * elems * 2 + 3 * elems * 2}
    return {
        "shape": {"rows": rows, "dim": dim, "periods": PERIODS, "dtype": "bfloat16"},
        "ms": {k: {m: round(v, 4) for m, v in d.items()} for k, d in med.items()},
        "ms_rounds": {k: {m: [round(x_, 4) for x_ in v] for m, v in d.items()} for k, d in times.items()},
        "composed_over_fused": {m: round(med["composed"][m] / med["fused"][m], 3) for m in ("fwd", "fwd_bwd")},
        "row_pass_bytes": row_pass_bytes,
        "max_abs_diff": {"out": float((outs["fused"].float() - outs["composed"].float()).abs().max()),
                         "grad_x": float((gx["fused"].float() - gx["composed"].float()).abs().max())},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_timestamp_postprocessor: needs a GPU (a timing without one says nothing)")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "workloads": {}}
    for name in args.shapes.split(","):
        res["workloads"][name] = run(*SHAPES[name], args.iters, args.rounds)
        torch.cuda.empty_cache()
    text = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
