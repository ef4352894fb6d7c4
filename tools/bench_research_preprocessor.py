#!/usr/bin/env python3
"""The research-path input preprocessor on one MI355X: the fused op (ops/research_preprocess.py, PLAIN layout) against the
reference's composition written with torch ops (scale, (B, N, D) positional gather, add, dropout, mask multiply) on the same
GPU, in ONE process, on the same inputs, alternating fused / composed rounds.  One JSON object on stdout, and in --out.

(B, N, D) = (128, 211, 50), (128, 211, 256), (128, 61, 64), (8192, 200, 256), fp32 and bf16, p = 0.2 (the composition uses
torch's own dropout: the two masks differ, the work does not).  Timed with HIP events after a warm-up; the median per call
over the rounds is reported for the forward and for forward + backward (gradients of the embeddings and of the position
table).  Traffic model: one read and one write of B N D elements forward, and the same backward -- `fraction_of_8TBps` is
that many bytes over the fused time, against 8 TB/s.  Ids, the position table and the partial sums of its gradient are
outside the model (they are small against B N D at every shape but the first three, where everything is launch-bound).

    python tools/bench_research_preprocessor.py [--iters 20] [--rounds 7] [--out profiles/research_preprocessor.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.ops.research_preprocess import research_input_preprocess  # noqa: E402

DEV = "cuda"
SHAPES = [(128, 211, 50), (128, 211, 256), (128, 61, 64), (8192, 200, 256)]
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
P = 0.2
PEAK = 8.0e12


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def composed(ids, emb, pos, p):
    B, N = ids.shape
    D = emb.shape[-1]
    x = emb * (D ** 0.5) + torch.nn.functional.embedding(torch.arange(N, device=ids.device).unsqueeze(0).repeat(B, 1), pos)
    x = torch.nn.functional.dropout(x, p=p, training=True)
    valid = (ids != 0).unsqueeze(-1).float()
    x *= valid
    return x


def run(B, N, D, dtype, iters, rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    ids = torch.randint(0, 1000, (B, N), device=DEV, generator=g)
    ids = ids * (torch.arange(N, device=DEV).unsqueeze(0) < torch.randint(N // 2, N + 1, (B, 1), device=DEV, generator=g))
    emb = (0.05 * torch.randn(B, N, D, device=DEV, generator=g)).to(dtype).requires_grad_()
    pos = (0.1 * torch.randn(N, D, device=DEV, generator=g)).to(dtype).requires_grad_()
    dy = torch.randn(B, N, D, device=DEV, generator=g).to(dtype)
    paths = {"fused": lambda: research_input_preprocess(ids, emb, pos, dropout_ratio=P, seed=1234)[0],
             "composed": lambda: composed(ids, emb, pos, P)}

    def fwd(fn):
        with torch.no_grad():
            return fn()

    def fwd_bwd(fn):
        emb.grad = pos.grad = None
        fn().backward(dy)

    for fn in paths.values():
        for _ in range(3):
            fwd(fn)
            fwd_bwd(fn)
    with torch.no_grad():       # dropout off: the two paths compute the same thing
        same = research_input_preprocess(ids, emb, pos)[0]
        ref = composed(ids, emb, pos, 0.0)
        max_abs_diff = float((same.float() - ref.float()).abs().max())
    times = {k: {"fwd": [], "fwd_bwd": []} for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            times[name]["fwd"].append(_events_ms(lambda: fwd(fn), iters))
            times[name]["fwd_bwd"].append(_events_ms(lambda: fwd_bwd(fn), iters))
    med = {k: {m: statistics.median(v) for m, v in d.items()} for k, d in times.items()}
    size = torch.empty((), dtype=dtype).element_size()
    model_bytes = {"fwd": 2 * B * N * D * size, "fwd_bwd": 4 * B * N * D * size}
    return {
        "shape": {"B": B, "N": N, "D": D, "dtype": str(dtype).replace("torch.", ""), "p": P},
        "ms": {k: {m: round(v, 4) for m, v in d.items()} for k, d in med.items()},
        "ms_rounds": {k: {m: [round(x_, 4) for x_ in v] for m, v in d.items()} for k, d in times.items()},
        "composed_over_fused": {m: round(med["composed"][m] / med["fused"][m], 3) for m in ("fwd", "fwd_bwd")},
        "model_bytes": model_bytes,
        "fraction_of_8TBps": {m: round(model_bytes[m] / (med["fused"][m] * 1e-3) / PEAK, 4) for m in ("fwd", "fwd_bwd")},
        "max_abs_diff_dropout_off": max_abs_diff,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_research_preprocessor: needs a GPU (a timing without one says nothing)")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "workloads": {}}
    for B, N, D in SHAPES:
        for name, dtype in DTYPES.items():
            res["workloads"][f"b{B}_n{N}_d{D}_{name}"] = run(B, N, D, dtype, args.iters, args.rounds)
            torch.cuda.empty_cache()
    text = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
