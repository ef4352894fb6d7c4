#!/usr/bin/env python3
"""The fused multitask prediction head against this package's own composition on one MI355X: one JSON object on stdout
(and, with --out, in a file).

Shape: rows = 131,072 of dim = 512 in bf16 (the hidden tensor behind DlrmHSTU's first prediction Linear), T = 1 (one
binary task) and T = 5 (3 binary + 2 regression), labels randint(0, 11) / randn, weights uniform(0, 2).  Timed per T:
forward and forward + backward of ``ops.multitask.multitask_head`` and, in the same process and alternating with it round
by round, what a caller had before it: ``swish_layer_norm`` (HIP) -> ``torch.addmm`` onto the T columns -> sigmoid / BCE /
MSE / normalisation in torch, and its autograd backward.  HIP events after a pre-warm and a warm-up; the median of the
rounds is reported.

Bytes are algorithmic (s = 2): forward rows dim s read + 2 T rows 4 written (logits and preds); backward 2 rows dim s (x
read, dx written) + the (T, rows) fp32 tensors it reads (logits, labels, weights, grad_pred).  The op is HBM-bound
(~10 FLOP / B); the line gives ms and the fraction of 8 TB/s.

    python tools/bench_multitask_head.py [--iters 20] [--rounds 7] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.ops.layer_norm import swish_layer_norm  # noqa: E402
from generative_recommenders_amd.ops.multitask import multitask_head  # noqa: E402

PEAK_HBM = 8.0e12
DEV = "cuda"
SCALE = 0.3


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def composition(x, g, b, w, c, labels, weights, nbin):
    """the head from this package's ops as they stood before the fused kernel"""
    y = swish_layer_norm(x, g, b, 1e-5)
    logits = torch.addmm(c.to(y.dtype), y, w.to(y.dtype).t()).t().float()
    preds = torch.cat([torch.sigmoid(logits[:nbin]), logits[nbin:]], 0)
    parts = []
    if nbin > 0:
        parts.append(F.binary_cross_entropy_with_logits(logits[:nbin], labels[:nbin], reduction="none") * weights[:nbin])
    if nbin < logits.shape[0]:
        parts.append(F.mse_loss(logits[nbin:], labels[nbin:], reduction="none") * weights[nbin:])
    losses = torch.cat(parts, 0).sum(-1) / weights.sum(-1).clamp(min=1.0) * SCALE
    return preds, losses


def run(rows, dim, nbin, nreg, iters, rounds):
    T = nbin + nreg
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(rows, dim, device=DEV, generator=gen).to(torch.bfloat16).requires_grad_()
    g = (1 + 0.1 * torch.randn(dim, device=DEV, generator=gen)).requires_grad_()
    b = (0.1 * torch.randn(dim, device=DEV, generator=gen)).requires_grad_()
    w = (torch.randn(T, dim, device=DEV, generator=gen) / dim ** 0.5).requires_grad_()
    c = (0.1 * torch.randn(T, device=DEV, generator=gen)).requires_grad_()
    labels = torch.cat([torch.randint(0, 11, (nbin, rows), device=DEV, generator=gen).float(),
                        torch.randn(nreg, rows, device=DEV, generator=gen)], 0)
    weights = 2 * torch.rand(T, rows, device=DEV, generator=gen)
    r = torch.randn(T, rows, device=DEV, generator=gen)
    leaves = (x, g, b, w, c)

    def fused_fwd():
        with torch.no_grad():
            return multitask_head(x, g, b, 1e-5, w, c, labels, weights, nbin, SCALE)

    def comp_fwd():
        with torch.no_grad():
            return composition(x, g, b, w, c, labels, weights, nbin)

    def both(fn):
        for t in leaves:
            t.grad = None
        preds, losses = fn()
        (losses.sum() + (preds * r).sum()).backward()

    fns = {
        "fused_fwd": fused_fwd,
        "composition_fwd": comp_fwd,
        "fused_fwd_bwd": lambda: both(lambda: multitask_head(x, g, b, 1e-5, w, c, labels, weights, nbin, SCALE)),
        "composition_fwd_bwd": lambda: both(lambda: composition(x, g, b, w, c, labels, weights, nbin)),
    }
    (pa, la), (pb, lb) = fused_fwd(), comp_fwd()
    agree = {"preds_rel_fro": float((pa - pb).norm() / pb.norm()), "losses_rel_fro": float((la - lb).norm() / lb.norm())}
    for fn in fns.values():         # pre-warm (code objects, hipBLASLt's choice, the allocator) and warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():   # alternating: every round times every variant once
            times[k].append(_events_ms(fn, iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    s = 2
    fwd_bytes = rows * dim * s + 2 * T * rows * 4
    bwd_bytes = 2 * rows * dim * s + 4 * T * rows * 4
    res = {
        "shape": {"rows": rows, "dim": dim, "binary_tasks": nbin, "regression_tasks": nreg, "dtype": "bfloat16"},
        "ms": {k: round(v, 4) for k, v in med.items()},
        "ms_rounds": {k: [round(v, 4) for v in vs] for k, vs in times.items()},
        "fused_over_composition": {"fwd": round(med["fused_fwd"] / med["composition_fwd"], 3),
                                   "fwd_bwd": round(med["fused_fwd_bwd"] / med["composition_fwd_bwd"], 3)},
        "fused_vs_composition": agree,
        "algorithmic_bytes": {"fwd": fwd_bytes, "fwd_bwd": fwd_bytes + bwd_bytes},
        "frac_of_8TBps": {"fused_fwd": round(fwd_bytes / (med["fused_fwd"] * 1e-3) / PEAK_HBM, 3),
                          "fused_fwd_bwd": round((fwd_bytes + bwd_bytes) / (med["fused_fwd_bwd"] * 1e-3) / PEAK_HBM, 3),
                          "composition_fwd": round(fwd_bytes / (med["composition_fwd"] * 1e-3) / PEAK_HBM, 3),
                          "composition_fwd_bwd": round((fwd_bytes + bwd_bytes) / (med["composition_fwd_bwd"] * 1e-3) / PEAK_HBM, 3)},
    }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multitask_head.py measures on the GPU: none found")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "workloads": {}}
    for name, (nbin, nreg) in (("T1", (1, 0)), ("T5", (3, 2))):
        res["workloads"][name] = run(args.rows, args.dim, nbin, nreg, args.iters, args.rounds)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
