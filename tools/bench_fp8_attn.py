#!/usr/bin/env python3
"""fp8 (e4m3) vs bf16 HSTU attention forward on one MI355X: one JSON object on stdout.

Shapes: M-full (8192 users x L 200 x 4 heads x 128), M-jag (L = randint(180, 200)), and the config-5 delta step of
tools/bench_kv_cache.py (32 users x 16 heads x 64, ~8K cached rows, 256 candidate rows per user: delta_q attention).
Both dtypes are timed in ONE process with HIP events after a warm-up, alternating bf16 / fp8 rounds; the median per call is
reported.  Bytes are algorithmic: 1 B (fp8) or 2 B (bf16) per q / k / v element read, 2 B per output element written.
Errors: fp8_vs_bf16_rel_fro is the relative (Frobenius) difference of the fp8 forward against the bf16 forward run on the
dequantized inputs x8 * descale ROUNDED TO bf16 (not exact: descale is an arbitrary fp32 value), so it holds the bf16 path's
input rounding as well as both kernels' own roundings.  rel_fro_vs_fp64_oracle separates them: each path against the fp64
oracle on exactly the inputs it was given (fp8: x8 * descale in fp64; bf16: those values rounded to bf16), on the first
users of the batch.

    python tools/bench_fp8_attn.py [--iters 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.ops import _launch  # noqa: E402
from generative_recommenders_amd.ops import fp8 as F  # noqa: E402
from oracle import hstu_oracle as O  # noqa: E402

PEAK_HBM = 8.0e12
DEV = "cuda"


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def _shape(name, gen):
    if name in ("M-full", "M-jag"):
        B, N, H, d = 8192, 200, 4, 128
        lengths = torch.full((B,), N) if name == "M-full" else torch.randint(180, N + 1, (B,), generator=gen)
        return dict(B=B, N=N, H=H, d=d, lengths=lengths, delta=0)
    B, N, H, d, delta = 32, 8192, 16, 64, 256      # BASELINE config 5 (tools/bench_kv_cache.py)
    lengths = torch.randint(int(0.9 * N), N - delta, (B,), generator=gen) + delta
    return dict(B=B, N=N, H=H, d=d, lengths=lengths, delta=delta)


def _dequant(x8, ds, off):
    rows = torch.repeat_interleave(ds, off[1:] - off[:-1], dim=0)
    return (x8.float() * rows[:, :, None]).to(torch.bfloat16)


def run(name, iters, rounds, gen):
    s = _shape(name, gen)
    B, N, H, d, delta = s["B"], s["N"], s["H"], s["d"], s["delta"]
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(s["lengths"], 0)
    off = off.to(DEV)
    rows = int(off[-1])
    qrows = B * delta if delta else rows
    mk = lambda n: (torch.rand(n, H, d, device=DEV, generator=gen_dev) - 0.5) * 0.2  # noqa: E731
    gen_dev = torch.Generator(device=DEV).manual_seed(1)
    q, k, v = mk(qrows).to(torch.bfloat16), mk(rows).to(torch.bfloat16), mk(rows).to(torch.bfloat16)
    qoff = torch.arange(B + 1, device=DEV, dtype=torch.int64) * delta if delta else off
    # quantizer throughput (bf16 in, e4m3 + descales out; two passes over the input, the second from cache)
    F.quantize_jagged_fp8(k, off)
    tq = _events_ms(lambda: F.quantize_jagged_fp8(k, off), iters)
    quant_gbps = (k.numel() * 2 + k.numel() * 1) / (tq * 1e-3) / 1e9
    (q8, qd), (k8, kd), (v8, vd) = F.quantize_jagged_fp8(q, qoff), F.quantize_jagged_fp8(k, off), F.quantize_jagged_fp8(v, off)
    qb, kb, vb = _dequant(q8, qd, qoff), _dequant(k8, kd, off), _dequant(v8, vd, off)
    alpha = 1.0 / d**0.5

    def bf16():
        return _launch.attn_fwd(qb, kb, vb, off, None, N, alpha, 1.0 / N, delta_q=delta)

    def f8():
        return F.hstu_mha_fp8(N, alpha, q8, k8, v8, off, q_descale=qd, k_descale=kd, v_descale=vd, delta=bool(delta))

    ob, o8 = bf16(), f8()
    rel = float((o8.float() - ob.float()).norm() / ob.float().norm())
    # both paths against the fp64 oracle, first users only (numpy)
    nu = 32 if not delta else 2
    offc = off[: nu + 1].cpu().numpy()
    kr, qr = int(offc[-1]), (nu * delta if delta else int(offc[-1]))
    def deq(x8, ds, o):   # x8 * descale in fp64, rows of the first nu users
        rows_ds = torch.repeat_interleave(ds[:nu], o[1:nu + 1] - o[:nu], dim=0)
        return x8[: int(o[nu])].double() * rows_ds[:, :, None].double()

    exact = [deq(q8, qd, qoff), deq(k8, kd, off), deq(v8, vd, off)]
    rounded = [qb[:qr].double(), kb[:kr].double(), vb[:kr].double()]
    oracle_err = {}
    for tag, inp, got in (("fp8", exact, o8), ("bf16", rounded, ob)):
        qn, kn, vn = (t.cpu().numpy() for t in inp)
        ref = O.delta_hstu_mha_fwd(N, alpha, qn, kn, vn, offc) if delta else O.hstu_mha_fwd(N, alpha, qn, kn, vn, offc)
        g = got[:qr].double().cpu().numpy()
        oracle_err[tag] = float(np.linalg.norm(g - ref) / np.linalg.norm(ref))
    for _ in range(3):
        bf16(), f8()
    tb, t8 = [], []
    for _ in range(rounds):
        tb.append(_events_ms(bf16, iters))
        t8.append(_events_ms(f8, iters))
    mb, m8 = statistics.median(tb), statistics.median(t8)
    out_bytes = qrows * H * d * 2
    bytes_bf16 = (qrows + 2 * rows) * H * d * 2 + out_bytes
    bytes_fp8 = (qrows + 2 * rows) * H * d * 1 + out_bytes
    return {
        "shape": {"users": B, "max_seq_len": N, "heads": H, "head_dim": d, "rows": rows, "q_rows": qrows, "delta_q": delta},
        "fwd_ms": {"bf16": round(mb, 4), "fp8": round(m8, 4)},
        "fwd_ms_rounds": {"bf16": [round(x, 4) for x in tb], "fp8": [round(x, 4) for x in t8]},
        "fp8_speedup": round(mb / m8, 3),
        "bytes": {"bf16": bytes_bf16, "fp8": bytes_fp8},
        "frac_of_8TBps": {"bf16": round(bytes_bf16 / (mb * 1e-3) / PEAK_HBM, 3), "fp8": round(bytes_fp8 / (m8 * 1e-3) / PEAK_HBM, 3)},
        "quantizer_GBps": round(quant_gbps, 1),
        "fp8_vs_bf16_rel_fro": rel,
        "rel_fro_vs_fp64_oracle": dict(oracle_err, users=nu),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="M-full,M-jag,C5-delta")
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "workloads": {}}
    for name in args.shapes.split(","):
        res["workloads"][name] = run(name, args.iters, args.rounds, gen)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
