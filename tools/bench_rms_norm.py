#!/usr/bin/env python3
"""RMS norm next to layer norm and the torch composition, alternating in ONE process:

    python tools/bench_rms_norm.py [--rounds 5] [--launches 10] [--out profiles/rms_norm_bench.json]

Per shape -- 204,800 x 512 and 204,800 x 1024 in bf16, 131,072 x 512 in fp32 -- forward and backward of
  rms_norm     this package's RMS kernels (_launch.rms_norm_fwd / rms_norm_bwd)
  layer_norm   this package's layer norm kernels at the same shape (_launch.layer_norm_fwd / layer_norm_bwd)
  torch        (x.float() * rsqrt(x.float().pow(2).mean(-1, True) + eps)).type_as(x) * w under autograd
are timed with HIP events, `--launches` calls per measurement, the three candidates taking turns inside every round; the
figure reported is the median over the rounds, with the smallest and the largest next to it (the alternating runs' own
spread), and the algorithmic HBM rate.  The result goes to a JSON file under profiles/.  No figure is a pass / fail condition."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from generative_recommenders_amd.ops import _launch  # noqa: E402

EPS = 1e-5
SHAPES = [(204800, 512, torch.bfloat16), (204800, 1024, torch.bfloat16), (131072, 512, torch.float32)]


def _timed(fn, launches):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3      # us


def bench_shape(rows, dim, dtype, rounds, launches):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(rows, dim, device=dev, dtype=dtype, generator=gen)
    dy = torch.randn(rows, dim, device=dev, dtype=dtype, generator=gen)
    w = 1 + 0.1 * torch.randn(dim, device=dev, dtype=dtype, generator=gen)
    b = 0.1 * torch.randn(dim, device=dev, dtype=dtype, generator=gen)
    _, rstd = _launch.rms_norm_fwd(x, w, EPS)
    _, mean, lrstd = _launch.layer_norm_fwd(x, w, b, EPS)
    xt, wt = x.clone().requires_grad_(), w.clone().requires_grad_()

    def torch_fwd():
        xf = xt.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, True) + EPS)).type_as(xt) * wt

    yt = torch_fwd()

    def torch_bwd():
        torch.autograd.grad(yt, (xt, wt), dy, retain_graph=True)

    es = x.element_size()
    calls = {
        # name -> (callable, bytes that must cross HBM: rows read + rows written; parameters and statistics are noise)
        "rms_norm_fwd": (lambda: _launch.rms_norm_fwd(x, w, EPS), 2 * rows * dim * es),
        "layer_norm_fwd": (lambda: _launch.layer_norm_fwd(x, w, b, EPS), 2 * rows * dim * es),
        "torch_fwd": (lambda: torch_fwd(), 2 * rows * dim * es),
        "rms_norm_bwd": (lambda: _launch.rms_norm_bwd(dy, x, w, rstd), 3 * rows * dim * es),
        "layer_norm_bwd": (lambda: _launch.layer_norm_bwd(dy, x, w, mean, lrstd), 3 * rows * dim * es),
        "torch_bwd": (torch_bwd, 3 * rows * dim * es),
    }
    times = {n: [] for n in calls}
    for r in range(rounds + 1):             # round 0 warms up
        for n, (fn, _) in calls.items():
            t = _timed(fn, launches)
            if r:
                times[n].append(t)
    res = {}
    for n, (_, nbytes) in calls.items():
        med = statistics.median(times[n])
        res[n] = dict(median_us=round(med, 2), min_us=round(min(times[n]), 2), max_us=round(max(times[n]), 2),
                      algorithmic_tb_per_s=round(nbytes / med / 1e6, 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rms_norm_bench.json"))
    a = ap.parse_args()
    if a.rounds < 3:
        raise SystemExit("--rounds must be at least 3 (the figure is a median)")
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, launches=a.launches, eps=EPS, shapes=[])
    for rows, dim, dtype in SHAPES:
        res = bench_shape(rows, dim, dtype, a.rounds, a.launches)
        out["shapes"].append(dict(rows=rows, dim=dim, dtype=str(dtype).replace("torch.", ""), results=res))
        for n, v in res.items():
            print(f"{rows:7d} x {dim:4d} {str(dtype).replace('torch.', ''):8s} {n:15s} {v['median_us']:9.1f} us  [{v['min_us']:.1f} .. {v['max_us']:.1f}]"
                  f"  {v['algorithmic_tb_per_s']:.2f} TB/s")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
