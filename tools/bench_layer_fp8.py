"""The three-layer STU step of bench.py's `layer` section (3 x STULayer, D = 512, 4 heads of 128, group norm, bf16
activations, fp32 masters, 1024 users of 180-199 items, forward + backward, reference recompute flags) with
STULayerConfig.fp8_in_addmm_fwd on and off: alternating rounds in one process, HIP events, one JSON line.  No gradient
all-reduce (bench.py's own number includes it).
    python tools/bench_layer_fp8.py [--users 1024] [--steps 10] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from generative_recommenders_amd.modules.stu import STULayer, STULayerConfig, STUStack  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev, N, H, d = "cuda", 200, 4, 128
    D = H * d
    gen = torch.Generator(device=dev).manual_seed(2002)
    lengths = torch.randint(int(0.9 * N), N, (a.users,), generator=gen, device=dev, dtype=torch.int64)
    off = torch.zeros(a.users + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lengths, 0)
    L = int(off[-1].item())
    x = torch.randn(L, D, device=dev, dtype=torch.bfloat16, generator=gen).requires_grad_()
    gy = torch.randn(L, D, device=dev, dtype=torch.bfloat16, generator=gen)
    nt = torch.minimum(torch.randint(1, 21, (a.users,), generator=gen, device=dev), lengths)

    def make(fp8):
        torch.manual_seed(7)
        stack = STUStack([STULayer(STULayerConfig(embedding_dim=D, num_heads=H, hidden_dim=d, attention_dim=d, output_dropout_ratio=0.0,
                                                  use_group_norm=True, fp8_in_addmm_fwd=fp8)) for _ in range(3)]).to(dev).train()

        def step():
            for p in stack.parameters():
                p.grad = None
            x.grad = None
            y = stack(x=x, x_lengths=lengths, x_offsets=off, max_seq_len=N, num_targets=nt)
            y.backward(gy)
            return y

        return step

    steps = {"fp8_off_ms": make(False), "fp8_on_ms": make(True)}
    outs = {}
    for _ in range(10):            # pre-warm: every kernel and library algorithm of the timed window, ~0.3 s of work
        for name, fn in steps.items():
            outs[name] = fn().detach().float()
    torch.cuda.synchronize()
    samples = {name: [] for name in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[name].append(e0.elapsed_time(e1) / a.steps)
    res = {"users": a.users, "rows": L, "layers": 3, "steps": a.steps, "rounds": a.rounds}
    for name, v in samples.items():
        v = sorted(v)
        res[name] = round(v[len(v) // 2], 4)
        res[name.replace("_ms", "_min_max")] = [round(v[0], 4), round(v[-1], 4)]
    res["on_over_off"] = round(res["fp8_on_ms"] / res["fp8_off_ms"], 4)
    res["out_rel_fro_on_vs_off"] = float((outs["fp8_on_ms"] - outs["fp8_off_ms"]).norm() / outs["fp8_off_ms"].norm())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
