"""Time the fused LayerNorm + UVQK projection kernel (csrc/hstu_ln_linear.cuh) against what it replaces
(hstu_layer_norm_fwd + hipBLASLt through torch) at the layer section's shape; HIP events, one JSON line.
    python tools/bench_ln_linear.py [--rows 204800] [--n 2048] [--iters 20]
    python tools/bench_ln_linear.py --fp8 [--rounds 7] [--out FILE]     the row-wise e4m3 kernel against the bf16 one"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from generative_recommenders_amd.ops import _launch  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=204800)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fused-only", action="store_true", help="time the fused kernel only (variant libraries: HSTU_HIP_LIBRARY)")
    ap.add_argument("--k512", action="store_true", help="the kernel without its LayerNorm (hstu_linear_k512) against torch.mm at the output "
                    "stage's data-gradient shape: d y = d out . W_out^T, rows x 512 -> n (default n for this mode: 1536)")
    ap.add_argument("--fp8", action="store_true", help="the row-wise e4m3 kernel (hstu_ln_linear_fp8_fwd) against the bf16 fused kernel, layer "
                    "norm + hipBLASLt, and layer norm + row quantizer + hstu_linear_fp8_rowwise: alternating rounds in one process")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="--fp8: also write the result line to this file")
    a = ap.parse_args()
    dev, dt, k = "cuda", torch.bfloat16, 512
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(a.rows, k, device=dev, generator=g).to(dt)
    lw = (1 + 0.1 * torch.randn(k, device=dev, generator=g)).to(dt)
    lb = (0.1 * torch.randn(k, device=dev, generator=g)).to(dt)
    w_nk = (torch.randn(a.n, k, device=dev, generator=g) / k**0.5).to(dt)
    b = (0.1 * torch.randn(a.n, device=dev, generator=g)).to(dt)
    if a.k512 and a.n == 2048:
        a.n = 1536
    flops = 2.0 * a.rows * k * a.n
    if a.k512:
        w_out = (torch.randn(a.n, k, device=dev, generator=g) / k**0.5).to(dt)     # `_output_weight` as stored: (3 H d, D)
        res = {"rows": a.rows, "k": k, "n": a.n, "dtype": "bf16", "what": "d y = d out . W_out^T"}
        for _ in range(40):
            _launch.linear_k512(x, w_out)
        res["hipblaslt_mm_us"] = timed(lambda: torch.mm(x, w_out.t()), a.iters)
        res["linear_k512_us"] = timed(lambda: _launch.linear_k512(x, w_out), a.iters)
        for key in ("hipblaslt_mm_us", "linear_k512_us"):
            res[key.replace("_us", "_tflops")] = round(flops / res[key] / 1e6, 1)
        res["bit_identical"] = bool(torch.equal(_launch.linear_k512(x, w_out), torch.mm(x, w_out.t())))
        print(json.dumps({k_: (round(v, 2) if isinstance(v, float) else v) for k_, v in res.items()}))
        return

    def unfused():
        nx, _, _ = _launch.layer_norm_fwd(x, lw, lb, 1e-6)
        return torch.nn.functional.linear(nx, w_nk, b)

    if a.fp8:
        wq, ws = _launch.quantize_rows_fp8(w_nk)

        def unfused_fp8():
            nx, _, _ = _launch.layer_norm_fwd(x, lw, lb, 1e-6)
            xq, xs = _launch.quantize_rows_fp8(nx)
            return _launch.linear_fp8_rowwise(xq, xs, wq, ws, b, out_dtype=dt)

        xq0, xs0 = _launch.quantize_rows_fp8(_launch.layer_norm_fwd(x, lw, lb, 1e-6)[0])
        cands = {
            "fp8_fused_us": lambda: _launch.ln_linear_fp8_fwd(x, lw, lb, 1e-6, wq, ws, b),
            "bf16_fused_us": lambda: _launch.ln_linear_fwd(x, lw, lb, 1e-6, w_nk, b),
            "ln_hipblaslt_us": unfused,
            "ln_quant_fp8_linear_us": unfused_fp8,
            "fp8_linear_only_us": lambda: _launch.linear_fp8_rowwise(xq0, xs0, wq, ws, b, out_dtype=dt),
            "fp8_fused_with_codes_us": lambda: _launch.ln_linear_fp8_fwd(x, lw, lb, 1e-6, wq, ws, b, want_q=True),
            "quantize_weight_us": lambda: _launch.quantize_rows_fp8(w_nk),
        }
        for _ in range(25):          # every shape of the timed window, and ~50 ms of work for the clocks
            for fn in cands.values():
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in cands}
        for _ in range(a.rounds):    # alternating: a drift of the clocks or a neighbour on the host hits every candidate alike
            for name, fn in cands.items():
                samples[name].append(timed(fn, a.iters))
        res = {"rows": a.rows, "k": k, "n": a.n, "dtype": "bf16", "rounds": a.rounds, "iters": a.iters,
               "lib": os.path.basename(os.environ.get("HSTU_HIP_LIBRARY", "libhstu_hip.so"))}
        for name, v in samples.items():
            v = sorted(v)
            res[name] = round(v[len(v) // 2], 2)
            res[name.replace("_us", "_min_max")] = [round(v[0], 2), round(v[-1], 2)]
        res["fp8_over_bf16_fused"] = round(res["fp8_fused_us"] / res["bf16_fused_us"], 4)
        res["fp8_fused_tflops"] = round(flops / res["fp8_fused_us"] / 1e6, 1)
        res["bf16_fused_tflops"] = round(flops / res["bf16_fused_us"] / 1e6, 1)
        y8 = _launch.ln_linear_fp8_fwd(x, lw, lb, 1e-6, wq, ws, b)[0].float()
        y16 = _launch.ln_linear_fwd(x, lw, lb, 1e-6, w_nk, b)[0].float()
        res["rel_fro_fp8_vs_bf16_fused"] = float((y8 - y16).norm() / y16.norm())
        res["plain_entry_bit_identical"] = bool(torch.equal(unfused_fp8().float(), unfused_fp8().float()))
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        return

    res = {"rows": a.rows, "k": k, "n": a.n, "dtype": "bf16", "lib": os.path.basename(os.environ.get("HSTU_HIP_LIBRARY", "libhstu_hip.so"))}
    if a.fused_only:
        for _ in range(60):      # ~30 ms of the same kernel first: the clocks of a cold device ramp for tens of milliseconds
            _launch.ln_linear_fwd(x, lw, lb, 1e-6, w_nk, b)
        res["fused_us"] = round(timed(lambda: _launch.ln_linear_fwd(x, lw, lb, 1e-6, w_nk, b), a.iters), 2)
        res["fused_tflops"] = round(flops / res["fused_us"] / 1e6, 1)
        print(json.dumps(res))
        return
    nx, _, _ = _launch.layer_norm_fwd(x, lw, lb, 1e-6)
    res["layer_norm_us"] = timed(lambda: _launch.layer_norm_fwd(x, lw, lb, 1e-6), a.iters)
    res["hipblaslt_linear_us"] = timed(lambda: torch.nn.functional.linear(nx, w_nk, b), a.iters)
    res["unfused_us"] = timed(unfused, a.iters)
    res["fused_us"] = timed(lambda: _launch.ln_linear_fwd(x, lw, lb, 1e-6, w_nk, b), a.iters)
    res["fused_with_normed_us"] = timed(lambda: _launch.ln_linear_fwd(x, lw, lb, 1e-6, w_nk, b, want_normed=True), a.iters)
    for key in ("hipblaslt_linear_us", "unfused_us", "fused_us", "fused_with_normed_us"):
        res[key.replace("_us", "_tflops")] = round(flops / res[key] / 1e6, 1)
    y, _, _, _ = _launch.ln_linear_fwd(x, lw, lb, 1e-6, w_nk, b)
    ref = unfused()
    res["rel_fro_vs_unfused"] = float((y.float() - ref.float()).norm() / ref.float().norm())
    res["max_abs_vs_unfused"] = float((y.float() - ref.float()).abs().max())
    print(json.dumps({k_: (round(v, 2) if isinstance(v, float) and v > 1 else v) for k_, v in res.items()}))


if __name__ == "__main__":
    main()
