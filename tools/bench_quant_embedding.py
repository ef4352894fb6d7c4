"""Times the int8 row-wise dequantizing gather (hstu_gather_rows_int8) beside torch's index_select on the fp32 and the fp16
table, and the quantize pass (hstu_quantize_rows_int8): the lookup of the DLRM-v3 serving path.

    python tools/bench_quant_embedding.py [--out profiles/quant_embedding_bench.json] [--reps 30] [--small]

8192 x 200 ids into tables of 1 M and 10 M rows x 192 and x 256 columns, ids drawn Zipf (exponent 1, hot rows scattered over
the table) and uniform.  The variants of one shape alternate inside one process, one call per variant per repetition, each
call between two HIP events; the figure is the median.  GB/s is ALGORITHMIC: n * (bytes of a table row + bytes of an output
row) over the time -- a Zipf draw re-reads hot rows from cache, so it can exceed what HBM delivers; the fraction is of the
8 TB/s HBM peak.  Needs a GPU: there is no fallback."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.ops.quant_embedding import gather_rows_int8, int8_row_stride, quantize_rows_int8  # noqa: E402

HBM_PEAK = 8.0e12


def draw_ids(rows: int, n: int, how: str, gen: torch.Generator) -> torch.Tensor:
    if how == "uniform":
        return torch.randint(0, rows, (n,), generator=gen, device="cuda")
    # Zipf with exponent 1: rank = rows ** u is log-uniform; a fixed odd multiplier scatters the ranks over the table
    rank = (float(rows) ** torch.rand(n, generator=gen, device="cuda", dtype=torch.float64)).long().clamp_(1, rows) - 1
    return (rank * 2654435761) % rows


def time_alternating(variants, reps: int, warmup: int = 3):
    """variants: name -> callable.  One call per variant per repetition, in turn; name -> median milliseconds"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end))
    return {name: statistics.median(t) for name, t in times.items()}, {name: (min(t), max(t)) for name, t in times.items()}


def row(what, ms, lo_hi, nbytes, **extra):
    gbs = nbytes / (ms * 1e-3) / 1e9
    return dict(what=what, ms=round(ms, 4), ms_min=round(lo_hi[0], 4), ms_max=round(lo_hi[1], 4), algorithmic_gb_s=round(gbs, 1),
                fraction_of_8_tb_s=round(gbs * 1e9 / HBM_PEAK, 3), **extra)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="quant_embedding_bench.json")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--small", action="store_true", help="a toy size, to rehearse the script")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quant_embedding needs a GPU")
    n = 64 * 20 if args.small else 8192 * 200
    table_rows = (1000, 5000) if args.small else (1_000_000, 10_000_000)
    gen = torch.Generator(device="cuda").manual_seed(0)
    results = []
    for rows in table_rows:
        for dim in (192, 256):
            w32 = torch.randn(rows, dim, device="cuda", generator=gen)
            w16 = w32.to(torch.float16)
            stride = int8_row_stride(dim)
            shape = dict(table_rows=rows, dim=dim, n=n)
            q = quantize_rows_int8(w32)
            med, span = time_alternating({"quantize fp32 table": lambda: quantize_rows_int8(w32),
                                          "quantize fp16 table": lambda: quantize_rows_int8(w16)}, max(5, args.reps // 3))
            results.append(row("quantize fp32 table", med["quantize fp32 table"], span["quantize fp32 table"], rows * (4 * dim + stride), **shape))
            results.append(row("quantize fp16 table", med["quantize fp16 table"], span["quantize fp16 table"], rows * (2 * dim + stride), **shape))
            for how in ("zipf", "uniform"):
                ids = draw_ids(rows, n, how, gen)
                out32 = torch.empty(n, dim, device="cuda")
                out16 = torch.empty(n, dim, device="cuda", dtype=torch.bfloat16)
                o32 = torch.empty(n, dim, device="cuda")
                o16 = torch.empty(n, dim, device="cuda", dtype=torch.float16)
                variants = {
                    "int8 gather -> fp32": lambda: gather_rows_int8(q, dim, ids, torch.float32, out=out32),
                    "int8 gather -> bf16": lambda: gather_rows_int8(q, dim, ids, torch.bfloat16, out=out16),
                    "index_select fp32 table": lambda: torch.index_select(w32, 0, ids, out=o32),
                    "index_select fp16 table": lambda: torch.index_select(w16, 0, ids, out=o16),
                }
                nbytes = {"int8 gather -> fp32": n * (stride + 4 * dim), "int8 gather -> bf16": n * (stride + 2 * dim),
                          "index_select fp32 table": n * 8 * dim, "index_select fp16 table": n * 4 * dim}
                med, span = time_alternating(variants, args.reps)
                for name in variants:
                    results.append(row(name, med[name], span[name], nbytes[name], ids=how, **shape))
                    print(json.dumps(results[-1]), flush=True)
            del w32, w16, q
            torch.cuda.empty_cache()
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, timing="HIP events around one call, variants alternating, median",
               bytes_model="n * (table row bytes + output row bytes); int8 table row = int8_row_stride(dim)", results=results)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
