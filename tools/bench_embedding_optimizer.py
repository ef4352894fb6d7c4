#!/usr/bin/env python3
"""In-backward sparse row-wise Adagrad on one MI355X: the fused step (ops/embedding.py: sort, one pass over the batch's gradient
rows and the touched table rows, one pass that combines the runs cut by a chunk boundary) against what the package did for the
same ids before it existed -- the dense table gradient of ``_table_grad`` (memset + segment sum over the whole table) followed
by the same formula over the dense table in torch ops.  One JSON object on stdout, and in --out.

bf16 gradient rows, dim 256, Zipf ids scattered over the table:
    1 M rows,  n = 65,536 and n = 1,638,400: both paths (the dense gradient and the dense update fit at this size);
    10 M rows (the reference's HASH_SIZE), the same two n: the fused path alone (the dense path's temporaries would be 10 GB each).
Both paths run in ONE process on the same inputs, timed with HIP events after a warm-up, alternating fused / dense rounds; the
median per call is reported.  The state keeps changing from call to call (the step is in place), which changes no address and
no amount of work.  Bytes are algorithmic: n * dim * sizeof(dout) + unique * (2 * dim * 4 + 8) -- every gradient row read
once, every touched table row and its state read and written once; GB/s is those bytes over the time, share_of_8TBs the
same over 8 TB/s.

--replicated W times the data-parallel path for tables replicated on W ranks instead, the ranks emulated on the one GPU: the
batch is cut into W equal shards, every shard is coalesced to one fp32 row per distinct id with scale 1 / W
(``coalesce_row_gradients``), the W lists are concatenated in rank order and applied with the same update.  What one rank
does per step -- coalesce ITS shard, then the merged update -- is timed against the one-shot update of the whole batch and of
one shard, all in one process, alternating.  ``sent_bytes`` is what a rank puts on the wire, u * (4 + 4 * dim) for its u
distinct ids, beside the raw alternative n / W * (4 + es * dim); the exchange itself is not timed (one GPU).

--table-dtype fp16 | bf16 times the update of a table stored in 16 bits (the fp32 update of the widened row, written back by
stochastic rounding) against the fp32 table's, the two alternating in one process on the same ids and gradient rows.  The
16-bit table's algorithmic bytes: n * dim * sizeof(dout) + unique * (2 * dim * 2 + 8).

--optimizer adam | sgd times the in-backward sparse Adam / SGD the same way (same shapes, same method).  Their dense path is
``_table_grad`` followed by ``torch.optim.Adam`` / ``torch.optim.SGD`` over the whole table (dense Adam also decays the
moments of rows outside the batch, so only the first step from zero state is compared).  Algorithmic bytes: Adam
n * dim * sizeof(dout) + unique * (6 * dim * 4 + 8) -- the table row and both moment rows read and written --, SGD
n * dim * sizeof(dout) + unique * 2 * dim * 4.

    python tools/bench_embedding_optimizer.py [--iters 10] [--rounds 7] [--out profiles/r15_bench_embedding_optimizer.json]
    python tools/bench_embedding_optimizer.py --replicated 8 --out profiles/r17_bench_embedding_replicated.json
    python tools/bench_embedding_optimizer.py --table-dtype fp16 --out profiles/r18_bench_embedding_lowp_fp16.json
    python tools/bench_embedding_optimizer.py --optimizer adam --out profiles/r19_bench_embedding_adam.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.ops.embedding import (coalesce_row_gradients, rowwise_adagrad_update_, sparse_adam_update_,  # noqa: E402
                                                       sparse_sgd_update_)
from generative_recommenders_amd.ops.position import _table_grad  # noqa: E402

DEV = "cuda"
DIM, LR, EPS, BETAS = 256, 0.01, 1e-8, (0.9, 0.999)
# name: (table rows, n, time the dense path too)
SHAPES = {"1Mx256_n65536": (1_000_000, 65_536, True), "1Mx256_n1638400": (1_000_000, 1_638_400, True),
          "10Mx256_n65536": (10_000_000, 65_536, False), "10Mx256_n1638400": (10_000_000, 1_638_400, False)}


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def _zipf_ids(rows, n, g):
    """rank r with probability ~ 1 / (r + 1); the ranks scattered over the table"""
    p = 1.0 / torch.arange(1, rows + 1, dtype=torch.float32, device=DEV)
    cdf = torch.cumsum(p.double(), 0)
    ranks = torch.searchsorted(cdf, torch.rand(n, device=DEV, generator=g, dtype=torch.float64) * cdf[-1]).clamp_(max=rows - 1)
    return ((ranks * 2_654_435_761) % rows).to(torch.int64)       # a fixed odd multiplier: hot ranks land far apart


def _dense_step(weight, momentum1, idx32, dout):
    """the parent's path for the same ids: the dense (rows, dim) fp32 gradient, then the formula over the whole table (rows
    outside the batch have a zero gradient row: their state and weights keep their values)"""
    grad = _table_grad(dout, idx32, weight.shape[0])
    momentum1.add_(grad.pow(2).mean(dim=1))
    weight.addcdiv_(grad, (momentum1.sqrt() + EPS).unsqueeze(1), value=-LR)


def run_adam_sgd(rows, n, dense, iters, rounds, optimizer):
    """the fused sparse Adam / SGD step against _table_grad + torch.optim.Adam / SGD over the whole table"""
    g = torch.Generator(device=DEV).manual_seed(0)
    idx = _zipf_ids(rows, n, g)
    idx32 = idx.to(torch.int32)
    counts = torch.bincount(idx, minlength=1)
    unique = int((counts > 0).sum())
    res = {"optimizer": optimizer, "shape": {"table_rows": rows, "dim": DIM, "n": n, "unique_ids": unique,
                                             "largest_multiplicity": int(counts.max()), "dout": "bfloat16"}}
    del counts
    dout = (0.01 * torch.randn(n, DIM, device=DEV, generator=g)).to(torch.bfloat16)
    weight = torch.randn(rows, DIM, device=DEV, generator=g)
    step = [0]
    if optimizer == "adam":
        exp_avg, exp_avg_sq = torch.zeros_like(weight), torch.zeros_like(weight)

        def fused():
            sparse_adam_update_(weight, exp_avg, exp_avg_sq, idx32, dout, LR, BETAS, EPS, step[0])
            step[0] += 1
    else:
        fused = lambda: sparse_sgd_update_(weight, idx32, dout, LR)
    paths = {"fused": fused}
    if dense:
        p2 = torch.nn.Parameter(weight.clone())
        opt = torch.optim.Adam([p2], lr=LR, betas=BETAS, eps=EPS) if optimizer == "adam" else torch.optim.SGD([p2], lr=LR)

        def dense_step():
            p2.grad = _table_grad(dout, idx32, rows)
            opt.step()

        paths["dense"] = dense_step
        for fn in paths.values():                                  # one step each from the same (zero) state: the results to compare
            fn()
        res["max_abs_diff_after_one_step"] = {"weight": float((weight - p2.detach()).abs().max())}
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            times[name].append(_events_ms(fn, iters))
    alg_bytes = n * DIM * dout.element_size() + unique * ((6 * DIM * 4 + 8) if optimizer == "adam" else 2 * DIM * 4)
    res["algorithmic_bytes"] = alg_bytes
    res["us"] = {k: round(1e3 * statistics.median(v), 2) for k, v in times.items()}
    res["us_rounds"] = {k: [round(1e3 * x, 2) for x in v] for k, v in times.items()}
    res["GBps"] = {k: round(alg_bytes / (1e-3 * statistics.median(v)) / 1e9, 1) for k, v in times.items()}
    res["share_of_8TBs"] = {k: round(alg_bytes / (1e-3 * statistics.median(v)) / 8e12, 4) for k, v in times.items()}
    if dense:
        res["dense_over_fused"] = round(statistics.median(times["dense"]) / statistics.median(times["fused"]), 2)
    return res


def run(rows, n, dense, iters, rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    idx = _zipf_ids(rows, n, g)
    idx32 = idx.to(torch.int32)
    counts = torch.bincount(idx, minlength=1)
    unique = int((counts > 0).sum())
    dout = (0.01 * torch.randn(n, DIM, device=DEV, generator=g)).to(torch.bfloat16)
    weight = torch.randn(rows, DIM, device=DEV, generator=g)
    momentum1 = torch.zeros(rows, device=DEV)
    paths = {"fused": lambda: rowwise_adagrad_update_(weight, momentum1, idx32, dout, LR, EPS)}
    res = {"shape": {"table_rows": rows, "dim": DIM, "n": n, "unique_ids": unique, "largest_multiplicity": int(counts.max()),
                     "dout": "bfloat16"}}
    del counts
    if dense:
        w2, m2 = weight.clone(), momentum1.clone()
        paths["dense"] = lambda: _dense_step(w2, m2, idx32, dout)
        for fn in paths.values():                                  # one step each from the same state: the results to compare
            fn()
        res["max_abs_diff_after_one_step"] = {"weight": float((weight - w2).abs().max()), "momentum1": float((momentum1 - m2).abs().max())}
    for fn in paths.values():                                      # warm-up of every shape of the timed window
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            times[name].append(_events_ms(fn, iters))
    alg_bytes = n * DIM * dout.element_size() + unique * (2 * DIM * 4 + 8)
    res["algorithmic_bytes"] = alg_bytes
    res["us"] = {k: round(1e3 * statistics.median(v), 2) for k, v in times.items()}
    res["us_rounds"] = {k: [round(1e3 * x, 2) for x in v] for k, v in times.items()}
    res["GBps"] = {k: round(alg_bytes / (1e-3 * statistics.median(v)) / 1e9, 1) for k, v in times.items()}
    res["share_of_8TBs"] = {k: round(alg_bytes / (1e-3 * statistics.median(v)) / 8e12, 4) for k, v in times.items()}
    if dense:
        res["dense_over_fused"] = round(statistics.median(times["dense"]) / statistics.median(times["fused"]), 2)
    return res


def run_lowp(rows, n, table_dtype, iters, rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    idx = _zipf_ids(rows, n, g)
    idx32 = idx.to(torch.int32)
    unique = int((torch.bincount(idx, minlength=1) > 0).sum())
    dout = (0.01 * torch.randn(n, DIM, device=DEV, generator=g)).to(torch.bfloat16)
    w32 = torch.randn(rows, DIM, device=DEV, generator=g)
    w16 = w32.to(table_dtype)
    m32, m16 = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
    step = [0]

    def lowp():
        step[0] += 1                                               # a fresh seed per call, as in training
        rowwise_adagrad_update_(w16, m16, idx32, dout, LR, EPS, seed=step[0])

    name16 = str(table_dtype).replace("torch.", "")
    paths = {"float32": lambda: rowwise_adagrad_update_(w32, m32, idx32, dout, LR, EPS), name16: lowp}
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            times[name].append(_events_ms(fn, iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    alg = {"float32": n * DIM * dout.element_size() + unique * (2 * DIM * 4 + 8), name16: n * DIM * dout.element_size() + unique * (2 * DIM * 2 + 8)}
    return {"shape": {"table_rows": rows, "dim": DIM, "n": n, "unique_ids": unique, "dout": "bfloat16", "table": name16},
            "algorithmic_bytes": alg,
            "us": {k: round(1e3 * v, 2) for k, v in med.items()},
            "us_rounds": {k: [round(1e3 * x, 2) for x in v] for k, v in times.items()},
            "GBps": {k: round(alg[k] / (1e-3 * med[k]) / 1e9, 1) for k in med},
            "lowp_over_float32": round(med[name16] / med["float32"], 3),
            "lowp_over_float32_rounds": [round(a / b, 3) for a, b in zip(times[name16], times["float32"])]}


def run_replicated(rows, n, world, iters, rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    idx32 = _zipf_ids(rows, n, g).to(torch.int32)
    dout = (0.01 * torch.randn(n, DIM, device=DEV, generator=g)).to(torch.bfloat16)
    weight = torch.randn(rows, DIM, device=DEV, generator=g)
    momentum1 = torch.zeros(rows, device=DEV)
    per = (n + world - 1) // world
    shards = [(idx32[r * per:(r + 1) * per], dout[r * per:(r + 1) * per]) for r in range(world)]
    lists = []
    for i, d in shards:
        r, G, count = coalesce_row_gradients(i, d, rows, 1.0 / world)
        u = int(count)
        lists.append((r[:u], G[:u]))
    rows_all, G_all = torch.cat([l[0] for l in lists]), torch.cat([l[1] for l in lists])
    i0, d0 = shards[0]
    paths = {"one_shot_whole_batch": lambda: rowwise_adagrad_update_(weight, momentum1, idx32, dout, LR, EPS),
             "one_shot_one_shard": lambda: rowwise_adagrad_update_(weight, momentum1, i0, d0, LR, EPS),
             "coalesce_one_shard": lambda: coalesce_row_gradients(i0, d0, rows, 1.0 / world),
             "merged_update": lambda: rowwise_adagrad_update_(weight, momentum1, rows_all, G_all, LR, EPS)}
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            times[name].append(_events_ms(fn, iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    u0, es = int(lists[0][0].numel()), dout.element_size()
    return {"shape": {"table_rows": rows, "dim": DIM, "n": n, "world": world, "shard_n": int(i0.numel()), "shard_unique_ids": u0,
                      "merged_rows": int(rows_all.numel()), "unique_ids": int(torch.unique(idx32).numel()), "dout": "bfloat16"},
            "us": {k: round(1e3 * v, 2) for k, v in med.items()},
            "us_rounds": {k: [round(1e3 * x, 2) for x in v] for k, v in times.items()},
            "rank_step_over_one_shot_whole_batch": round((med["coalesce_one_shard"] + med["merged_update"]) / med["one_shot_whole_batch"], 3),
            "rank_step_over_one_shot_one_shard": round((med["coalesce_one_shard"] + med["merged_update"]) / med["one_shot_one_shard"], 3),
            "sent_bytes": {"coalesced": u0 * (4 + 4 * DIM), "raw": int(i0.numel()) * (4 + es * DIM)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--replicated", type=int, default=0, metavar="W", help="time the replicated-table path with W emulated ranks")
    ap.add_argument("--table-dtype", choices=["fp32", "fp16", "bf16"], default="fp32",
                    help="fp16 / bf16: time the 16-bit table's update against the fp32 table's, alternating in one process")
    ap.add_argument("--optimizer", choices=["adagrad", "adam", "sgd"], default="adagrad",
                    help="adam / sgd: time the sparse Adam / SGD step against _table_grad + torch.optim.Adam / SGD (fp32 tables)")
    args = ap.parse_args()
    if args.optimizer != "adagrad" and (args.replicated > 0 or args.table_dtype != "fp32"):
        raise SystemExit("bench_embedding_optimizer: --optimizer adam | sgd times the fp32 one-shot step only")
    if not torch.cuda.is_available():
        raise SystemExit("bench_embedding_optimizer: needs a GPU (a timing without one says nothing)")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "workloads": {}}
    for name in args.shapes.split(","):
        if args.optimizer != "adagrad":
            res["workloads"][name] = run_adam_sgd(*SHAPES[name], args.iters, args.rounds, args.optimizer)
        elif args.table_dtype != "fp32":
            res["workloads"][name] = run_lowp(*SHAPES[name][:2], {"fp16": torch.float16, "bf16": torch.bfloat16}[args.table_dtype],
                                              args.iters, args.rounds)
        elif args.replicated > 0:
            res["workloads"][name] = run_replicated(*SHAPES[name][:2], args.replicated, args.iters, args.rounds)
        else:
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
