#!/usr/bin/env python3
"""The two fused input-preprocessor ops against the reference's composition built from this package's existing ops, on one
MI355X: one JSON object on stdout (and, with --out, in a file).

Shape (the DLRM-v3 debug shape): 1024 users, N = 200 with M-jag lengths (randint(180, 200)), num_targets = randint(1, 21),
D = 512 in bf16, T * Da = 8 * 32 (five action weights + three watchtime thresholds), C = 3 contextual rows.  Timed, forward
and forward + backward, in the same process and alternating round by round:

* ``action_encode`` against modules/action_encoder.py:73-112 as the reference runs it: torch bit ops, the broadcast
  multiply, ``tile``, this package's ``concat_2D_jagged`` and the cast to bf16;
* ``combine_embeddings`` in its three modes against modules/contextual_interleave_preprocessor.py:101-224: ``stack``, the mask
  path (``dense_to_jagged`` + boolean indexing, a host sync) and two ``concat_2D_jagged`` (embeddings and timestamps).

HIP events after a pre-warm and a warm-up; the median of the rounds is reported, every round is kept.  The fused results
are compared with the composition's (``torch.equal``) before anything is timed.

Bytes are algorithmic (s = 2): combine moves every source row it reads and every output row it writes once, D * s bytes
each, plus 8 bytes per timestamp -- for the interleave that is 2 reads + 2 writes of (sum L, D); the backward moves the
same rows the other way.  The encoder writes (sum L, T * Da) once (forward) or reads it once (backward).  Both ops are
HBM-bound; the line gives ms and the fraction of 8 TB/s.

    python tools/bench_preprocessor.py [--iters 20] [--rounds 7] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generative_recommenders_amd.ops.jagged_tensors import (  # noqa: E402
    asynchronous_complete_cumsum,
    concat_2D_jagged,
    dense_to_jagged,
)
from generative_recommenders_amd.ops.preprocess import (  # noqa: E402
    COMBINE_INTERLEAVE_ALL,
    COMBINE_INTERLEAVE_UIH,
    COMBINE_SUM,
    action_encode,
    combine_embeddings,
)

PEAK_HBM = 8.0e12
DEV = "cuda"
WEIGHTS = [1, 2, 4, 8, 16]
THRESHOLDS = [(30, 32), (60, 64), (100, 128)]
MODES = {"sum": COMBINE_SUM, "interleave_all": COMBINE_INTERLEAVE_ALL, "interleave_uih": COMBINE_INTERLEAVE_UIH}


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def encoder_composition(actions, watchtimes, uih_offsets, target_offsets, table, target_table, combined, max_uih_len,
                        max_targets, total_targets, dtype):
    """ActionEncoder.forward as the reference writes it, on this package's concat_2D_jagged, then the preprocessor's cast"""
    a = actions
    for thr, w in THRESHOLDS:
        a = torch.bitwise_or(a, (watchtimes >= thr).to(torch.int64) * w)
    exploded = torch.bitwise_and(a.unsqueeze(-1), combined.unsqueeze(0)) > 0
    emb = (exploded.unsqueeze(-1) * table.unsqueeze(0)).view(-1, table.numel())
    out = concat_2D_jagged(max_seq_len=max_uih_len + max_targets, values_left=emb,
                           values_right=target_table.tile(total_targets, 1), max_len_left=max_uih_len,
                           max_len_right=max_targets, offsets_left=uih_offsets, offsets_right=target_offsets)
    return out.to(dtype)


def combine_composition(mode, max_uih_len, max_targets, seq_lengths, seq_timestamps, content, action, contextual, num_targets):
    """combine_embeddings as the reference writes it (modules/contextual_interleave_preprocessor.py:101-224)"""
    D = content.shape[1]
    C = contextual.shape[1]
    if mode == COMBINE_SUM:
        out_max, out_len, out_ts, out = max_uih_len + max_targets, seq_lengths, seq_timestamps, content + action
    else:
        out_ts = seq_timestamps.repeat_interleave(2)
        out = torch.stack([content, action], dim=1).reshape(-1, D)
        if mode == COMBINE_INTERLEAVE_ALL:
            out_len, out_max = seq_lengths * 2, (max_uih_len + max_targets) * 2
        else:
            by2 = seq_lengths * 2
            out_len, out_max = by2 - num_targets, 2 * max_uih_len + max_targets
            idx = torch.arange(2 * (max_uih_len + max_targets), device=seq_lengths.device).view(1, -1)
            valid = torch.logical_and(idx < by2.view(-1, 1),
                                      torch.logical_or(idx < (out_len - num_targets).view(-1, 1), torch.remainder(idx, 2) == 0))
            jagged_valid = dense_to_jagged(valid.int().unsqueeze(-1), asynchronous_complete_cumsum(by2),
                                           2 * content.shape[0]).to(torch.bool).squeeze(1)
            out, out_ts = out[jagged_valid], out_ts[jagged_valid]
    off = asynchronous_complete_cumsum(out_len)
    out = concat_2D_jagged(max_seq_len=C + out_max, values_left=contextual.reshape(-1, D), values_right=out, max_len_left=C,
                           max_len_right=out_max, offsets_left=None, offsets_right=off)
    out_ts = concat_2D_jagged(max_seq_len=C + out_max,
                              values_left=torch.zeros((seq_lengths.numel() * C, 1), dtype=out_ts.dtype, device=out_ts.device),
                              values_right=out_ts.unsqueeze(-1), max_len_left=C, max_len_right=out_max, offsets_left=None,
                              offsets_right=off).squeeze(-1)
    out_len = out_len + C
    return out, out_ts, out_len, asynchronous_complete_cumsum(out_len)


def _time(fns, iters, rounds):
    for fn in fns.values():         # pre-warm (code objects, the allocator) and warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():   # alternating: every round times every variant once
            times[k].append(_events_ms(fn, iters))
    return {k: statistics.median(v) for k, v in times.items()}, times


def _report(med, times, fwd_bytes, bwd_bytes):
    return {
        "ms": {k: round(v, 4) for k, v in med.items()},
        "ms_rounds": {k: [round(v, 4) for v in vs] for k, vs in times.items()},
        "fused_over_composition": {"fwd": round(med["fused_fwd"] / med["composition_fwd"], 3),
                                   "fwd_bwd": round(med["fused_fwd_bwd"] / med["composition_fwd_bwd"], 3)},
        "algorithmic_bytes": {"fwd": fwd_bytes, "fwd_bwd": fwd_bytes + bwd_bytes},
        "frac_of_8TBps": {k: round((fwd_bytes + (bwd_bytes if k.endswith("bwd") else 0)) / (v * 1e-3) / PEAK_HBM, 3)
                          for k, v in med.items()},
    }


def run(users, N, D, da, C, iters, rounds):
    gen = torch.Generator(device=DEV).manual_seed(1)
    lengths = torch.randint(int(0.9 * N), N, (users,), generator=gen, device=DEV, dtype=torch.int64)
    targets = torch.minimum(torch.randint(1, 21, (users,), generator=gen, device=DEV, dtype=torch.int64), lengths)
    total, total_targets = int(lengths.sum()), int(targets.sum())          # set-up only: the timed calls get the integers
    total_uih = total - total_targets
    max_uih_len, max_targets = int((lengths - targets).max()), int(targets.max())
    seq_offsets, target_offsets = asynchronous_complete_cumsum(lengths), asynchronous_complete_cumsum(targets)
    uih_offsets = seq_offsets - target_offsets
    s = 2
    res = {"shape": {"users": users, "max_seq_len": N, "rows": total, "target_rows": total_targets, "dim": D,
                     "action_width": len(WEIGHTS + THRESHOLDS) * da, "contextual_len": C, "dtype": "bfloat16"}}

    # ---- action encode
    T = len(WEIGHTS) + len(THRESHOLDS)
    combined_list = WEIGHTS + [w for _, w in THRESHOLDS]
    combined = torch.tensor(combined_list, device=DEV)
    actions = torch.randint(0, 32, (total_uih,), generator=gen, device=DEV, dtype=torch.int64)
    watch = torch.randint(0, 130, (total_uih,), generator=gen, device=DEV, dtype=torch.int64)
    table = (0.1 * torch.randn(T, da, device=DEV, generator=gen)).requires_grad_()
    ttable = (0.1 * torch.randn(1, T * da, device=DEV, generator=gen)).requires_grad_()
    r = torch.randn(total, T * da, device=DEV, generator=gen).to(torch.bfloat16)

    def enc_fused():
        return action_encode(actions, watch, uih_offsets, target_offsets, table, ttable, combined_list, THRESHOLDS, total_uih,
                             total_targets, torch.bfloat16)

    def enc_comp():
        return encoder_composition(actions, watch, uih_offsets, target_offsets, table, ttable, combined, max_uih_len,
                                   max_targets, total_targets, torch.bfloat16)

    def with_bwd(fn, leaves, grad):
        def go():
            for t in leaves:
                t.grad = None
            fn().backward(grad)
        return go

    def no_grad(fn):
        def go():
            with torch.no_grad():
                return fn()
        return go

    equal = torch.equal(enc_fused().view(torch.int16), enc_comp().view(torch.int16))
    med, times = _time({"fused_fwd": no_grad(enc_fused), "composition_fwd": no_grad(enc_comp),
                        "fused_fwd_bwd": with_bwd(enc_fused, (table, ttable), r),
                        "composition_fwd_bwd": with_bwd(enc_comp, (table, ttable), r)}, iters, rounds)
    res["action_encode"] = _report(med, times, total * T * da * s + total_uih * 16, total * T * da * s + total_uih * 16)
    res["action_encode"]["fused_equals_composition"] = equal
    del r
    torch.cuda.empty_cache()

    # ---- combine
    content = torch.randn(total, D, device=DEV, generator=gen).to(torch.bfloat16).requires_grad_()
    action = torch.randn(total, D, device=DEV, generator=gen).to(torch.bfloat16).requires_grad_()
    ctx = torch.randn(users, C, D, device=DEV, generator=gen).to(torch.bfloat16).requires_grad_()
    ts = torch.randint(1, 10**9, (total,), generator=gen, device=DEV, dtype=torch.int64)
    res["combine"] = {}
    for name, mode in MODES.items():
        def fused(mode=mode):
            return combine_embeddings(content, action, ctx, ts, lengths, seq_offsets, targets, total_uih, total_targets, mode)[0]

        def comp(mode=mode):
            return combine_composition(mode, max_uih_len, max_targets, lengths, ts, content, action, ctx, targets)[0]

        a = combine_embeddings(content, action, ctx, ts, lengths, seq_offsets, targets, total_uih, total_targets, mode)
        b = combine_composition(mode, max_uih_len, max_targets, lengths, ts, content, action, ctx, targets)
        equal = all(torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y)
                    for x, y in zip(a, b))
        out_rows = a[0].shape[0]
        grad = torch.randn(out_rows, D, device=DEV, generator=gen).to(torch.bfloat16)
        src_rows = {"sum": 2 * total, "interleave_all": 2 * total, "interleave_uih": 2 * total - total_targets}[name] + users * C
        med, times = _time({"fused_fwd": no_grad(fused), "composition_fwd": no_grad(comp),
                            "fused_fwd_bwd": with_bwd(fused, (content, action, ctx), grad),
                            "composition_fwd_bwd": with_bwd(comp, (content, action, ctx), grad)}, iters, rounds)
        fwd_bytes = (src_rows + out_rows) * D * s + 8 * (total + out_rows)
        bwd_bytes = (out_rows + 2 * total + users * C) * D * s
        res["combine"][name] = _report(med, times, fwd_bytes, bwd_bytes)
        res["combine"][name]["out_rows"] = out_rows
        res["combine"][name]["fused_equals_composition"] = equal
        del grad, a, b
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--max-seq-len", type=int, default=200)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--action-dim", type=int, default=32)
    ap.add_argument("--contextual-len", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocessor.py measures on the GPU: none found")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds}
    res.update(run(args.users, args.max_seq_len, args.dim, args.action_dim, args.contextual_len, args.iters, args.rounds))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
