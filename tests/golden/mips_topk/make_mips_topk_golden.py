#!/usr/bin/env python3
"""Mint the fixtures of the fused MIPS top-k from the REFERENCE's brute-force path on the CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/mips_topk/make_mips_topk_golden.py [--out DIR]

It imports the reference's ``MIPSBruteForceTopK`` (torch.mm + torch.topk) and ``CandidateIndex`` unmodified; both need
torch alone.  Every case is EXACT: queries are integers in [-2, 2], table entries integers in [-2, 2] (D <= 32) or
[-1, 1], so every score is an integer of magnitude <= 128 -- exact in fp32, bf16 and fp16 under any accumulation order --
and the reference's scores are checked here against fp64 before they are stored.  A row has few distinct scores, so ties
are everywhere; the reference's tie ORDER is arbitrary and is not stored: a fixture holds the inputs (int8), the
reference's top-k' scores and its filtered ``get_top_k_outputs`` scores (int16) per dtype.  The filtered score multiset
does not depend on the tie order: k' = k + N0 and filtering removes at most N0.  One compressed ``.npz`` per shape."""

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np
import torch

from generative_recommenders.research.indexing.candidate_index import CandidateIndex  # noqa: E402
from generative_recommenders.research.rails.indexing.mips_top_k import MIPSBruteForceTopK  # noqa: E402

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}

# (B, X, D, k, N0): k' = min(k + N0, X) results are fetched, k survive the filter
CASES = [
    (5, 700, 50, 33, 7),          # D needs padding, X ragged
    (3, 4500, 64, 2500, 61),      # k' = 2561: many item chunks, more than 2048 candidates
    (17, 1000, 32, 1000, 0),      # k == X, B ragged
    (1, 1, 8, 1, 0),
    (2, 257, 16, 1, 0),
    (64, 8195, 256, 300, 0),
]


def case_name(B, X, D, k, n0):
    return f"exact_b{B}_x{X}_d{D}_k{k}_n{n0}"


def make_case(B, X, D, k, n0, seed):
    g = torch.Generator().manual_seed(seed)
    queries = torch.randint(-2, 3, (B, D), generator=g, dtype=torch.int64)
    lim = 2 if D <= 32 else 1
    items = torch.randint(-lim, lim + 1, (X, D), generator=g, dtype=torch.int64)
    item_ids = (torch.randperm(4 * X + 11, generator=g)[:X] + 1).to(torch.int64)           # positive, distinct, not arange
    k_prime = min(k + n0, X)
    exact = (queries.double() @ items.double().t()).sort(dim=1, descending=True, stable=True)
    # invalid ids: some of the row's true best ids (every second of the first ~N0), zeros elsewhere
    invalid = torch.zeros((B, n0), dtype=torch.int64)
    for b in range(B):
        take = exact.indices[b, : min(2 * n0, X) : 2][: (n0 + 1) // 2]
        invalid[b, : take.numel()] = item_ids[take]
        invalid[b] = invalid[b, torch.randperm(n0, generator=g)] if n0 else invalid[b]
    out = {"queries": queries.to(torch.int8).numpy(), "items": items.to(torch.int8).numpy(), "item_ids": item_ids.numpy(),
           "invalid_ids": invalid.numpy(), "k": np.int64(k), "k_prime": np.int64(k_prime)}
    for name, dt in DTYPES.items():
        module = MIPSBruteForceTopK(item_embeddings=items.to(dt).unsqueeze(0), item_ids=item_ids.unsqueeze(0))
        scores, _ = module(query_embeddings=queries.to(dt), k=k_prime)
        assert torch.equal(scores.double(), exact.values[:, :k_prime]), f"reference scores are not exact in {name}"
        index = CandidateIndex(ids=item_ids.unsqueeze(0), embeddings=items.to(dt).unsqueeze(0))
        _, filtered, _ = index.get_top_k_outputs(query_embeddings=queries.to(dt), k=min(k, X), top_k_module=module,
                                                 invalid_ids=invalid if n0 else None)
        out[f"ref_scores_{name}"] = scores.to(torch.int16).numpy()
        out[f"ref_filtered_scores_{name}"] = filtered.to(torch.int16).numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for i, case in enumerate(CASES):
        np.savez_compressed(os.path.join(args.out, case_name(*case) + ".npz"), **make_case(*case, seed=20240 + i))


if __name__ == "__main__":
    main()
