"""Shared by the MIPS top-k tests: the fixtures under tests/golden/mips_topk/ and the ranking RULE the kernel is held to --
score descending, then position in the table ascending -- restated in fp64 with a stable sort."""

import os

import numpy as np
import torch

from conftest import GOLDEN

FIXTURES = os.path.join(GOLDEN, "mips_topk")
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def fixture_files():
    return sorted(os.path.join(FIXTURES, f) for f in os.listdir(FIXTURES) if f.endswith(".npz"))


def load_case(path):
    z = np.load(path, allow_pickle=False)
    c = {k: z[k] for k in z.files}
    c["name"] = os.path.basename(path)[:-4]
    return c


def rule_topk(queries: torch.Tensor, items: torch.Tensor, k: int):
    """(scores fp64 (B, k), positions int64 (B, k)) by the rule; -0.0 == +0.0 in the comparison, the stable sort breaks
    ties by position"""
    s = queries.double() @ items.double().t()
    order = torch.sort(s, dim=1, descending=True, stable=True)
    return order.values[:, :k], order.indices[:, :k]


def rule_filtered(ids: torch.Tensor, scores: torch.Tensor, invalid_ids, k: int):
    """the first k entries of every row of (ids, scores) whose id is not among the row's invalid ids"""
    if invalid_ids is None:
        return ids[:, :k], scores[:, :k]
    out_i, out_s = [], []
    for b in range(ids.shape[0]):
        bad = set(invalid_ids[b].tolist())
        keep = [j for j, v in enumerate(ids[b].tolist()) if v not in bad][:k]
        out_i.append(ids[b, keep])
        out_s.append(scores[b, keep])
    return torch.stack(out_i), torch.stack(out_s)
