"""Drop-in for generative_recommenders/research/rails/indexing/mips_top_k.py.  ``MIPSBruteForceTopK`` is exhaustive like the
reference's (every item is scored) but fused: csrc/mips_topk.hip recomputes MFMA score tiles inside a radix select, so the
(B, X) logit matrix of ``torch.mm`` + ``torch.topk`` never exists.  The order is fixed -- score descending, then position in
the table ascending -- where ``torch.topk`` leaves ties unspecified."""

from typing import Tuple

import torch

from generative_recommenders_amd import _lib as L
from generative_recommenders_amd.ops import _launch
from generative_recommenders_amd.research.rails.indexing.candidate_index import TopKModule


class MIPSTopKModule(TopKModule):
    def __init__(self, item_embeddings: torch.Tensor, item_ids: torch.Tensor) -> None:
        """item_embeddings (1, X, D), item_ids (1, X)"""
        super().__init__()
        self._item_embeddings: torch.Tensor = item_embeddings
        self._item_ids: torch.Tensor = item_ids


class MIPSBruteForceTopK(MIPSTopKModule):
    def __init__(self, item_embeddings: torch.Tensor, item_ids: torch.Tensor) -> None:
        super().__init__(item_embeddings=item_embeddings, item_ids=item_ids)
        del self._item_embeddings
        if item_embeddings.dim() != 3 or item_embeddings.size(0) != 1 or item_ids.shape != item_embeddings.shape[:2]:
            raise ValueError(f"item_embeddings (1, X, D) and item_ids (1, X) expected, got {tuple(item_embeddings.shape)} and "
                             f"{tuple(item_ids.shape)}")
        table = item_embeddings.detach().squeeze(0)
        self._dim: int = table.size(1)
        # the kernel reads 16-byte aligned rows: the table is zero-padded (50 -> 56 columns in bf16) once, here
        pad = _launch.mips_topk_dim(self._dim, table.dtype) - self._dim if table.is_floating_point() else 0
        self._items: torch.Tensor = (torch.nn.functional.pad(table, (0, pad)) if pad else table).contiguous()

    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """query_embeddings (B, D) -> (top_k_scores (B, k) in the queries' dtype, top_k_ids (B, k)), always sorted (which serves
        both values of ``sorted``)"""
        L.require_gpu_tensor(query_embeddings, "query_embeddings")
        L.require_gpu_tensor(self._items, "item_embeddings")
        if query_embeddings.dim() != 2 or query_embeddings.size(1) != self._dim:
            raise RuntimeError(f"query_embeddings (B, {self._dim}) expected, got {tuple(query_embeddings.shape)}")
        scores, indices = _launch.mips_topk(query_embeddings.detach(), self._items, k)
        return scores, self._item_ids.squeeze(0)[indices.long()]
