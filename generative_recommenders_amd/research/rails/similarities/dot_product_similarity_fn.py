"""Inner-product similarity (research/rails/similarities/dot_product_similarity_fn.py): plain torch GEMMs."""

from typing import Dict, Tuple

import torch

from generative_recommenders_amd.research.rails.similarities.module import SimilarityModule


class DotProductSimilarity(SimilarityModule):
    def __init__(self) -> None:
        super().__init__()

    def debug_str(self) -> str:
        return "dp"

    def forward(self, query_embeddings: torch.Tensor, item_embeddings: torch.Tensor,
                **kwargs) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        """query_embeddings (B, D) or (B * r, D); item_embeddings (1, X, D) or (B, X, D).  Returns (B [* r], X)."""
        item_batch, X, D = item_embeddings.size()
        if item_batch == 1:                                      # one item set for every query: (B, D) x (D, X)
            return torch.mm(query_embeddings, item_embeddings.squeeze(0).t()), {}
        if query_embeddings.size(0) != item_batch:               # r queries per item set: (B, r, D) x (B, D, X)
            scores = torch.bmm(query_embeddings.view(item_batch, -1, D), item_embeddings.permute(0, 2, 1))
            return scores.view(-1, X), {}
        return torch.bmm(item_embeddings, query_embeddings.unsqueeze(2)).squeeze(2), {}    # one item set per query
