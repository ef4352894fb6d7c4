"""The similarity interface of the research path (research/rails/similarities/module.py)."""

import abc
from typing import Dict, Tuple

import torch


class SimilarityModule(torch.nn.Module):
    """query_embeddings (B, D) and item_embeddings (1 or B, X, D) -> ((B, X) similarities, auxiliary losses by name);
    further keyword arguments (item ids, side information) are the implementation's"""

    @abc.abstractmethod
    def forward(self, query_embeddings: torch.Tensor, item_embeddings: torch.Tensor,
                **kwargs) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        pass
