"""Drop-in for generative_recommenders/research/rails/indexing/candidate_index.py: the interface of a top-k module."""

import abc
from typing import Tuple

import torch


class TopKModule(torch.nn.Module, abc.ABC):
    @abc.abstractmethod
    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """query_embeddings (B, ...), implementation-specific -> (top_k_scores (B, k), top_k_ids (B, k))"""
