"""The interface of MoL's component-embedding generators (research/rails/similarities/mol/embeddings_fn.py)."""

import abc
from typing import Dict, Tuple

import torch


class MoLEmbeddingsFn(torch.nn.Module):
    """input embeddings (B, ...) -> ((B, P, D_P) component embeddings, auxiliary losses by name); P = P_Q on the query
    side, P_X on the item side.  Keyword arguments are the implementation's."""

    @abc.abstractmethod
    def forward(self, input_embeddings: torch.Tensor, **kwargs) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        pass
