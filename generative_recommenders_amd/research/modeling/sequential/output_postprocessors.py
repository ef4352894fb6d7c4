"""The output postprocessors of the research path (research/modeling/sequential/output_postprocessors.py) on the row
kernels of this package: ``hstu_l2_norm_*`` and ``hstu_layer_norm_*``.  Neither owns a parameter.  The slice
``[..., :embedding_dim]`` is a no-op in every shipped configuration; when it really cuts, the kept columns are copied to
contiguous rows once (the row kernels read whole contiguous rows) and autograd scatters the gradient back."""

import abc

import torch

from generative_recommenders_amd.modules.postprocessors import l2_norm
from generative_recommenders_amd.ops.layer_norm import layer_norm


class OutputPostprocessorModule(torch.nn.Module):
    @abc.abstractmethod
    def debug_str(self) -> str:
        pass

    @abc.abstractmethod
    def forward(self, output_embeddings: torch.Tensor) -> torch.Tensor:
        pass


class L2NormEmbeddingPostprocessor(OutputPostprocessorModule):
    def __init__(self, embedding_dim: int, eps: float = 1e-6) -> None:
        super().__init__()
        self._embedding_dim: int = embedding_dim
        self._eps: float = eps

    def debug_str(self) -> str:
        return "l2"

    def forward(self, output_embeddings: torch.Tensor) -> torch.Tensor:
        return l2_norm(output_embeddings[..., : self._embedding_dim], self._eps)


class LayerNormEmbeddingPostprocessor(OutputPostprocessorModule):
    def __init__(self, embedding_dim: int, eps: float = 1e-6) -> None:
        super().__init__()
        self._embedding_dim: int = embedding_dim
        self._eps: float = eps

    def debug_str(self) -> str:
        return "ln"

    def forward(self, output_embeddings: torch.Tensor) -> torch.Tensor:
        x = output_embeddings[..., : self._embedding_dim]
        # no affine parameters: the kernel's weight and bias are ones and zeros
        ones = torch.ones(self._embedding_dim, dtype=x.dtype, device=x.device)
        return layer_norm(x, ones, torch.zeros_like(ones), self._eps)
