"""Gated projection layers of the learned similarities (research/rails/similarities/layers.py): one GEMM producing both
halves, then activation(left) * right.  Parameter names ``_w`` (in, 2 out) and ``_b`` (1, 2 out) as in the reference."""

import torch
import torch.nn.functional as F


class _GatedLinearUnit(torch.nn.Module):
    def __init__(self, in_features: int, out_features: int) -> None:
        super().__init__()
        self._in_features = in_features
        self._out_features = out_features
        self._w = torch.nn.Parameter(torch.empty((in_features, 2 * out_features)).normal_(mean=0, std=0.02))
        self._b = torch.nn.Parameter(torch.zeros((1, 2 * out_features)))

    def _activation(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        lead = x.shape[:-1]
        both = torch.mm(x.reshape(-1, self._in_features), self._w) + self._b
        left, right = both.split(self._out_features, dim=-1)
        return (self._activation(left) * right).reshape(lead + (self._out_features,))


class GeGLU(_GatedLinearUnit):
    def _activation(self, x: torch.Tensor) -> torch.Tensor:
        return F.gelu(x)


class SwiGLU(_GatedLinearUnit):
    """https://arxiv.org/abs/2002.05202"""

    def _activation(self, x: torch.Tensor) -> torch.Tensor:
        return F.silu(x)
