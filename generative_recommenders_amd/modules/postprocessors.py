"""Drop-in for generative_recommenders/modules/postprocessors.py:30-176: the output postprocessors applied to the
(candidate) embeddings after the STU stack -- ``L2NormPostprocessor``, ``LayerNormPostprocessor`` and
``TimestampLayerNormPostprocessor`` on the HIP row kernels (same class, parameter and buffer names).  The last one
(:105-176: time features concatenated onto every row, a Linear, a LayerNorm) is the postprocessor ``DlrmHSTU`` builds by
default (modules/dlrm_hstu.py:182-191); here it is one GEMM with an aligned contraction length and one fused row pass
(ops/timestamp_layer_norm.py)."""

from abc import abstractmethod
from typing import Dict, List, Tuple

import torch

from generative_recommenders_amd.common import HammerModule
from generative_recommenders_amd.modules.contextualize_mlps import init_mlp_weights_optional_bias
from generative_recommenders_amd.ops import _launch
from generative_recommenders_amd.ops.layer_norm import layer_norm
from generative_recommenders_amd.ops.timestamp_layer_norm import timestamp_layer_norm


class _L2NormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        ctx.save_for_backward(x)
        ctx.eps = eps
        return _launch.l2_norm_fwd(x, eps)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return _launch.l2_norm_bwd(dy, x, ctx.eps), None


def l2_norm(x: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """x / max(||x||_2, eps) over the last dim"""
    return _L2NormFunction.apply(x, eps)


class OutputPostprocessor(HammerModule):
    """An abstract class for post-processing user embeddings after HSTU layers."""

    @abstractmethod
    def forward(self, seq_embeddings: torch.Tensor, seq_timestamps: torch.Tensor,
                seq_payloads: Dict[str, torch.Tensor]) -> torch.Tensor:
        pass


class L2NormPostprocessor(OutputPostprocessor):
    """Postprocesses user embeddings with l2 norm."""

    def __init__(self, is_inference: bool = False) -> None:
        super().__init__(is_inference=is_inference)

    def forward(self, seq_embeddings: torch.Tensor, seq_timestamps: torch.Tensor,
                seq_payloads: Dict[str, torch.Tensor]) -> torch.Tensor:
        return l2_norm(seq_embeddings, 1e-6)


class LayerNormPostprocessor(OutputPostprocessor):
    """Postprocesses user embeddings with layer norm."""

    def __init__(self, embedding_dim: int, eps: float = 1e-5, is_inference: bool = False) -> None:
        super().__init__(is_inference=is_inference)
        self._layer_norm: torch.nn.LayerNorm = torch.nn.LayerNorm(normalized_shape=[embedding_dim], eps=eps)

    def forward(self, seq_embeddings: torch.Tensor, seq_timestamps: torch.Tensor,
                seq_payloads: Dict[str, torch.Tensor]) -> torch.Tensor:
        ln = self._layer_norm
        return layer_norm(seq_embeddings.to(ln.weight.dtype), ln.weight, ln.bias, ln.eps)


class TimestampLayerNormPostprocessor(OutputPostprocessor):
    """Postprocesses user embeddings with timestamp-based MLP -> layer norm."""

    def __init__(self, embedding_dim: int, time_duration_features: List[Tuple[int, int]], eps: float = 1e-5,
                 is_inference: bool = False) -> None:
        super().__init__(is_inference=is_inference)
        self._layer_norm: torch.nn.LayerNorm = torch.nn.LayerNorm(normalized_shape=[embedding_dim], eps=eps)
        self.register_buffer("_period_units", torch.Tensor([f[0] for f in time_duration_features]).view(1, -1))
        self.register_buffer("_units_per_period", torch.Tensor([f[1] for f in time_duration_features]).view(1, -1))
        self._time_feature_combiner: torch.nn.Linear = torch.nn.Linear(
            embedding_dim + 2 * len(time_duration_features), embedding_dim).apply(init_mlp_weights_optional_bias)

    def _apply(self, fn, *args, **kwargs):
        """the two time buffers stay fp32 whatever dtype the module is cast to (they only move between devices):
        ``.to(torch.bfloat16)`` would turn 86400 into 86528 and ``.double()`` would move timestamps into other buckets"""
        period_units, units_per_period = self._period_units, self._units_per_period
        super()._apply(fn, *args, **kwargs)
        if self._period_units.dtype != torch.float32:
            self._period_units = period_units.to(self._period_units.device)
            self._units_per_period = units_per_period.to(self._units_per_period.device)
        return self

    def forward(self, seq_embeddings: torch.Tensor, seq_timestamps: torch.Tensor,
                seq_payloads: Dict[str, torch.Tensor]) -> torch.Tensor:
        """seq_embeddings (L, D) with seq_timestamps (L,), or the reference's (B, N, D) with (B, N): flattened around the op"""
        lin, ln = self._time_feature_combiner, self._layer_norm
        shape = seq_embeddings.shape
        out = timestamp_layer_norm(seq_embeddings.reshape(-1, shape[-1]), seq_timestamps.reshape(-1), lin.weight, lin.bias,
                                   ln.weight, ln.bias, self._period_units, self._units_per_period, ln.eps)
        return out.view(shape)
