"""Drop-in for generative_recommenders/modules/contextualize_mlps.py: the per-user action / content MLPs of DLRM-v3's
``ContextualInterleavePreprocessor`` (modules/contextual_interleave_preprocessor.py:266-268).  Constructor arguments and
parameter names are the reference's, so its ``state_dict`` loads with ``strict=True``:

* ``SimpleContextualizedMLP`` (:48-78): ``_mlp.{0,1,2,3}`` = Linear, SwishLayerNorm, Linear, LayerNorm; ignores the context.
* ``ParameterizedContextualizedMLP`` (:81-146): the contextual embedding is compressed (``_dense_features_compress``), one
  small linear turns it into a (K, N) weight per user (``_attn_raw_weights.0``, normalised over both dims by
  ``_attn_weights_norm``), another branch into a per-user bias (``_res_weights.{0,1,2}``), and the sequence goes through
  ``jagged_dense_bmm_broadcast_add`` -- the HIP per-user GEMM -- with them.

The small linears stay ``torch.nn.Linear`` (they see B rows, not sum(L)); the two norms of the sequence path and the GEMM
are this package's HIP kernels."""

import abc
from typing import Optional

import torch

from generative_recommenders_amd.common import HammerModule
from generative_recommenders_amd.ops.jagged_tensors import jagged_dense_bmm_broadcast_add
from generative_recommenders_amd.ops.layer_norm import LayerNorm, SwishLayerNorm


def init_mlp_weights_optional_bias(m: torch.nn.Module) -> None:
    """common.py:361-365: Xavier-uniform weights and zero biases for every Linear"""
    if isinstance(m, torch.nn.Linear):
        torch.nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            m.bias.data.fill_(0.0)


class ContextualizedMLP(HammerModule):
    @abc.abstractmethod
    def forward(
        self,
        seq_embeddings: torch.Tensor,
        seq_offsets: torch.Tensor,
        max_seq_len: int,
        contextual_embeddings: Optional[torch.Tensor],
    ) -> torch.Tensor:
        """seq_embeddings (L, D), seq_offsets (B + 1,), contextual_embeddings (B, D') -> (L, D_out)"""


class SimpleContextualizedMLP(ContextualizedMLP):
    def __init__(self, sequential_input_dim: int, sequential_output_dim: int, hidden_dim: int,
                 is_inference: bool = False) -> None:
        super().__init__(is_inference=is_inference)
        self._mlp: torch.nn.Module = torch.nn.Sequential(
            torch.nn.Linear(in_features=sequential_input_dim, out_features=hidden_dim),
            SwishLayerNorm(hidden_dim, is_inference=is_inference),
            torch.nn.Linear(in_features=hidden_dim, out_features=sequential_output_dim),
            LayerNorm(sequential_output_dim),
        ).apply(init_mlp_weights_optional_bias)

    def forward(
        self,
        seq_embeddings: torch.Tensor,
        seq_offsets: torch.Tensor,
        max_seq_len: int,
        contextual_embeddings: Optional[torch.Tensor],
    ) -> torch.Tensor:
        return self._mlp(seq_embeddings)


class ParameterizedContextualizedMLP(ContextualizedMLP):
    def __init__(self, contextual_embedding_dim: int, sequential_input_dim: int, sequential_output_dim: int,
                 hidden_dim: int, is_inference: bool = False) -> None:
        super().__init__(is_inference=is_inference)
        self._sequential_input_dim: int = sequential_input_dim
        self._sequential_output_dim: int = sequential_output_dim
        self._dense_features_compress: torch.nn.Module = torch.nn.Linear(
            in_features=contextual_embedding_dim, out_features=hidden_dim,
        ).apply(init_mlp_weights_optional_bias)
        self._attn_raw_weights: torch.nn.Module = torch.nn.Sequential(
            torch.nn.Linear(in_features=hidden_dim, out_features=sequential_input_dim * sequential_output_dim),
        ).apply(init_mlp_weights_optional_bias)
        self._attn_weights_norm: torch.nn.Module = torch.nn.LayerNorm([sequential_input_dim, sequential_output_dim])
        self._res_weights: torch.nn.Module = torch.nn.Sequential(
            torch.nn.Linear(in_features=hidden_dim, out_features=hidden_dim),
            SwishLayerNorm(hidden_dim),
            torch.nn.Linear(in_features=hidden_dim, out_features=sequential_output_dim),
        ).apply(init_mlp_weights_optional_bias)

    def forward(
        self,
        seq_embeddings: torch.Tensor,
        seq_offsets: torch.Tensor,
        max_seq_len: int,
        contextual_embeddings: Optional[torch.Tensor],
    ) -> torch.Tensor:
        if contextual_embeddings is None:
            raise RuntimeError("ParameterizedContextualizedMLP needs contextual_embeddings")
        shared_input = self._dense_features_compress(contextual_embeddings)
        attn_weights = self._attn_weights_norm(
            self._attn_raw_weights(shared_input).reshape(-1, self._sequential_input_dim, self._sequential_output_dim)
        )
        return jagged_dense_bmm_broadcast_add(
            max_seq_len=max_seq_len,
            seq_offsets=seq_offsets,
            jagged=seq_embeddings,
            dense=attn_weights.to(seq_embeddings.dtype),
            bias=self._res_weights(shared_input),
            kernel=self.hammer_kernel(),
        )
