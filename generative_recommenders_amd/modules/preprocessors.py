"""Drop-in for generative_recommenders/modules/preprocessors.py: ``InputPreprocessor`` (:35-79),
``get_contextual_input_embeddings`` (:82-105) and ``ContextualPreprocessor`` (:108-304), with the reference's constructor
arguments, parameter names and forward signatures.  The action rows come from the fused encoder (ops/preprocess.py), the
contextual rows are put in front of every user's sequence by ``combine_embeddings`` (one gather that also writes the
timestamps) and the MLPs' norms are this package's HIP kernels.  The contextual projection is ``B * C`` rows and stays a
torch ``baddbmm``."""

import abc
from math import sqrt
from typing import Dict, List, Optional, Tuple

import torch

from generative_recommenders_amd.common import HammerModule
from generative_recommenders_amd.modules.action_encoder import ActionEncoder
from generative_recommenders_amd.modules.contextualize_mlps import init_mlp_weights_optional_bias
from generative_recommenders_amd.ops.jagged_tensors import asynchronous_complete_cumsum, jagged_to_padded_dense
from generative_recommenders_amd.ops.layer_norm import LayerNorm, SwishLayerNorm
from generative_recommenders_amd.ops.preprocess import COMBINE_SUM, combine_embeddings

PreprocessorOutput = Tuple[int, int, int, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                           Dict[str, torch.Tensor]]


class InputPreprocessor(HammerModule):
    """An abstract class for pre-processing sequence embeddings before HSTU layers."""

    @abc.abstractmethod
    def forward(
        self,
        max_uih_len: int,
        max_targets: int,
        total_uih_len: int,
        total_targets: int,
        seq_lengths: torch.Tensor,
        seq_timestamps: torch.Tensor,
        seq_embeddings: torch.Tensor,
        num_targets: torch.Tensor,
        seq_payloads: Dict[str, torch.Tensor],
    ) -> PreprocessorOutput:
        """seq_lengths (B,), seq_timestamps (sum L,), seq_embeddings (sum L, D), num_targets (B,), seq_payloads: str-keyed
        tensors.  Returns (max_seq_len, total_uih_len, total_targets, lengths, offsets, timestamps, embeddings,
        num_targets, payloads) of the preprocessed sequence."""

    def interleave_targets(self) -> bool:
        return False


def get_contextual_input_embeddings(
    seq_lengths: torch.Tensor,
    seq_payloads: Dict[str, torch.Tensor],
    contextual_feature_to_max_length: Dict[str, int],
    contextual_feature_to_min_uih_length: Dict[str, int],
    dtype: torch.dtype,
) -> torch.Tensor:
    padded_values: List[torch.Tensor] = []
    for key, max_len in contextual_feature_to_max_length.items():
        v = torch.flatten(
            jagged_to_padded_dense(seq_payloads[key].to(dtype), seq_payloads[key + "_offsets"], max_len), 1, 2)
        min_uih_length = contextual_feature_to_min_uih_length.get(key, 0)
        if min_uih_length > 0:
            v = v * (seq_lengths.view(-1, 1) >= min_uih_length)
        padded_values.append(v)
    return torch.cat(padded_values, dim=1)


def contextual_projection(contextual_input_embeddings: torch.Tensor, weights: torch.Tensor, bias: torch.Tensor,
                          max_contextual_seq_len: int, input_embedding_dim: int) -> torch.Tensor:
    """(B, C * D_in) -> (B, C, D_out): one linear per contextual position (B * C rows: a torch ``baddbmm``)"""
    dt = contextual_input_embeddings.dtype
    return torch.baddbmm(
        bias.view(max_contextual_seq_len, 1, -1).to(dt),
        contextual_input_embeddings.view(-1, max_contextual_seq_len, input_embedding_dim).transpose(0, 1),
        weights.to(dt),
    ).transpose(0, 1)


class ContextualPreprocessor(InputPreprocessor):
    def __init__(
        self,
        input_embedding_dim: int,
        output_embedding_dim: int,
        contextual_feature_to_max_length: Dict[str, int],
        contextual_feature_to_min_uih_length: Dict[str, int],
        action_embedding_dim: int = 8,
        action_feature_name: str = "",
        action_weights: Optional[List[int]] = None,
        is_inference: bool = True,
    ) -> None:
        super().__init__(is_inference=is_inference)
        self._output_embedding_dim: int = output_embedding_dim
        self._input_embedding_dim: int = input_embedding_dim
        self._contextual_feature_to_max_length: Dict[str, int] = contextual_feature_to_max_length
        self._max_contextual_seq_len: int = sum(contextual_feature_to_max_length.values())
        self._contextual_feature_to_min_uih_length: Dict[str, int] = contextual_feature_to_min_uih_length
        if self._max_contextual_seq_len > 0:
            std = 1.0 * sqrt(2.0 / float(input_embedding_dim + self._output_embedding_dim))
            self._batched_contextual_linear_weights: torch.nn.Parameter = torch.nn.Parameter(
                torch.empty((self._max_contextual_seq_len, input_embedding_dim, self._output_embedding_dim)).normal_(0.0, std))
            self._batched_contextual_linear_bias: torch.nn.Parameter = torch.nn.Parameter(
                torch.empty((self._max_contextual_seq_len, self._output_embedding_dim)).fill_(0.0))
        hidden_dim = 256
        self._content_embedding_mlp: torch.nn.Module = torch.nn.Sequential(
            torch.nn.Linear(in_features=self._input_embedding_dim, out_features=hidden_dim),
            SwishLayerNorm(hidden_dim),
            torch.nn.Linear(in_features=hidden_dim, out_features=self._output_embedding_dim),
            LayerNorm(self._output_embedding_dim),
        ).apply(init_mlp_weights_optional_bias)
        self._action_feature_name: str = action_feature_name
        self._action_weights: Optional[List[int]] = action_weights
        if self._action_weights is not None:
            self._action_encoder: ActionEncoder = ActionEncoder(
                action_feature_name=action_feature_name, action_weights=self._action_weights,
                action_embedding_dim=action_embedding_dim, is_inference=is_inference)
            self._action_embedding_mlp: torch.nn.Module = torch.nn.Sequential(
                torch.nn.Linear(in_features=self._action_encoder.output_embedding_dim, out_features=hidden_dim),
                SwishLayerNorm(hidden_dim),
                torch.nn.Linear(in_features=hidden_dim, out_features=self._output_embedding_dim),
                LayerNorm(self._output_embedding_dim),
            ).apply(init_mlp_weights_optional_bias)

    def forward(
        self,
        max_uih_len: int,
        max_targets: int,
        total_uih_len: int,
        total_targets: int,
        seq_lengths: torch.Tensor,
        seq_timestamps: torch.Tensor,
        seq_embeddings: torch.Tensor,
        num_targets: torch.Tensor,
        seq_payloads: Dict[str, torch.Tensor],
    ) -> PreprocessorOutput:
        content_embeddings = self._content_embedding_mlp(seq_embeddings)
        seq_offsets = asynchronous_complete_cumsum(seq_lengths)
        action_embeddings: Optional[torch.Tensor] = None
        if self._action_weights is not None:
            target_offsets = asynchronous_complete_cumsum(num_targets)
            action_embeddings = self._action_embedding_mlp(self._action_encoder(
                max_uih_len=max_uih_len, max_targets=max_targets, uih_offsets=seq_offsets - target_offsets,
                target_offsets=target_offsets, seq_embeddings=seq_embeddings, seq_payloads=seq_payloads))
        contextual_embeddings: Optional[torch.Tensor] = None
        C = self._max_contextual_seq_len
        if C > 0:
            contextual_embeddings = contextual_projection(
                get_contextual_input_embeddings(
                    seq_lengths=seq_lengths, seq_payloads=seq_payloads,
                    contextual_feature_to_max_length=self._contextual_feature_to_max_length,
                    contextual_feature_to_min_uih_length=self._contextual_feature_to_min_uih_length,
                    dtype=seq_embeddings.dtype),
                self._batched_contextual_linear_weights, self._batched_contextual_linear_bias, C, self._input_embedding_dim)
        if action_embeddings is None and contextual_embeddings is None:
            return (max_uih_len + max_targets, total_uih_len, total_targets, seq_lengths, seq_offsets, seq_timestamps,
                    content_embeddings, num_targets, seq_payloads)
        # content + action and the contextual rows (timestamp 0) in front of every user: one gather
        output_seq_embeddings, output_seq_timestamps, output_seq_lengths, output_seq_offsets = combine_embeddings(
            content_embeddings, action_embeddings, contextual_embeddings, seq_timestamps, seq_lengths, seq_offsets,
            num_targets, total_uih_len, total_targets, COMBINE_SUM)
        return (max_uih_len + max_targets + C, total_uih_len + C * seq_lengths.size(0), total_targets, output_seq_lengths,
                output_seq_offsets, output_seq_timestamps, output_seq_embeddings, num_targets, seq_payloads)
