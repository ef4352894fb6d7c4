"""Drop-in for generative_recommenders/modules/contextual_interleave_preprocessor.py:37-357
(``ContextualInterleavePreprocessor``): the input stage of DLRM-v3.  Constructor arguments, parameter names
(``_batched_contextual_linear_weights`` / ``_bias``, ``_content_encoder.*``, ``_content_embedding_mlp.*``,
``_action_encoder.*``, ``_action_embedding_mlp.*``) and both signatures are the reference's.

What runs where: the action encoder and ``combine_embeddings`` are the two fused HIP row passes of ops/preprocess.py (the
reference's stack / mask / ``dense_to_jagged`` / boolean index / two ``concat_2D_jagged`` chain, host sync included, is one
gather here); the contextualized MLPs are modules/contextualize_mlps.py; the contextual projection and the pMLP dropout
see ``B * C`` rows and stay torch calls.  The autocast context is the reference's: it is what lets the fp32 Linears of the
MLPs take bf16 activations."""

from math import sqrt
from typing import Callable, Dict, Optional, Tuple

import torch

from generative_recommenders_amd.modules.action_encoder import ActionEncoder
from generative_recommenders_amd.modules.content_encoder import ContentEncoder
from generative_recommenders_amd.modules.contextualize_mlps import ContextualizedMLP, ParameterizedContextualizedMLP
from generative_recommenders_amd.modules.preprocessors import (
    InputPreprocessor,
    PreprocessorOutput,
    contextual_projection,
    get_contextual_input_embeddings,
)
from generative_recommenders_amd.ops.jagged_tensors import asynchronous_complete_cumsum
from generative_recommenders_amd.ops.preprocess import (
    COMBINE_INTERLEAVE_ALL,
    COMBINE_INTERLEAVE_UIH,
    COMBINE_SUM,
    combine_embeddings,
)


class ContextualInterleavePreprocessor(InputPreprocessor):
    def __init__(
        self,
        input_embedding_dim: int,
        output_embedding_dim: int,
        contextual_feature_to_max_length: Dict[str, int],
        contextual_feature_to_min_uih_length: Dict[str, int],
        content_encoder: ContentEncoder,
        content_contextualize_mlp_fn: Callable[[int, int, int, bool], ContextualizedMLP],
        action_encoder: ActionEncoder,
        action_contextualize_mlp_fn: Callable[[int, int, int, bool], ContextualizedMLP],
        pmlp_contextual_dropout_ratio: float = 0.0,
        enable_interleaving: bool = False,
        is_inference: bool = False,
    ) -> None:
        super().__init__(is_inference=is_inference)
        self._input_embedding_dim: int = input_embedding_dim
        self._output_embedding_dim: int = output_embedding_dim
        self._contextual_feature_to_max_length: Dict[str, int] = contextual_feature_to_max_length
        self._max_contextual_seq_len: int = sum(contextual_feature_to_max_length.values())
        self._contextual_feature_to_min_uih_length: Dict[str, int] = contextual_feature_to_min_uih_length
        std = 1.0 * sqrt(2.0 / float(input_embedding_dim + output_embedding_dim))
        self._batched_contextual_linear_weights = torch.nn.Parameter(
            torch.empty((self._max_contextual_seq_len, input_embedding_dim, output_embedding_dim)).normal_(0.0, std))
        self._pmlp_contextual_dropout_ratio: float = pmlp_contextual_dropout_ratio
        self._batched_contextual_linear_bias = torch.nn.Parameter(
            torch.empty((self._max_contextual_seq_len, 1, output_embedding_dim)).fill_(0.0))
        contextual_embedding_dim: int = self._max_contextual_seq_len * input_embedding_dim
        self._content_encoder: ContentEncoder = content_encoder
        self._content_embedding_mlp: ContextualizedMLP = content_contextualize_mlp_fn(
            self._content_encoder.output_embedding_dim, output_embedding_dim, contextual_embedding_dim, is_inference)
        self._action_encoder: ActionEncoder = action_encoder
        self._action_embedding_mlp: ContextualizedMLP = action_contextualize_mlp_fn(
            self._action_encoder.output_embedding_dim, output_embedding_dim, contextual_embedding_dim, is_inference)
        self._enable_interleaving: bool = enable_interleaving

    def combine_mode(self) -> int:
        if not self._enable_interleaving:
            return COMBINE_SUM
        return COMBINE_INTERLEAVE_ALL if self.interleave_targets() else COMBINE_INTERLEAVE_UIH

    def combine_embeddings(
        self,
        max_uih_len: int,
        max_targets: int,
        total_uih_len: int,
        total_targets: int,
        seq_lengths: torch.Tensor,
        seq_timestamps: torch.Tensor,
        content_embeddings: torch.Tensor,
        action_embeddings: torch.Tensor,
        contextual_embeddings: Optional[torch.Tensor],
        num_targets: torch.Tensor,
        seq_offsets: Optional[torch.Tensor] = None,
    ) -> Tuple[int, int, int, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """the reference's method (:101-224) and return tuple; ``seq_offsets``: the caller's, when it has them already"""
        mode = self.combine_mode()
        C = self._max_contextual_seq_len
        if seq_offsets is None:
            seq_offsets = asynchronous_complete_cumsum(seq_lengths)
        output_seq_embeddings, output_seq_timestamps, output_seq_lengths, output_seq_offsets = combine_embeddings(
            content_embeddings, action_embeddings, contextual_embeddings if C > 0 else None, seq_timestamps, seq_lengths,
            seq_offsets, num_targets, total_uih_len, total_targets, mode)
        if mode == COMBINE_SUM:
            output_max_seq_len = max_uih_len + max_targets
            output_num_targets, output_total_uih_len, output_total_targets = num_targets, total_uih_len, total_targets
        elif mode == COMBINE_INTERLEAVE_ALL:
            output_max_seq_len = (max_uih_len + max_targets) * 2
            output_num_targets, output_total_uih_len, output_total_targets = num_targets * 2, total_uih_len * 2, total_targets * 2
        else:
            output_max_seq_len = 2 * max_uih_len + max_targets
            output_num_targets, output_total_uih_len, output_total_targets = num_targets, total_uih_len * 2, total_targets
        return (output_max_seq_len + C, output_total_uih_len + C * seq_lengths.size(0), output_total_targets,
                output_seq_lengths, output_seq_offsets, output_seq_timestamps, output_seq_embeddings, output_num_targets)

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
        max_seq_len = max_uih_len + max_targets
        with torch.autocast("cuda", dtype=torch.bfloat16,
                            enabled=(not self.is_inference and self._training_dtype == torch.bfloat16)):
            contextual_embeddings: Optional[torch.Tensor] = None
            pmlp_contextual_embeddings: Optional[torch.Tensor] = None
            if self._max_contextual_seq_len > 0:
                contextual_input_embeddings = get_contextual_input_embeddings(
                    seq_lengths=seq_lengths, seq_payloads=seq_payloads,
                    contextual_feature_to_max_length=self._contextual_feature_to_max_length,
                    contextual_feature_to_min_uih_length=self._contextual_feature_to_min_uih_length,
                    dtype=seq_embeddings.dtype)
                if isinstance(self._action_embedding_mlp, ParameterizedContextualizedMLP) or isinstance(
                        self._content_embedding_mlp, ParameterizedContextualizedMLP):
                    pmlp_contextual_embeddings = torch.nn.functional.dropout(
                        contextual_input_embeddings, p=self._pmlp_contextual_dropout_ratio, training=self.training)
                contextual_embeddings = contextual_projection(
                    contextual_input_embeddings, self._batched_contextual_linear_weights,
                    self._batched_contextual_linear_bias, self._max_contextual_seq_len, self._input_embedding_dim)

            seq_offsets = asynchronous_complete_cumsum(seq_lengths)
            target_offsets = asynchronous_complete_cumsum(num_targets)
            uih_offsets = seq_offsets - target_offsets
            content_embeddings = self._content_encoder(
                max_uih_len=max_uih_len, max_targets=max_targets, uih_offsets=uih_offsets, target_offsets=target_offsets,
                seq_embeddings=seq_embeddings, seq_payloads=seq_payloads)
            content_embeddings = self._content_embedding_mlp(
                seq_embeddings=content_embeddings, seq_offsets=seq_offsets, max_seq_len=max_seq_len,
                contextual_embeddings=pmlp_contextual_embeddings)

            # the encoder writes the activation dtype directly (the reference casts behind it)
            action_embeddings = self._action_encoder.encode(
                uih_offsets=uih_offsets, target_offsets=target_offsets, seq_embeddings=seq_embeddings,
                seq_payloads=seq_payloads, dtype=seq_embeddings.dtype)
            action_embeddings = self._action_embedding_mlp(
                seq_embeddings=action_embeddings, seq_offsets=seq_offsets, max_seq_len=max_seq_len,
                contextual_embeddings=pmlp_contextual_embeddings)
            if action_embeddings.dtype != content_embeddings.dtype:
                action_embeddings = action_embeddings.to(content_embeddings.dtype)
            if contextual_embeddings is not None and contextual_embeddings.dtype != content_embeddings.dtype:
                contextual_embeddings = contextual_embeddings.to(content_embeddings.dtype)

            return self.combine_embeddings(
                max_uih_len=max_uih_len, max_targets=max_targets, total_uih_len=total_uih_len, total_targets=total_targets,
                seq_lengths=seq_lengths, seq_timestamps=seq_timestamps, content_embeddings=content_embeddings,
                action_embeddings=action_embeddings, contextual_embeddings=contextual_embeddings, num_targets=num_targets,
                seq_offsets=seq_offsets) + (seq_payloads,)

    def interleave_targets(self) -> bool:
        return self.is_train and self._enable_interleaving
