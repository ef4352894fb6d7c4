"""Drop-in for generative_recommenders/modules/action_encoder.py:27-112 (``ActionEncoder``): same constructor, buffer and
parameter names (``_combined_action_weights``, ``_action_embedding_table``, ``_target_action_embedding_table``) and forward
signature.  The forward is ONE HIP row pass (ops/preprocess.py ``action_encode``) instead of two bit ops, a
(rows, T, Da) product, a tile and ``concat_2D_jagged``; the weights and watchtime thresholds travel as kernel arguments
(the python lists the constructor got -- the buffer is kept for the state_dict and never read back)."""

from typing import Dict, List, Optional, Tuple

import torch

from generative_recommenders_amd.common import HammerModule
from generative_recommenders_amd.ops.preprocess import action_encode


class ActionEncoder(HammerModule):
    def __init__(
        self,
        action_embedding_dim: int,
        action_feature_name: str,
        action_weights: List[int],
        watchtime_feature_name: str = "",
        watchtime_to_action_thresholds_and_weights: Optional[List[Tuple[int, int]]] = None,
        is_inference: bool = False,
    ) -> None:
        super().__init__(is_inference=is_inference)
        self._watchtime_feature_name: str = watchtime_feature_name
        self._action_feature_name: str = action_feature_name
        self._watchtime_to_action_thresholds_and_weights: List[Tuple[int, int]] = (
            watchtime_to_action_thresholds_and_weights if watchtime_to_action_thresholds_and_weights is not None else []
        )
        self._combined_action_weight_list: List[int] = [int(w) for w in action_weights] + [
            int(x[1]) for x in self._watchtime_to_action_thresholds_and_weights]
        self.register_buffer("_combined_action_weights", torch.tensor(self._combined_action_weight_list))
        self._num_action_types: int = len(self._combined_action_weight_list)
        self._action_embedding_dim = action_embedding_dim
        self._action_embedding_table: torch.nn.Parameter = torch.nn.Parameter(
            torch.empty((self._num_action_types, action_embedding_dim)).normal_(mean=0, std=0.1),
        )
        self._target_action_embedding_table: torch.nn.Parameter = torch.nn.Parameter(
            torch.empty((1, self._num_action_types * action_embedding_dim)).normal_(mean=0, std=0.1),
        )

    @property
    def output_embedding_dim(self) -> int:
        return self._action_embedding_dim * self._num_action_types

    def encode(
        self,
        uih_offsets: torch.Tensor,
        target_offsets: torch.Tensor,
        seq_embeddings: torch.Tensor,
        seq_payloads: Dict[str, torch.Tensor],
        dtype: Optional[torch.dtype] = None,
    ) -> torch.Tensor:
        """forward with the output written in ``dtype`` directly (the preprocessors ask for the activation dtype: the
        reference's ``.to(seq_embeddings.dtype)`` behind the encoder costs no pass here)"""
        seq_actions = seq_payloads[self._action_feature_name]
        thresholds = self._watchtime_to_action_thresholds_and_weights
        watchtimes = seq_payloads[self._watchtime_feature_name] if len(thresholds) > 0 else None
        total_uih_len = seq_actions.numel()
        return action_encode(
            actions=seq_actions, watchtimes=watchtimes, uih_offsets=uih_offsets, target_offsets=target_offsets,
            table=self._action_embedding_table, target_table=self._target_action_embedding_table,
            action_weights=self._combined_action_weight_list, watchtime_to_action_thresholds_and_weights=thresholds,
            total_uih_len=total_uih_len, total_targets=seq_embeddings.size(0) - total_uih_len, dtype=dtype)

    def forward(
        self,
        max_uih_len: int,
        max_targets: int,
        uih_offsets: torch.Tensor,
        target_offsets: torch.Tensor,
        seq_embeddings: torch.Tensor,
        seq_payloads: Dict[str, torch.Tensor],
    ) -> torch.Tensor:
        return self.encode(uih_offsets, target_offsets, seq_embeddings, seq_payloads)
