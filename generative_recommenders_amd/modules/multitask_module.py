"""Drop-in for generative_recommenders/modules/multitask_module.py: ``MultitaskTaskType``, ``TaskConfig``,
``MultitaskModule`` and ``DefaultMultitaskModule`` (:30-277) with the reference's constructor arguments, asserts,
``state_dict`` names and four-tuple return.

With the prediction module DlrmHSTU builds (modules/dlrm_hstu.py:139-149: Linear -> SwishLayerNorm -> Linear) the first
projection is a GEMM on u * i in the training dtype and EVERYTHING behind it -- the gate, the task projection, the
sigmoid, the weighted losses and their normalisation -- is one HIP row pass (ops/multitask.py) with fp32 math, so no
autocast context is involved.  Any other ``prediction_fn`` runs as given, followed by the same formulas in torch."""

import abc
from dataclasses import dataclass
from enum import IntEnum
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from generative_recommenders_amd.common import HammerModule
from generative_recommenders_amd.ops import _launch
from generative_recommenders_amd.ops.layer_norm import SwishLayerNorm
from generative_recommenders_amd.ops.mm import addmm
from generative_recommenders_amd.ops.multitask import multitask_head


class MultitaskTaskType(IntEnum):
    BINARY_CLASSIFICATION = 0
    REGRESSION = 1


@dataclass
class TaskConfig:
    task_name: str
    task_weight: int
    task_type: MultitaskTaskType


class MultitaskModule(HammerModule):
    @abc.abstractmethod
    def forward(
        self,
        encoded_user_embeddings: torch.Tensor,
        item_embeddings: torch.Tensor,
        supervision_labels: Dict[str, torch.Tensor],
        supervision_weights: Dict[str, torch.Tensor],
    ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
        """
        Args:
            encoded_user_embeddings: (L, D) x float.
            item_embeddings: (L, D) x float.
            supervision_labels: Dict[T, L] x float or int
            supervision_weights: Dict[T', L] x float or int, T' <= T
        Returns:
            (T, L) x float, predictions, labels, weights, losses
        """
        pass


def _compute_labels_and_weights(
    supervision_labels: Dict[str, torch.Tensor],
    supervision_weights: Dict[str, torch.Tensor],
    task_configs: List[TaskConfig],
    device: torch.device,
    dtype: torch.dtype = torch.float32,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """multitask_module.py:107-133: (T, L) labels and weights in task order; a task without weights gets ones"""
    first_label = list(supervision_labels.values())[0]
    default_supervision_weight = torch.ones_like(first_label, dtype=dtype, device=device)
    labels = [supervision_labels[task.task_name] for task in task_configs]
    weights = [supervision_weights.get(task.task_name, default_supervision_weight) for task in task_configs]
    if len(task_configs) > 1:
        return torch.stack(labels, dim=0), torch.stack(weights, dim=0)
    return labels[0].unsqueeze(0), weights[0].unsqueeze(0)


def _preds_from_logits(mt_logits: torch.Tensor, num_binary: int) -> torch.Tensor:
    """multitask_module.py:80-104: sigmoid on the binary rows, the regression rows as they are"""
    tasks = mt_logits.shape[0]
    if num_binary == tasks:
        return torch.sigmoid(mt_logits)
    if num_binary == 0:
        return mt_logits
    return torch.concat([torch.sigmoid(mt_logits[:num_binary]), mt_logits[num_binary:]], dim=0)


def _losses_from_logits(mt_logits: torch.Tensor, mt_labels: torch.Tensor, mt_weights: torch.Tensor, num_binary: int,
                        causal_multitask_weights: float) -> torch.Tensor:
    """multitask_module.py:136-191"""
    parts = []
    if num_binary > 0:
        parts.append(F.binary_cross_entropy_with_logits(input=mt_logits[:num_binary], target=mt_labels[:num_binary],
                                                        reduction="none") * mt_weights[:num_binary])
    if num_binary < mt_logits.shape[0]:
        parts.append(F.mse_loss(mt_logits[num_binary:], mt_labels[num_binary:], reduction="none") * mt_weights[num_binary:])
    mt_losses = parts[0] if len(parts) == 1 else torch.concat(parts, dim=0)
    return mt_losses.sum(-1) / mt_weights.sum(-1).clamp(min=1.0) * causal_multitask_weights


class DefaultMultitaskModule(MultitaskModule):
    def __init__(
        self,
        task_configs: List[TaskConfig],
        embedding_dim: int,
        prediction_fn: Callable[[int, int], torch.nn.Module],
        causal_multitask_weights: float,
        is_inference: bool,
    ) -> None:
        super().__init__(is_inference)
        assert (
            sorted(task_configs, key=lambda x: x.task_type) == task_configs
        ), "task_configs must be sorted by task_type."
        assert len(task_configs) > 0, "task_configs must be non-empty."
        self._task_configs: List[TaskConfig] = task_configs
        self._task_offsets: List[int] = [0] * (len(MultitaskTaskType) + 1)
        for task in self._task_configs:
            self._task_offsets[task.task_type + 1] += 1
        self._has_multiple_task_types: bool = self._task_offsets.count(0) < len(MultitaskTaskType)
        self._task_offsets[1:] = np.cumsum(self._task_offsets[1:]).tolist()
        self._causal_multitask_weights: float = causal_multitask_weights
        self._prediction_module: torch.nn.Module = prediction_fn(embedding_dim, len(task_configs))

    def _fused_layers(self, x: torch.Tensor):
        """(Linear, SwishLayerNorm, Linear) when the prediction module is that chain and the kernel takes its shapes"""
        pm = self._prediction_module
        if not (isinstance(pm, torch.nn.Sequential) and len(pm) == 3 and isinstance(pm[0], torch.nn.Linear)
                and isinstance(pm[1], SwishLayerNorm) and isinstance(pm[2], torch.nn.Linear)):
            return None
        if not (x.is_cuda and pm[0].weight.is_cuda and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16, torch.float32)):
            return None
        hidden, tasks = pm[0].out_features, pm[2].out_features
        es = x.element_size()
        if not 1 <= tasks <= _launch.MULTITASK_MAX_TASKS or hidden > (4096 if hidden % (16 // es) == 0 else 2048):
            return None
        return pm[0], pm[1], pm[2]

    def forward(
        self,
        encoded_user_embeddings: torch.Tensor,
        item_embeddings: torch.Tensor,
        supervision_labels: Dict[str, torch.Tensor],
        supervision_weights: Dict[str, torch.Tensor],
    ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
        orig_dtype = encoded_user_embeddings.dtype
        if not self._is_inference:
            encoded_user_embeddings = encoded_user_embeddings.to(self._training_dtype)
            item_embeddings = item_embeddings.to(self._training_dtype)
        num_binary = self._task_offsets[MultitaskTaskType.BINARY_CLASSIFICATION + 1]

        mt_labels: Optional[torch.Tensor] = None
        mt_weights: Optional[torch.Tensor] = None
        mt_losses: Optional[torch.Tensor] = None
        if not self._is_inference:
            mt_labels, mt_weights = _compute_labels_and_weights(
                supervision_labels=supervision_labels,
                supervision_weights=supervision_weights,
                task_configs=self._task_configs,
                device=encoded_user_embeddings.device,
            )

        fused = self._fused_layers(encoded_user_embeddings)
        if fused is not None:
            lin_in, norm, lin_out = fused
            x = encoded_user_embeddings * item_embeddings
            dt = x.dtype
            if lin_in.bias is not None:
                hidden = addmm(lin_in.bias.to(dt), x, lin_in.weight.to(dt).t())
            else:
                hidden = torch.mm(x, lin_in.weight.to(dt).t())
            out_bias = lin_out.bias if lin_out.bias is not None else lin_out.weight.new_zeros(lin_out.out_features)
            mt_preds, mt_losses = multitask_head(
                hidden, norm.weight, norm.bias, norm._eps, lin_out.weight, out_bias, mt_labels, mt_weights, num_binary,
                self._causal_multitask_weights)
            # (the reference's predictions leave the prediction module in its compute dtype)
            mt_preds = mt_preds.to(orig_dtype if not self._is_inference else dt)
        else:
            # losses are always computed in fp32; the autocast is what lets an fp32 module take bf16 activations
            with torch.autocast("cuda", dtype=torch.bfloat16,
                                enabled=(not self.is_inference and self._training_dtype == torch.bfloat16)):
                mt_logits = self._prediction_module(encoded_user_embeddings * item_embeddings).transpose(0, 1)
                mt_preds = _preds_from_logits(mt_logits, num_binary)
            if not self._is_inference:
                mt_losses = _losses_from_logits(mt_logits.to(mt_labels.dtype), mt_labels, mt_weights, num_binary,
                                                self._causal_multitask_weights)
                mt_preds = mt_preds.to(orig_dtype)

        return mt_preds, mt_labels, mt_weights, mt_losses
