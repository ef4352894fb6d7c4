"""Mixture-of-Logits scoring on csrc/mol_ops.hip: the (B, X, L) logits and the gating MLP's (B, X, H) hidden layer of
research/rails/similarities/mol/similarity_fn.py live in registers and LDS; only the (B, X) scores reach memory."""

from typing import Optional

import torch

from generative_recommenders_amd.ops import _launch

MOL_MAX_LOGITS, MOL_MAX_DIM, MOL_MAX_HIDDEN = _launch.MOL_MAX_LOGITS, _launch.MOL_MAX_DIM, _launch.MOL_MAX_HIDDEN
MOL_COMBINATIONS = tuple(_launch.MOL_COMBINATIONS)


def mol_check_limits(num_query_groups: int, num_item_groups: int, dim: int, hidden: int) -> None:
    """``ValueError`` naming the limit of hstu_mol_scores a shape exceeds"""
    if num_query_groups < 1 or num_item_groups < 1 or num_query_groups * num_item_groups > MOL_MAX_LOGITS:
        raise ValueError(f"MoL: {num_query_groups} x {num_item_groups} logits exceed the fused kernel's limit "
                         f"P_Q * P_X <= {MOL_MAX_LOGITS}")
    if dim < 1 or dim > MOL_MAX_DIM:
        raise ValueError(f"MoL: dot product dimension {dim} exceeds the fused kernel's limit 1 <= D_P <= {MOL_MAX_DIM}")
    if hidden < 0 or hidden > MOL_MAX_HIDDEN:
        raise ValueError(f"MoL: {hidden} hidden units of the gating MLP exceed the fused kernel's limit H <= {MOL_MAX_HIDDEN}")


def mol_pad_components(c: torch.Tensor) -> torch.Tensor:
    """(.., P, D) component embeddings with D zero-padded to the kernel's unit of 8 (a dot product does not change)"""
    pad = -c.shape[-1] % 8
    return (torch.nn.functional.pad(c, (0, pad)) if pad else c).contiguous()


def mol_scores(qc: torch.Tensor, xc: torch.Tensor, gq: torch.Tensor, gi: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor],
               w2: Optional[torch.Tensor], b2: torch.Tensor, temperature: float, combination: str = "glu_silu") -> torch.Tensor:
    """(B, X) fp32 scores: softmax(gate(gq[b] * gi[x] + MLP(l)))-weighted sum of the logits l[n P_X + m] =
    <qc[b, n], xc[x, m]> / temperature.  MLP(l) = w2 silu(w1 l + b1) + b2, or w1 l + b2 when b1 and w2 are None;
    gate = ``glu_silu`` or ``glu_silu_ln``.  One dtype (bf16 / fp16 / fp32) for all operands, fp32 arithmetic."""
    if qc.dim() == 3 and xc.dim() == 3:
        mol_check_limits(qc.shape[1], xc.shape[1], qc.shape[2], w1.shape[0] if w2 is not None else 0)
    return _launch.mol_scores(mol_pad_components(qc), mol_pad_components(xc), gq, gi, w1, b1, w2, b2, 1.0 / temperature, combination)
