"""The multitask prediction head behind the first projection as ONE row pass (hstu_multitask_head_fwd / _bwd):

    y = x * sigmoid(LayerNorm(x));  logits = y W^T + c;  preds = sigmoid(logits) | logits;  per-task weighted losses

-- what the reference runs as SwishLayerNorm + Linear + a trail of (T, L) torch ops in DefaultMultitaskModule
(modules/multitask_module.py:70-104, :136-191).  fp32 math throughout, whatever x's dtype: no autocast is involved."""

from typing import Optional, Tuple

import torch

from generative_recommenders_amd.ops import _launch


class _MultitaskHeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ln_weight, ln_bias, eps, weight, bias, labels, weights, num_binary_tasks, loss_scale):
        logits, preds, mean, rstd, loss, wsum = _launch.multitask_head_fwd(
            x, ln_weight, ln_bias, eps, weight, bias, labels, weights, num_binary_tasks, loss_scale)
        ctx.save_for_backward(x, ln_weight, ln_bias, weight, bias, labels, weights, logits, mean, rstd, wsum)
        ctx.num_binary_tasks, ctx.loss_scale = num_binary_tasks, loss_scale
        ctx.set_materialize_grads(False)
        if loss is None:
            loss = preds.new_empty(0)
            ctx.mark_non_differentiable(loss)
        return preds, loss

    @staticmethod
    def backward(ctx, grad_pred, grad_loss):
        x, ln_weight, ln_bias, weight, bias, labels, weights, logits, mean, rstd, wsum = ctx.saved_tensors
        if labels is None:
            grad_loss = None
        if grad_pred is None and grad_loss is None:
            return (None,) * 10
        dx, dw, dc, dg, db = _launch.multitask_head_bwd(grad_loss, grad_pred, x, ln_weight, ln_bias, weight, labels, weights,
                                                        logits, mean, rstd, wsum, ctx.num_binary_tasks, ctx.loss_scale)
        return (dx, dg.to(ln_weight.dtype), db.to(ln_bias.dtype), None, dw.to(weight.dtype), dc.to(bias.dtype), None, None,
                None, None)


def multitask_head(
    x: torch.Tensor,
    ln_weight: torch.Tensor,
    ln_bias: torch.Tensor,
    eps: float,
    weight: torch.Tensor,
    bias: torch.Tensor,
    labels: Optional[torch.Tensor],
    weights: Optional[torch.Tensor],
    num_binary_tasks: int,
    loss_scale: float,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """x (L, dim) bf16 / fp16 / fp32; ln_weight, ln_bias (dim); weight (T, dim), bias (T): the task projection; labels,
    weights (T, L) or None (weights None: all ones; labels None: inference, no losses).  The first ``num_binary_tasks``
    tasks are binary classification, the rest regression.  Returns preds (T, L) fp32 and losses (T) fp32 or None:
    losses[t] = sum_l weights * loss / max(sum_l weights, 1) * loss_scale.  Gradients flow from both outputs to x and the
    four parameters."""
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1] or bias.shape != (weight.shape[0],):
        raise RuntimeError(f"multitask_head: x (L, dim), weight (T, dim), bias (T) expected, got {tuple(x.shape)}, "
                           f"{tuple(weight.shape)}, {tuple(bias.shape)}")
    tasks = weight.shape[0]
    if not 0 <= num_binary_tasks <= tasks:
        raise RuntimeError(f"multitask_head: num_binary_tasks = {num_binary_tasks} with {tasks} tasks")
    for name, t in (("labels", labels), ("weights", weights)):
        if t is not None and tuple(t.shape) != (tasks, x.shape[0]):
            raise RuntimeError(f"multitask_head: {name} must be (T, L) = ({tasks}, {x.shape[0]}), got {tuple(t.shape)}")
    if weights is not None and labels is None:
        raise RuntimeError("multitask_head: weights without labels")
    preds, loss = _MultitaskHeadFunction.apply(x, ln_weight, ln_bias, eps, weight, bias, labels, weights, num_binary_tasks,
                                               loss_scale)
    return preds, (None if labels is None else loss)
