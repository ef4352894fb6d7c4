"""Embedding tables trained in backward: the sparse row-wise Adagrad the reference's DLRM-v3 configurations apply through
``apply_optimizer_in_backward`` (dlrm_v3/train/utils.py:190-227; TorchRec's ``RowWiseAdagrad`` / fbgemm's exact row-wise
Adagrad with ``weight_decay = 0`` and ``lr_decay = 0``).  For every table row r among the batch's ids, and only those:

    G[r, :]      = sum over i with idx[i] == r of dout[i, :]                       (fp32)
    momentum1[r] = momentum1[r] + mean_d(G[r, d]^2)
    W[r, :]      = W[r, :] - lr / (sqrt(momentum1[r]) + eps) * G[r, :]              (the updated momentum1)

One HIP pass (csrc/embedding_optim.hip) that reads the gradient rows and touches only those table rows: no table-sized
gradient exists at any point."""

import ctypes as C
from typing import Any, Optional

import torch

from generative_recommenders_amd import _lib as L


class RowWiseAdagradConfig:
    """step size, epsilon and the dtype of the gathered rows (None: the table's) of one fused table; mutable, read at every
    forward / backward (``set_learning_rate``)"""

    def __init__(self, lr: float, eps: float = 1e-8, rows_dtype: Optional[torch.dtype] = None) -> None:
        self.lr = float(lr)
        self.eps = float(eps)
        self.rows_dtype = rows_dtype


def rowwise_adagrad_update_(weight: torch.Tensor, momentum1: torch.Tensor, idx: torch.Tensor, dout: torch.Tensor, lr: float,
                            eps: float = 1e-8) -> None:
    """in place: the update above on ``weight`` (rows, dim) fp32 and ``momentum1`` (rows) fp32 for the ids ``idx`` (n) and
    their gradient rows ``dout`` (n, dim) in bf16, fp16 or fp32.  Ids outside [0, rows) are the caller's error (not checked)."""
    for name, t in (("weight", weight), ("momentum1", momentum1), ("idx", idx), ("dout", dout)):
        L.require_gpu_tensor(t, name)
    if not (weight.device == momentum1.device == idx.device == dout.device):
        raise RuntimeError(f"rowwise_adagrad_update_: weight, momentum1, idx and dout must be on one device, got {weight.device}, "
                           f"{momentum1.device}, {idx.device} and {dout.device}")
    if weight.dtype != torch.float32 or momentum1.dtype != torch.float32:
        raise RuntimeError(f"rowwise_adagrad_update_: weight and momentum1 must be float32 (TorchRec keeps fused tables in fp32), "
                           f"got {weight.dtype} and {momentum1.dtype}")
    if not weight.is_contiguous() or not momentum1.is_contiguous():
        raise RuntimeError("rowwise_adagrad_update_: weight and momentum1 must be contiguous (they are updated in place)")
    if weight.dim() != 2 or momentum1.shape != (weight.shape[0],):
        raise RuntimeError(f"rowwise_adagrad_update_: weight (rows, dim) and momentum1 (rows), got {tuple(weight.shape)} and "
                           f"{tuple(momentum1.shape)}")
    rows, dim = weight.shape
    if dout.dim() != 2 or dout.shape[1] != dim or idx.dim() != 1 or idx.shape[0] != dout.shape[0]:
        raise RuntimeError(f"rowwise_adagrad_update_: idx (n) and dout (n, {dim}), got {tuple(idx.shape)} and {tuple(dout.shape)}")
    n = idx.shape[0]
    if n == 0:
        return
    dout = dout.detach().contiguous()
    idx = idx.detach().to(torch.int32).contiguous()
    need = C.c_int64(0)
    L.check(L.lib().hstu_embedding_rowwise_adagrad_workspace_bytes(n, rows, C.byref(need)))
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=weight.device)
    with torch.cuda.device(weight.device):
        L.check(L.lib().hstu_embedding_rowwise_adagrad(
            dout.data_ptr(), idx.data_ptr(), n, dim, rows, weight.data_ptr(), momentum1.data_ptr(), float(lr), float(eps),
            ws.data_ptr(), ws.numel(), L.torch_dtype_code(dout.dtype), L.current_stream_ptr(weight.device)))


def _refuse_replicated_tables() -> None:
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(
            "in-backward row-wise Adagrad updates each rank's copy of the table with that rank's gradient: replicated tables "
            f"would diverge, and sharded tables are out of scope (world size {dist.get_world_size()})")


class _GatherRowsFusedFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, momentum1, idx, cfg, rows_dtype):
        ctx.save_for_backward(idx)
        ctx.table = (weight, momentum1, cfg)        # the parameter and its state themselves: the update is in place
        rows = weight.index_select(0, idx)
        return rows if rows_dtype is None else rows.to(rows_dtype)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        weight, momentum1, cfg = ctx.table
        _refuse_replicated_tables()
        with torch.no_grad():
            rowwise_adagrad_update_(weight, momentum1, idx, g, cfg.lr, cfg.eps)
        return None, None, None, None, None


def gather_rows_fused(weight: torch.Tensor, momentum1: torch.Tensor, idx: torch.Tensor, cfg: Any,
                      rows_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``weight[idx]`` (cast to ``rows_dtype`` when given) whose backward applies the row-wise Adagrad step of ``cfg`` (``lr``,
    ``eps``) to ``weight`` and ``momentum1`` in place and hands autograd no gradient for the table: ``weight.grad`` stays None."""
    return _GatherRowsFusedFunction.apply(weight, momentum1, idx, cfg, rows_dtype)
