"""The compute of ``TimestampLayerNormPostprocessor`` (generative_recommenders/modules/postprocessors.py:105-176):
``LayerNorm(Linear(cat([x, time_features(t)], -1)))``.  Writing the combiner weight as ``W = [Wx | Wt]`` splits it into the
aligned GEMM ``z0 = x Wx^T`` (``hstu_linear_k512`` at D = 512, hipBLASLt otherwise) and ONE row pass over z0: the time
features of the row's timestamp, the rank-2F update ``tf Wt^T``, the bias and the LayerNorm (csrc/time_ln_ops.hip).  The
(rows, D + 2F) concatenation -- a full copy to a row stride that is no 16-byte multiple -- and the LayerNorm's own pass are
never made; the backward recomputes z from z0 and the timestamps.

``F`` outside 1..4 or a row wider than the kernels' class limit runs ``timestamp_layer_norm_composed``: the same result from
this package's ops (``hstu_time_features`` -> cat -> addmm -> layer_norm), which is also the benchmark's baseline
(tools/bench_timestamp_postprocessor.py)."""

import torch

from generative_recommenders_amd.ops import _launch
from generative_recommenders_amd.ops.layer_norm import layer_norm
from generative_recommenders_amd.ops.mm import weight_grad_mm


def _num_periods(period_units: torch.Tensor) -> int:
    return int(period_units.numel())


class _TimestampLayerNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, timestamps, weight, bias, ln_weight, ln_bias, period_units, units_per_period, eps):
        dim = x.shape[1]
        x = x.contiguous()
        # Wx: the (D, D) K-contiguous block in x's dtype; Wt: the 2F time columns, transposed, fp32
        wx = weight.detach()[:, :dim].to(x.dtype).contiguous()
        wt = weight.detach()[:, dim:].t().to(torch.float32).contiguous()
        if _launch.linear_k512_supported(x, dim):
            z0 = _launch.linear_k512(x, wx)
        else:
            z0 = torch.mm(x, wx.t())
        b = bias.detach() if bias is not None else torch.zeros(dim, dtype=torch.float32, device=x.device)
        y, mean, rstd = _launch.time_ln_fwd(z0, timestamps, period_units, units_per_period, b, wt, ln_weight.detach(),
                                            ln_bias.detach(), eps)
        ctx.save_for_backward(x, z0, timestamps, wx, wt, b, ln_weight, mean, rstd, period_units, units_per_period)
        ctx.dtypes = (weight.dtype, None if bias is None else bias.dtype, ln_weight.dtype, ln_bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, z0, timestamps, wx, wt, b, ln_weight, mean, rstd, period_units, units_per_period = ctx.saved_tensors
        w_dtype, b_dtype, g_dtype, h_dtype = ctx.dtypes
        dz, dg, dh, db, dwt = _launch.time_ln_bwd(dy, z0, timestamps, period_units, units_per_period, b, wt, ln_weight.detach(),
                                                  mean, rstd)
        dx = torch.mm(dz, wx) if ctx.needs_input_grad[0] else None
        dweight = None
        if ctx.needs_input_grad[2]:
            # d Wx = dz^T x (the contraction runs over all rows: the split weight-gradient GEMM), d W = [d Wx | d Wt^T]
            dwx = weight_grad_mm(dz, x, out_dtype=torch.float32)
            dweight = torch.cat([dwx, dwt.t()], dim=1).to(w_dtype)
        dbias = db.to(b_dtype) if b_dtype is not None and ctx.needs_input_grad[3] else None
        return dx, None, dweight, dbias, dg.to(g_dtype), dh.to(h_dtype), None, None, None


def timestamp_layer_norm_composed(x, timestamps, weight, bias, ln_weight, ln_bias, period_units, units_per_period,
                                  eps: float = 1e-5) -> torch.Tensor:
    """the unfused composition on this package's ops: time features (HIP), cat, addmm, layer_norm (HIP)"""
    rows = x
    if _num_periods(period_units) > 0:
        rows = torch.cat([x, _launch.time_features(timestamps, period_units, units_per_period).to(x.dtype)], dim=-1)
    w = weight.to(x.dtype)
    if bias is not None:
        z = torch.addmm(bias.to(x.dtype), rows, w.t())
    else:
        z = torch.mm(rows, w.t())
    return layer_norm(z, ln_weight, ln_bias, eps)


def timestamp_layer_norm(x: torch.Tensor, timestamps: torch.Tensor, weight: torch.Tensor, bias, ln_weight: torch.Tensor,
                         ln_bias: torch.Tensor, period_units: torch.Tensor, units_per_period: torch.Tensor,
                         eps: float = 1e-5) -> torch.Tensor:
    """``x`` (rows, D) in bf16 / fp16 / fp32, ``timestamps`` (rows) integers, ``weight`` (D, D + 2F) and ``bias`` (D) of the
    combiner, ``ln_weight`` / ``ln_bias`` (D), ``period_units`` / ``units_per_period`` F numbers each (the module's
    buffers).  Returns (rows, D) in x's dtype.  A non-contiguous x is copied to contiguous rows first."""
    _launch.L.require_gpu_tensor(x, "x")
    torch._assert(x.dim() == 2 and timestamps.numel() == x.shape[0], "x must be (rows, D) with one timestamp per row")
    f = _num_periods(period_units)
    torch._assert(weight.shape == (x.shape[1], x.shape[1] + 2 * f), "weight must be (D, D + 2F)")
    if not _launch.time_ln_supported(x.shape[1], f, x.dtype):
        return timestamp_layer_norm_composed(x, timestamps, weight, bias, ln_weight, ln_bias, period_units, units_per_period, eps)
    return _TimestampLayerNormFunction.apply(x, timestamps, weight, bias, ln_weight, ln_bias, period_units, units_per_period, eps)
