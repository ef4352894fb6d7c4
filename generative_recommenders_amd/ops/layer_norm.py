"""Drop-in for generative_recommenders/ops/layer_norm.py on the HIP row kernels (fp32 math, affine; backward returns dx,
dweight, dbias): ``layer_norm`` (:46-76), ``swish_layer_norm`` (:79-112: x * sigmoid(LayerNorm(x))), ``rms_norm`` and the
modules that own the parameters, ``LayerNorm`` (:112-136), ``RMSNorm`` (:139-158) and ``SwishLayerNorm`` (:161-186)."""

from typing import List, Optional

import torch

from generative_recommenders_amd.common import HammerKernel, HammerModule
from generative_recommenders_amd.ops import _launch


class _LayerNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        y, mean, rstd = _launch.layer_norm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.wdtype, ctx.bdtype = weight.dtype, bias.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        dx, dw, db = _launch.layer_norm_bwd(dy, x, weight, mean, rstd)
        return dx, dw.to(ctx.wdtype), db.to(ctx.bdtype), None


def layer_norm(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    eps: float = 1e-5,
    kernel: HammerKernel = HammerKernel.HIP,
) -> torch.Tensor:
    del kernel
    shape = x.shape
    y = _LayerNormFunction.apply(x.reshape(-1, shape[-1]), weight, bias, eps)
    return y.view(shape)


class _SwishLayerNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        y, mean, rstd = _launch.swish_layer_norm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mean, rstd = ctx.saved_tensors
        dx, dw, db = _launch.swish_layer_norm_bwd(dy, x, weight, bias, mean, rstd)
        return dx, dw.to(weight.dtype), db.to(bias.dtype), None


def swish_layer_norm(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    eps: float = 1e-5,
    kernel: HammerKernel = HammerKernel.HIP,
) -> torch.Tensor:
    """``x * sigmoid(layer_norm(x))`` in one pass (reference: ops/layer_norm.py:79-112)."""
    del kernel
    shape = x.shape
    y = _SwishLayerNormFunction.apply(x.reshape(-1, shape[-1]), weight, bias, eps)
    return y.view(shape)


class _RMSNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        y, rstd = _launch.rms_norm_fwd(x, weight, eps)
        ctx.save_for_backward(x, weight, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, rstd = ctx.saved_tensors
        dx, dw = _launch.rms_norm_bwd(dy, x, weight, rstd)
        return dx, dw.to(weight.dtype), None


def rms_norm(
    x: torch.Tensor,
    weight: torch.Tensor,
    eps: float = 1e-5,
    kernel: HammerKernel = HammerKernel.HIP,
) -> torch.Tensor:
    """``x * rsqrt(mean(x^2, -1) + eps) * weight`` in one pass, with the semantics of the reference's Triton kernels
    (ops/triton/triton_layer_norm.py:525-749), as ``layer_norm`` has them: fp32 math, one rounding at the store, the output
    in ``x``'s dtype.  (The reference's PyTorch branch, ``RMSNorm.forward`` :153-158, rounds the normalised value to ``x``'s
    dtype before the weight multiply and returns the promoted dtype of that product; for fp32 input the two agree.)"""
    del kernel
    shape = x.shape
    y = _RMSNormFunction.apply(x.reshape(-1, shape[-1]), weight, eps)
    return y.view(shape)


class LayerNorm(HammerModule):
    """ops/layer_norm.py:115-142: owns ``weight`` (ones) and ``bias`` (zeros) of shape (dim,)"""

    def __init__(self, dim: int, eps: float = 1e-5, is_inference: bool = False) -> None:
        super().__init__(is_inference=is_inference)
        self._normalized_shape: List[int] = [dim]
        self._eps = eps
        self.weight = torch.nn.Parameter(torch.ones(self._normalized_shape))
        self.bias = torch.nn.Parameter(torch.zeros(self._normalized_shape))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return layer_norm(x=x, weight=self.weight, bias=self.bias, eps=self._eps, kernel=self.hammer_kernel())


class RMSNorm(HammerModule):
    """ops/layer_norm.py:139-158: owns ``weight`` (ones) of shape (dim,), no bias; runs ``rms_norm`` (the Triton branch's
    semantics, see there)"""

    def __init__(self, dim: int, eps: float = 1e-5, is_inference: bool = False) -> None:
        super().__init__(is_inference=is_inference)
        self._eps = eps
        self.weight = torch.nn.Parameter(torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return rms_norm(x=x, weight=self.weight, eps=self._eps, kernel=self.hammer_kernel())


class SwishLayerNorm(HammerModule):
    """ops/layer_norm.py:162-186"""

    def __init__(self, dim: int, eps: float = 1e-5, is_inference: bool = False) -> None:
        super().__init__(is_inference=is_inference)
        self._normalized_shape: List[int] = [dim]
        self.weight = torch.nn.Parameter(torch.ones(self._normalized_shape))
        self.bias = torch.nn.Parameter(torch.zeros(self._normalized_shape))
        self._eps = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return swish_layer_norm(x=x, weight=self.weight, bias=self.bias, eps=self._eps, kernel=self.hammer_kernel())
