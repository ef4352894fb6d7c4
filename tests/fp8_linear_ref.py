"""Restatement of the row-wise e4m3 UVQK projection's arithmetic (include/hstu_hip.h: hstu_quantize_rows_fp8,
hstu_ln_linear_fp8_fwd, hstu_linear_fp8_rowwise) in torch on the CPU -- fp64 wherever something is summed.  Not a test
module: the tests of the entry points import it.

  nx[r,:]    = LayerNorm(x[r,:]) ln_w + ln_b                       (fp64 here, handed to the quantizer as fp32)
  x_scale[r] = max_k |nx[r,k]| / 448   (1 for a zero row)           fp32, IEEE division
  xq[r,k]    = e4m3_rne(clamp(nx[r,k] / x_scale[r], -448, 448))     OCP e4m3fn
  y[r,n]     = (sum_k xq[r,k] wq[n,k]) x_scale[r] w_scale[n] + bias[n]
"""

import torch

FP8 = torch.float8_e4m3fn
E4M3_MAX = 448.0


def quantize_rows(src: torch.Tensor):
    """(codes, scale) of the rows of a 2-D tensor: the rule of the C entry point, on fp32 values"""
    a = src.detach().cpu().float()
    amax = a.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    q = (a / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(FP8)
    return q, scale


def layer_norm_f64(x, ln_w, ln_b, eps):
    """(nx, mean, rstd) in fp64 from the 16-bit operands as they are"""
    xd = x.detach().cpu().double()
    mean = xd.mean(dim=1)
    var = ((xd - mean[:, None]) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + eps)
    nx = (xd - mean[:, None]) * rstd[:, None] * ln_w.detach().cpu().double() + ln_b.detach().cpu().double()
    return nx, mean, rstd


def ln_quantize(x, ln_w, ln_b, eps):
    """(xq, x_scale, mean, rstd): the fused kernel's prologue"""
    nx, mean, rstd = layer_norm_f64(x, ln_w, ln_b, eps)
    xq, xs = quantize_rows(nx.float())
    return xq, xs, mean, rstd


def product(xq, x_scale, wq, w_scale, bias=None):
    """y in fp64 from codes and scales; wq is the (n, k) K-contiguous table"""
    acc = xq.detach().cpu().double() @ wq.detach().cpu().double().t()
    y = acc * x_scale.detach().cpu().double()[:, None] * w_scale.detach().cpu().double()[None, :]
    return y if bias is None else y + bias.detach().cpu().double()


def exact_product(x, ln_w, ln_b, eps, w_nk, bias=None):
    """the unquantized LayerNorm(x) W^T + b in fp64; w_nk is the (n, k) 16-bit weight"""
    nx, _, _ = layer_norm_f64(x, ln_w, ln_b, eps)
    y = nx @ w_nk.detach().cpu().double().t()
    return y if bias is None else y + bias.detach().cpu().double()


def rel_fro(got, ref) -> float:
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((g - r).norm() / max(float(r.norm()), 1e-300))


def code_order(q: torch.Tensor) -> torch.Tensor:
    """e4m3 codes as integers in value order (+0 and -0 both 0): neighbouring values differ by one"""
    c = q.detach().cpu().view(torch.uint8).to(torch.int32)
    mag = c & 0x7F
    return torch.where((c & 0x80) != 0, -mag, mag)
