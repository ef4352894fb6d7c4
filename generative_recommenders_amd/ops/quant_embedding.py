"""int8 row-wise quantized embedding tables for inference on csrc/quant_embedding.hip: what the reference's DLRM-v3 serving
flow makes of every table after loading the checkpoint (dlrm_v3/inference/model_family.py:122-143, ``quantize_dynamic`` to
``QuantEmbeddingCollection`` with int8 weights and float activations).

A quantized table of ``rows x dim`` is one uint8 tensor ``(rows, stride)`` -- fbgemm's "fused 8-bit row-wise" arithmetic with
row starts aligned for 16-byte loads (include/hstu_hip.h holds the format)::

    meta = round_up(dim, 4);  stride = round_up(meta + 8, 16)
    [0, dim) codes | [meta, meta + 4) fp32 scale | [meta + 4, meta + 8) fp32 bias | every other byte 0
    scale = (max - min) / 255, bias = min, code = clamp(rint((x - min) * (255 / (max - min + 1e-8))), 0, 255)
    value = code * scale + bias

GPU tensors go through the kernels; CPU tensors through the same formula in torch ops (``EmbeddingCollection`` works on the
CPU too), with every operation rounded to fp32 on its own."""

from typing import Optional

import torch

from generative_recommenders_amd import _lib as L

INT8_MAX_DIM = 2048
_FLOAT = (torch.float32, torch.float16, torch.bfloat16)


def int8_check_dim(dim: int) -> None:
    """``ValueError`` naming the limit of the int8 row kernels a row width exceeds"""
    if dim < 1 or dim > INT8_MAX_DIM:
        raise ValueError(f"int8 row-wise quantization: rows of {dim} columns are outside the kernels' limit 1 <= D <= {INT8_MAX_DIM}")


def _meta_offset(dim: int) -> int:
    return (dim + 3) // 4 * 4


def int8_row_stride(dim: int) -> int:
    """bytes of a quantized row of ``dim`` columns (``hstu_int8_row_stride``)"""
    int8_check_dim(dim)
    return (_meta_offset(dim) + 8 + 15) // 16 * 16


def _check_qweight(qweight: torch.Tensor, dim: int, who: str) -> None:
    int8_check_dim(dim)
    if qweight.dtype != torch.uint8 or qweight.dim() != 2:
        raise ValueError(f"{who}: qweight must be uint8 (rows, stride), got {qweight.dtype} {tuple(qweight.shape)}")
    if qweight.shape[1] < int8_row_stride(dim) or qweight.shape[1] % 16:
        raise ValueError(f"{who}: rows of {qweight.shape[1]} bytes do not hold {dim} columns: the stride must be a multiple of 16 and "
                         f"at least int8_row_stride({dim}) = {int8_row_stride(dim)}")
    if qweight.shape[0] >= 2**31:
        raise ValueError(f"{who}: {qweight.shape[0]} rows exceed the kernels' limit rows < 2^31")


def _fp32_bytes(x: torch.Tensor) -> torch.Tensor:
    """(rows) fp32 -> (rows, 4) uint8, little endian"""
    return x.contiguous().view(torch.uint8).view(-1, 4)


def quantize_rows_int8(weight: torch.Tensor) -> torch.Tensor:
    """``weight`` (rows, dim) in fp32, fp16 or bf16 -> its quantized table, uint8 (rows, int8_row_stride(dim))"""
    if weight.dim() != 2 or weight.dtype not in _FLOAT:
        raise ValueError(f"quantize_rows_int8: weight must be (rows, dim) in float32, float16 or bfloat16, got {weight.dtype} "
                         f"{tuple(weight.shape)}")
    rows, dim = weight.shape
    int8_check_dim(dim)
    if rows >= 2**31:
        raise ValueError(f"quantize_rows_int8: {rows} rows exceed the kernels' limit rows < 2^31")
    stride, meta = int8_row_stride(dim), _meta_offset(dim)
    weight = weight.detach()
    if weight.is_cuda:
        if weight.stride(1) != 1:
            weight = weight.contiguous()
        q = torch.empty((rows, stride), dtype=torch.uint8, device=weight.device)
        with torch.cuda.device(weight.device):
            L.check(L.lib().hstu_quantize_rows_int8(weight.data_ptr(), weight.stride(0), rows, dim, q.data_ptr(), stride,
                                                    L.torch_dtype_code(weight.dtype), L.current_stream_ptr(weight.device)))
        return q
    q = torch.zeros((rows, stride), dtype=torch.uint8)
    if rows == 0:
        return q
    x = weight.to(torch.float32)
    mn, mx = x.amin(dim=1), x.amax(dim=1)
    rng = mx - mn
    c255 = torch.full_like(rng, 255.0)                    # tensor operands: true fp32 divisions
    scale, inv = rng / c255, c255 / (rng + torch.full_like(rng, 1e-8))
    codes = torch.round((x - mn[:, None]) * inv[:, None]).clamp_(0.0, 255.0)       # torch.round: ties to even
    q[:, :dim] = codes.to(torch.uint8)
    q[:, meta:meta + 4] = _fp32_bytes(scale)
    q[:, meta + 4:meta + 8] = _fp32_bytes(mn)
    return q


def _scale_bias(qweight: torch.Tensor, dim: int):
    meta = _meta_offset(dim)
    sb = qweight[:, meta:meta + 8].contiguous().view(torch.float32)
    return sb[:, 0:1], sb[:, 1:2]


def gather_rows_int8(qweight: torch.Tensor, dim: int, idx: Optional[torch.Tensor], out_dtype: torch.dtype = torch.float32,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[i] = code * scale + bias`` of row ``idx[i]`` of the quantized table (fp32 arithmetic, 16-bit outputs rounded to
    nearest even) -> (n, dim) in ``out_dtype``.  ``idx``: int32 or int64 (n), or None for rows ``0 .. rows - 1`` in order.
    ``out``: write there instead -- (n, dim) with unit column stride, possibly a column slice of a wider tensor, every row
    16-byte aligned.  Without ``out``, GPU rows that are no multiple of 16 bytes come back as the leading columns of a padded
    buffer (a view with a longer row stride).  Ids outside the table are the caller's error: the kernel clamps them (memory safety), the CPU path
    raises as ``index_select`` does."""
    who = "gather_rows_int8"
    _check_qweight(qweight, dim, who)
    if out_dtype not in _FLOAT:
        raise ValueError(f"{who}: out_dtype must be float32, float16 or bfloat16, got {out_dtype}")
    if idx is not None:
        if idx.dim() != 1 or idx.dtype not in (torch.int32, torch.int64) or idx.device != qweight.device:
            raise ValueError(f"{who}: idx must be int32 or int64 (n) on {qweight.device}, got {idx.dtype} {tuple(idx.shape)} on {idx.device}")
        if idx.numel() >= 2**31:
            raise ValueError(f"{who}: {idx.numel()} ids exceed the kernels' limit n < 2^31")
    n = qweight.shape[0] if idx is None else idx.numel()
    if out is None:
        # the kernel wants every row 16-byte aligned: rows that are no 16-byte multiple come back as the leading columns of
        # a padded buffer (on the GPU; the CPU path has no such need)
        per16 = 16 // torch.empty((), dtype=out_dtype).element_size()
        padded = -(-dim // per16) * per16 if qweight.is_cuda else dim
        out = torch.empty((n, padded), dtype=out_dtype, device=qweight.device)[:, :dim]
    elif (out.shape != (n, dim) or out.dtype != out_dtype or out.device != qweight.device or (dim > 1 and out.stride(1) != 1)
          or out.data_ptr() % 16 or (n > 1 and out.stride(0) * out.element_size() % 16)):
        raise ValueError(f"{who}: out must be ({n}, {dim}) {out_dtype} on {qweight.device} with unit column stride and 16-byte aligned "
                         f"rows, got {tuple(out.shape)} {out.dtype} on {out.device}, strides {out.stride()}")
    if n == 0:
        return out
    if qweight.shape[0] == 0:
        raise ValueError(f"{who}: {n} rows asked of an empty table")
    if qweight.is_cuda:
        qweight = qweight if qweight.is_contiguous() else qweight.contiguous()
        if idx is not None:
            idx = idx.detach().contiguous()
        out_rs = out.stride(0) if n > 1 else -(-dim // 16) * 16       # (a single row's stride is never used: any aligned one)
        with torch.cuda.device(qweight.device):
            L.check(L.lib().hstu_gather_rows_int8(qweight.data_ptr(), qweight.stride(0), qweight.shape[0], dim,
                                                  idx.data_ptr() if idx is not None else None,
                                                  L.index_dtype_code(idx) if idx is not None else L.HSTU_INDEX_I32, n, out.data_ptr(),
                                                  out_rs, L.torch_dtype_code(out_dtype), L.current_stream_ptr(qweight.device)))
        return out
    rows = qweight if idx is None else qweight.index_select(0, idx.to(torch.int64))
    scale, bias = _scale_bias(rows, dim)
    out.copy_((rows[:, :dim].to(torch.float32) * scale + bias).to(out_dtype))
    return out


def dequantize_rows_int8(qweight: torch.Tensor, dim: int, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """the whole table back as (rows, dim) in ``out_dtype``: the gather with the identity"""
    return gather_rows_int8(qweight, dim, None, out_dtype)


def from_fbgemm_fused_8bit_rowwise(t: torch.Tensor) -> torch.Tensor:
    """fbgemm's packed layout, uint8 (rows, D + 8) = D codes, fp32 scale, fp32 bias without padding -> the aligned table"""
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] < 9:
        raise ValueError(f"from_fbgemm_fused_8bit_rowwise: uint8 (rows, D + 8) expected, got {t.dtype} {tuple(t.shape)}")
    dim = t.shape[1] - 8
    meta = _meta_offset(dim)
    q = torch.zeros((t.shape[0], int8_row_stride(dim)), dtype=torch.uint8, device=t.device)
    q[:, :dim] = t[:, :dim]
    q[:, meta:meta + 8] = t[:, dim:]
    return q


def to_fbgemm_fused_8bit_rowwise(qweight: torch.Tensor, dim: int) -> torch.Tensor:
    """the aligned table -> fbgemm's packed uint8 (rows, dim + 8)"""
    _check_qweight(qweight, dim, "to_fbgemm_fused_8bit_rowwise")
    meta = _meta_offset(dim)
    return torch.cat([qweight[:, :dim], qweight[:, meta:meta + 8]], dim=1)
