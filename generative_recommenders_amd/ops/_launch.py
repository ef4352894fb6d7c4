"""Tensor -> C-ABI marshalling for libhstu_hip.so.  No math here: every function packs
pointers / strides / sizes, launches on torch's current stream, and returns torch tensors
it allocated for the outputs."""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import torch

from generative_recommenders_amd import _lib as L


# Outputs are torch.empty and the kernels write what the jagged metadata describes -- nothing else.  Rows the metadata
# does NOT describe stay uninitialised (the reference's padded-dense PyTorch path would truncate / zero them): attention
# output rows past seq_offsets[-1], delta-attention rows of a user shorter than delta_q, concat / split rows of a user
# whose left + right length exceeds max_seq_len.  All three are caller errors; HSTU_DEBUG_CHECKS=1 turns them into
# exceptions (one host sync per call, debugging only).
DEBUG_CHECKS = os.environ.get("HSTU_DEBUG_CHECKS", "0") not in ("", "0")


def _check_attention_metadata(q, seq_offsets, max_seq_len, delta_q) -> None:
    lengths = (seq_offsets[1:] - seq_offsets[:-1])
    if bool((lengths < 0).any()):
        raise RuntimeError("seq_offsets must be non-decreasing")
    if delta_q > 0:
        if bool((lengths < delta_q).any()):
            raise RuntimeError(f"delta attention: a user has fewer than delta_q = {delta_q} rows (its output rows would stay uninitialised)")
    elif int(seq_offsets[-1]) != q.shape[0]:
        raise RuntimeError(f"seq_offsets[-1] = {int(seq_offsets[-1])} but q has {q.shape[0]} rows (the rows beyond would stay uninitialised)")
    if bool((lengths > max_seq_len).any()):
        raise RuntimeError(f"a user is longer than max_seq_len = {max_seq_len}")


def _check_pair_lengths(ol, orr, max_len_left, max_len_right, max_seq_len, batch) -> None:
    def lens(o, m):
        return (o[1:] - o[:-1]) if o is not None else torch.full((batch,), int(m), dtype=torch.int64, device=(ol if ol is not None else orr).device)
    tot = lens(ol, max_len_left).to(torch.int64) + lens(orr, max_len_right).to(torch.int64)
    if bool((tot > max_seq_len).any()):
        raise RuntimeError(f"concat / split: a user's left + right length exceeds max_seq_len = {max_seq_len} (rows beyond it are not written)")


def _vp(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _aligned_rows(t: torch.Tensor) -> torch.Tensor:
    """(rows, H, d) tensor whose last dim is contiguous and whose (row, head) vectors start
    16-byte aligned; copies only when the layout forces it (flash_common.cpp:360-365)."""
    es = t.element_size()
    ok = (
        t.stride(-1) == 1
        and (t.stride(0) * es) % 16 == 0
        and (t.stride(1) * es) % 16 == 0
        and t.data_ptr() % 16 == 0
    )
    return t if ok else t.contiguous()


def _idx(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype not in (torch.int32, torch.int64):
        t = t.to(torch.int64)
    return t.contiguous()


_ORDER_CACHE = {}


def length_order(seq_offsets: torch.Tensor) -> torch.Tensor:
    """users by descending length (int32 permutation) -- the launch order of the reference's ``sort_by_length``
    (ops/triton/triton_hstu_attention.py:1968-1973) -- at the granularity the kernels' work has: the number of 32-row
    tiles, ties in batch order.  (Sorted by the exact length, a batch of near-equal lengths -- 180..199 rows: 6 or 7 tiles
    -- is walked in a random order for no gain in balance: measured +5 % forward / +3 % backward at 1024 users against
    batch order; by tiles it is two runs in batch order.)  One argsort per batch: the layers of a stack call with the same
    offsets TENSOR OBJECT, so the last result is kept, keyed on that object (a weak reference: alive and the same
    version).  Keying on the storage address would hand the next batch -- whose freshly built offsets the caching
    allocator likes to put at the same address -- the previous batch's order: still a valid permutation, silently the
    wrong one."""
    import weakref

    hit = _ORDER_CACHE.get("last")
    if hit is not None and hit[0]() is seq_offsets and hit[1] == seq_offsets._version:
        return hit[2]
    tiles = (seq_offsets[1:] - seq_offsets[:-1] + 31) >> 5
    order = torch.argsort(tiles, descending=True, stable=True).to(torch.int32)
    _ORDER_CACHE["last"] = (weakref.ref(seq_offsets), seq_offsets._version, order)
    return order


def _fill_attn_params(p: L.HstuAttnParams, q, k, v, out, seq_offsets, num_targets, max_seq_len, alpha, scale,
                      max_attn_len, contextual_seq_len, min_full_attn_seq_len, delta_q, user_order=None) -> None:
    p.user_order = _vp(user_order)
    p.q, p.k, p.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    p.out = _vp(out)
    p.seq_offsets = seq_offsets.data_ptr()
    p.num_targets = _vp(num_targets)
    p.q_row_stride, p.q_head_stride = q.stride(0), q.stride(1)
    p.k_row_stride, p.k_head_stride = k.stride(0), k.stride(1)
    p.v_row_stride, p.v_head_stride = v.stride(0), v.stride(1)
    if out is not None:
        p.o_row_stride, p.o_head_stride = out.stride(0), out.stride(1)
    p.batch = seq_offsets.numel() - 1
    p.heads = q.shape[1]
    p.dqk, p.dv = q.shape[2], v.shape[2]
    p.max_seq_len = int(max_seq_len)
    p.delta_q = int(delta_q)
    p.alpha = float(alpha)
    p.scale = float(scale)
    p.max_attn_len = int(max_attn_len)
    p.contextual_seq_len = int(contextual_seq_len)
    p.min_full_attn_seq_len = int(min_full_attn_seq_len)
    p.dtype = L.torch_dtype_code(q.dtype)
    p.offsets_dtype = L.index_dtype_code(seq_offsets)
    p.targets_dtype = L.index_dtype_code(num_targets) if num_targets is not None else 0


def attn_fwd(q, k, v, seq_offsets, num_targets, max_seq_len, alpha, scale, max_attn_len=0,
             contextual_seq_len=0, min_full_attn_seq_len=0, delta_q=0, user_order=None, descales=None) -> torch.Tensor:
    """``descales``: fp8 (e4m3) q / k / v only -- (q_descale, k_descale, v_descale), each None (= 1) or an fp32 (B, H) GPU
    tensor with any strides (hstu_attn_fwd_fp8)."""
    for name, t in (("q", q), ("k", k), ("v", v), ("seq_offsets", seq_offsets)):
        L.require_gpu_tensor(t, name)
    if not (q.dtype == k.dtype == v.dtype):
        raise RuntimeError("q, k, v must have the same dtype")
    q, k, v = _aligned_rows(q), _aligned_rows(k), _aligned_rows(v)
    seq_offsets, num_targets = _idx(seq_offsets), _idx(num_targets)
    # fp8 (e4m3) q / k / v: bf16 output, as the reference's fp8 forward (flash_common.cpp:454)
    out_dtype = torch.bfloat16 if q.dtype == torch.float8_e4m3fn else q.dtype
    out = torch.empty((q.shape[0], q.shape[1], v.shape[2]), dtype=out_dtype, device=q.device)
    if q.shape[0] == 0:
        return out
    if DEBUG_CHECKS:
        _check_attention_metadata(q, seq_offsets, max_seq_len, delta_q)
    p = L.HstuAttnParams()
    _fill_attn_params(p, q, k, v, out, seq_offsets, num_targets, max_seq_len, alpha, scale, max_attn_len,
                      contextual_seq_len, min_full_attn_seq_len, delta_q, user_order)
    with torch.cuda.device(q.device):
        if descales is None:
            L.check(L.lib().hstu_attn_fwd(C.byref(p), L.current_stream_ptr(q.device)))
        else:
            L.check(L.lib().hstu_attn_fwd_fp8(C.byref(p), C.byref(_fp8_descale(descales, p.batch, p.heads, q.device)),
                                              L.current_stream_ptr(q.device)))
    return out


def _fp8_descale(descales, batch: int, heads: int, device) -> "L.HstuFp8Descale":
    """(q, k, v) descale tensors, each None or fp32 (batch, heads) on q's GPU with any strides -> HstuFp8Descale"""
    d = L.HstuFp8Descale()
    for name, t in zip("qkv", descales):
        if t is None:
            continue
        L.require_gpu_tensor(t, f"{name}_descale")
        if t.dtype != torch.float32 or tuple(t.shape) != (batch, heads):
            raise RuntimeError(f"fp8 attention: {name}_descale must be an fp32 ({batch}, {heads}) tensor, got {t.dtype} {tuple(t.shape)}")
        if t.device != device:
            raise RuntimeError(f"fp8 attention: {name}_descale is on {t.device}, q on {device}")
        setattr(d, name, t.data_ptr())
        setattr(d, f"{name}_batch_stride", t.stride(0))
        setattr(d, f"{name}_head_stride", t.stride(1))
    return d


def jagged_quantize_fp8(x: torch.Tensor, seq_offsets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x8, descale) of a jagged (rows, H, d) bf16 / fp16 / fp32 tensor (hstu_jagged_quantize_fp8): x8 contiguous e4m3, descale
    fp32 (B, H)"""
    L.require_gpu_tensor(x, "x")
    L.require_gpu_tensor(seq_offsets, "seq_offsets")
    if x.dim() != 3 or x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise RuntimeError(f"quantize_jagged_fp8: x must be a (rows, heads, dim) bf16 / fp16 / fp32 tensor, got {x.dtype} {tuple(x.shape)}")
    if x.stride(2) != 1:
        x = x.contiguous()
    seq_offsets = _idx(seq_offsets)
    if seq_offsets.device != x.device:
        raise RuntimeError(f"quantize_jagged_fp8: seq_offsets is on {seq_offsets.device}, x on {x.device}")
    B, H, d = seq_offsets.numel() - 1, x.shape[1], x.shape[2]
    if DEBUG_CHECKS and B > 0:   # (the kernel reads and writes the rows the offsets name: one host sync, debugging only)
        if bool((seq_offsets[1:] < seq_offsets[:-1]).any()) or int(seq_offsets[0]) < 0 or int(seq_offsets[-1]) > x.shape[0]:
            raise RuntimeError(f"quantize_jagged_fp8: seq_offsets must be non-decreasing within [0, {x.shape[0]}] (the rows of x)")
    x8 = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    descale = torch.empty((B, H), dtype=torch.float32, device=x.device)
    if B == 0 or x8.numel() == 0:
        return x8, descale.fill_(1.0)
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_jagged_quantize_fp8(x.data_ptr(), x.stride(0), x.stride(1), x8.data_ptr(), descale.data_ptr(),
                                                 seq_offsets.data_ptr(), B, H, d, L.torch_dtype_code(x.dtype),
                                                 L.index_dtype_code(seq_offsets), L.current_stream_ptr(x.device)))
    return x8, descale


def attn_bwd(dout, q, k, v, seq_offsets, num_targets, max_seq_len, alpha, scale, max_attn_len=0,
             contextual_seq_len=0, min_full_attn_seq_len=0,
             dq: Optional[torch.Tensor] = None, dk: Optional[torch.Tensor] = None,
             dv: Optional[torch.Tensor] = None, user_order=None,
             deterministic: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """dq/dk/dv may be pre-allocated (possibly strided views of one fused buffer), as in
    hstu::hstu_mha_bwd (flash_api.cpp:111-141).  ``deterministic`` (default: torch's own switch,
    ``torch.are_deterministic_algorithms_enabled()``): sequences that need several key blocks add their dq partials in block
    order instead of with atomics (HstuAttnBwdParams::deterministic)."""
    for name, t in (("dout", dout), ("q", q), ("k", k), ("v", v)):
        L.require_gpu_tensor(t, name)
    q, k, v, dout = _aligned_rows(q), _aligned_rows(k), _aligned_rows(v), _aligned_rows(dout)
    seq_offsets, num_targets = _idx(seq_offsets), _idx(num_targets)
    dq = torch.empty_like(q, memory_format=torch.contiguous_format) if dq is None else dq
    dk = torch.empty_like(k, memory_format=torch.contiguous_format) if dk is None else dk
    dv = torch.empty_like(v, memory_format=torch.contiguous_format) if dv is None else dv
    if q.shape[0] == 0:
        return dq, dk, dv
    bp = L.HstuAttnBwdParams()
    _fill_attn_params(bp.fwd, q, k, v, None, seq_offsets, num_targets, max_seq_len, alpha, scale, max_attn_len,
                      contextual_seq_len, min_full_attn_seq_len, 0, user_order)
    bp.dout, bp.dq, bp.dk, bp.dv = dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    bp.do_row_stride, bp.do_head_stride = dout.stride(0), dout.stride(1)
    bp.dq_row_stride, bp.dq_head_stride = dq.stride(0), dq.stride(1)
    bp.dk_row_stride, bp.dk_head_stride = dk.stride(0), dk.stride(1)
    bp.dv_row_stride, bp.dv_head_stride = dv.stride(0), dv.stride(1)
    bp.total_rows = q.shape[0]
    bp.deterministic = int(torch.are_deterministic_algorithms_enabled() if deterministic is None else deterministic)
    ws_bytes = L.lib().hstu_attn_bwd_workspace_bytes(C.byref(bp))
    ws = None
    if ws_bytes:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
        bp.workspace = ws.data_ptr()
    with torch.cuda.device(q.device):
        L.check(L.lib().hstu_attn_bwd(C.byref(bp), L.current_stream_ptr(q.device)))
    return dq, dk, dv


def _shape_params(p: L.HstuAttnParams, dtype, heads, dqk, dv, max_seq_len, alpha, max_attn_len, contextual_seq_len,
                  min_full_attn_seq_len, with_bias) -> None:
    p.batch, p.heads, p.dqk, p.dv, p.max_seq_len = 1, int(heads), int(dqk), int(dv), int(max_seq_len)
    p.alpha, p.scale = float(alpha), 1.0 / max_seq_len
    p.max_attn_len, p.contextual_seq_len, p.min_full_attn_seq_len = int(max_attn_len), int(contextual_seq_len), int(min_full_attn_seq_len)
    p.dtype = L.torch_dtype_code(dtype)
    p.pos_w = 1 if with_bias else None          # only NULL / non-NULL is looked at
    if with_bias and with_bias != "position":   # True: position AND time tables (128 buckets unless with_bias is a number)
        p.ts_w, p.timestamps = 1, 1
        p.num_buckets = 128 if with_bias is True else int(with_bias)


def attn_fwd_kernel_name(dtype, dqk, dv, max_seq_len, heads=1, alpha=1.0, max_attn_len=0, contextual_seq_len=0,
                         min_full_attn_seq_len=0, with_bias=False) -> str:
    """the forward instantiation the library dispatches for this shape (hstu_attn_fwd_kernel_name)"""
    p = L.HstuAttnParams()
    _shape_params(p, dtype, heads, dqk, dv, max_seq_len, alpha, max_attn_len, contextual_seq_len, min_full_attn_seq_len, with_bias)
    buf = C.create_string_buffer(128)
    L.check(L.lib().hstu_attn_fwd_kernel_name(C.byref(p), buf, 128))
    return buf.value.decode()


def attn_bwd_kernel_name(dtype, dqk, dv, max_seq_len, heads=1, alpha=1.0, max_attn_len=0, contextual_seq_len=0,
                         min_full_attn_seq_len=0, with_bias=False) -> str:
    """the backward instantiation the library dispatches for this shape (hstu_attn_bwd_kernel_name)"""
    bp = L.HstuAttnBwdParams()
    _shape_params(bp.fwd, dtype, heads, dqk, dv, max_seq_len, alpha, max_attn_len, contextual_seq_len, min_full_attn_seq_len,
                  with_bias)
    buf = C.create_string_buffer(128)
    L.check(L.lib().hstu_attn_bwd_kernel_name(C.byref(bp), buf, 128))
    return buf.value.decode()


# ----------------------------------------------------------------------------- jagged
def complete_cumsum(lengths: torch.Tensor) -> torch.Tensor:
    L.require_gpu_tensor(lengths, "lengths")
    lengths = _idx(lengths)
    out = torch.empty(lengths.numel() + 1, dtype=lengths.dtype, device=lengths.device)
    with torch.cuda.device(lengths.device):
        L.check(L.lib().hstu_complete_cumsum(lengths.data_ptr(), out.data_ptr(), lengths.numel(),
                                             L.index_dtype_code(lengths), L.current_stream_ptr(lengths.device)))
    return out


def _pair_offsets(offsets_left, offsets_right):
    ol, orr = _idx(offsets_left), _idx(offsets_right)
    if ol is not None and orr is not None and ol.dtype != orr.dtype:
        ol, orr = ol.to(torch.int64), orr.to(torch.int64)
    ref = ol if ol is not None else orr
    return ol, orr, L.index_dtype_code(ref), ref.numel() - 1


def concat_2d_jagged(values_left, values_right, offsets_left, offsets_right, max_len_left, max_len_right,
                     max_seq_len, n_prefix=0) -> torch.Tensor:
    L.require_gpu_tensor(values_left, "values_left")
    L.require_gpu_tensor(values_right, "values_right")
    vl, vr = values_left.contiguous(), values_right.contiguous()
    dim = vl.shape[1]
    out = torch.empty((vl.shape[0] + vr.shape[0], dim), dtype=vl.dtype, device=vl.device)
    if out.shape[0] == 0:
        return out
    if offsets_left is None and offsets_right is None:
        batch, idt, ol, orr = vl.shape[0] // max_len_left, 0, None, None
    else:
        ol, orr, idt, batch = _pair_offsets(offsets_left, offsets_right)
        if DEBUG_CHECKS:
            _check_pair_lengths(ol, orr, max_len_left, max_len_right, max_seq_len, batch)
    with torch.cuda.device(vl.device):
        L.check(L.lib().hstu_concat_2d_jagged(vl.data_ptr(), vr.data_ptr(), out.data_ptr(), _vp(ol), _vp(orr),
                                              int(max_len_left or 0), int(max_len_right or 0), int(max_seq_len),
                                              batch, dim, vl.element_size(), int(n_prefix), idt,
                                              L.current_stream_ptr(vl.device)))
    return out


def split_2d_jagged(values, total_left, total_right, offsets_left, offsets_right, max_len_left, max_len_right,
                    max_seq_len, n_prefix=0) -> Tuple[torch.Tensor, torch.Tensor]:
    L.require_gpu_tensor(values, "values")
    vals = values.contiguous()
    dim = vals.shape[1]
    left = torch.empty((total_left, dim), dtype=vals.dtype, device=vals.device)
    right = torch.empty((total_right, dim), dtype=vals.dtype, device=vals.device)
    if vals.shape[0] == 0:
        return left, right
    ol, orr, idt, batch = _pair_offsets(offsets_left, offsets_right)
    if DEBUG_CHECKS:
        _check_pair_lengths(ol, orr, max_len_left, max_len_right, max_seq_len, batch)
    with torch.cuda.device(vals.device):
        L.check(L.lib().hstu_split_2d_jagged(vals.data_ptr(), left.data_ptr(), right.data_ptr(), _vp(ol), _vp(orr),
                                             int(max_len_left or 0), int(max_len_right or 0), int(max_seq_len),
                                             batch, dim, vals.element_size(), int(n_prefix), idt,
                                             L.current_stream_ptr(vals.device)))
    return left, right


def jagged_to_padded_dense(values, offsets, max_len) -> torch.Tensor:
    L.require_gpu_tensor(values, "values")
    vals = values.contiguous()
    offsets = _idx(offsets)
    B = offsets.numel() - 1
    dim = 1
    for s_ in vals.shape[1:]:
        dim *= s_
    dense = torch.empty((B, max_len) + tuple(vals.shape[1:]), dtype=vals.dtype, device=vals.device)
    if dense.numel() == 0:
        return dense
    with torch.cuda.device(vals.device):
        L.check(L.lib().hstu_jagged_to_padded_dense(vals.data_ptr(), dense.data_ptr(), offsets.data_ptr(), B,
                                                    int(max_len), dim, vals.element_size(),
                                                    L.index_dtype_code(offsets), L.current_stream_ptr(vals.device)))
    return dense


def jagged_write_tail_(values: torch.Tensor, dense: torch.Tensor, offsets: torch.Tensor, tail: int) -> torch.Tensor:
    """IN PLACE: the last ``tail`` rows of every user's region of ``values`` (sum L, ...) <- dense (B * tail, ...)."""
    L.require_gpu_tensor(values, "values")
    L.require_gpu_tensor(dense, "dense")
    if not values.is_contiguous():
        raise RuntimeError("jagged_write_tail_: the destination must be contiguous (it is written in place)")
    dense = dense.contiguous()
    offsets = _idx(offsets)
    B = offsets.shape[0] - 1
    dim = values[0].numel() if values.shape[0] else 0
    if dense.dtype != values.dtype or dense.shape[0] != B * tail or (dense.shape[0] and dense[0].numel() != dim):
        raise RuntimeError(f"jagged_write_tail_: dense {tuple(dense.shape)} {dense.dtype} does not hold {B} x {tail} rows of values {tuple(values.shape)} {values.dtype}")
    if B == 0 or tail == 0 or dim == 0:
        return values
    with torch.cuda.device(values.device):
        L.check(L.lib().hstu_jagged_write_tail(dense.data_ptr(), values.data_ptr(), offsets.data_ptr(), B, int(tail), dim,
                                               values.element_size(), L.index_dtype_code(offsets),
                                               L.current_stream_ptr(values.device)))
    return values


def dense_to_jagged(dense, offsets, total_rows) -> torch.Tensor:
    L.require_gpu_tensor(dense, "dense")
    d = dense.contiguous()
    offsets = _idx(offsets)
    B, max_len = d.shape[0], d.shape[1]
    dim = 1
    for s in d.shape[2:]:
        dim *= s
    out = torch.zeros((total_rows,) + tuple(d.shape[2:]), dtype=d.dtype, device=d.device)
    if out.numel() == 0 or d.numel() == 0:
        return out
    with torch.cuda.device(d.device):
        L.check(L.lib().hstu_dense_to_jagged(d.data_ptr(), out.data_ptr(), offsets.data_ptr(), B, max_len, dim,
                                             d.element_size(), L.index_dtype_code(offsets),
                                             L.current_stream_ptr(d.device)))
    return out


def expand_1d_jagged_to_dense(values, offsets, max_len) -> torch.Tensor:
    L.require_gpu_tensor(values, "values")
    vals, offsets = values.contiguous(), _idx(offsets)
    B = offsets.numel() - 1
    out = torch.empty((B, max_len), dtype=vals.dtype, device=vals.device)
    with torch.cuda.device(vals.device):
        L.check(L.lib().hstu_expand_1d_jagged_to_dense(vals.data_ptr(), offsets.data_ptr(), out.data_ptr(), B,
                                                       int(max_len), vals.element_size(),
                                                       L.index_dtype_code(offsets), L.current_stream_ptr(vals.device)))
    return out


def concat_1d_jagged_jagged(lengths_left, values_left, lengths_right, values_right) -> torch.Tensor:
    L.require_gpu_tensor(values_left, "values_left")
    ol = complete_cumsum(lengths_left.to(torch.int64))
    orr = complete_cumsum(lengths_right.to(torch.int64))
    vl, vr = values_left.contiguous(), values_right.contiguous()
    out = torch.empty(vl.numel() + vr.numel(), dtype=vl.dtype, device=vl.device)
    with torch.cuda.device(vl.device):
        L.check(L.lib().hstu_concat_1d_jagged_jagged(vl.data_ptr(), ol.data_ptr(), vr.data_ptr(), orr.data_ptr(),
                                                     out.data_ptr(), lengths_left.numel(), vl.element_size(),
                                                     L.HSTU_INDEX_I64, L.current_stream_ptr(vl.device)))
    return out


# ----------------------------------------------------------------------------- jagged x dense bmm
def _bmm_unit(dtype: torch.dtype) -> int:
    return 4 if dtype == torch.float32 else 8      # elements per 16 bytes


def _bmm_rows(t: torch.Tensor, cols: int) -> torch.Tensor:
    """(rows, c) -> (rows, cols >= c) with unit column stride and 16-byte aligned rows; zero-padded copy only when needed"""
    es = t.element_size()
    if t.shape[1] == cols and t.stride(1) == 1 and (t.stride(0) * es) % 16 == 0 and t.stride(0) >= cols and t.data_ptr() % 16 == 0:
        return t
    if t.shape[1] == cols:
        return t.contiguous()
    return torch.nn.functional.pad(t, (0, cols - t.shape[1]))


def _bmm_dense(d: torch.Tensor, kp: int, np_: int) -> torch.Tensor:
    """(B, K, N) -> (B, kp, np_) the kernel can read: a unit stride along K or N, the other strides multiples of 16 bytes"""
    es = d.element_size()
    ok = d.shape[1] == kp and d.shape[2] == np_ and d.data_ptr() % 16 == 0 and (d.stride(0) * es) % 16 == 0
    if ok and d.stride(2) == 1 and (d.stride(1) * es) % 16 == 0:
        return d
    if ok and d.stride(1) == 1 and (d.stride(2) * es) % 16 == 0:
        return d
    if d.shape[1] == kp and d.shape[2] == np_:
        return d.contiguous()
    return torch.nn.functional.pad(d, (0, np_ - d.shape[2], 0, kp - d.shape[1]))


def _bmm_check(jagged, dense, seq_offsets, what):
    L.require_gpu_tensor(jagged, what)
    L.require_gpu_tensor(dense, "dense")
    L.require_gpu_tensor(seq_offsets, "seq_offsets")
    if jagged.dtype not in (torch.bfloat16, torch.float16, torch.float32) or dense.dtype != jagged.dtype:
        raise RuntimeError(f"jagged_dense_bmm: {what} and dense must share a bf16 / fp16 / fp32 dtype, got {jagged.dtype} and {dense.dtype}")
    if dense.device != jagged.device or seq_offsets.device != jagged.device:
        raise RuntimeError(f"jagged_dense_bmm: {what} is on {jagged.device}, dense on {dense.device}, seq_offsets on {seq_offsets.device}")


def jagged_dense_bmm_fwd(jagged: torch.Tensor, dense: torch.Tensor, bias: Optional[torch.Tensor],
                         seq_offsets: torch.Tensor) -> torch.Tensor:
    """out[s:e] = jagged[s:e] @ dense[b] (+ bias[b]) per user (hstu_jagged_dense_bmm_fwd).  jagged (rows, K), dense (B, K, N) with
    any strides, bias (B, N) of any float dtype or None -> (rows, N).  The data gradient is this with d_out as ``jagged``,
    ``dense.transpose(1, 2)`` and no bias.  K / N that are not multiples of 16 bytes are zero-padded here (exact)."""
    _bmm_check(jagged, dense, seq_offsets, "jagged")
    seq_offsets = _idx(seq_offsets)
    rows, K = jagged.shape
    B, _, N = dense.shape
    unit = _bmm_unit(jagged.dtype)
    kp, np_ = -(-K // unit) * unit, -(-N // unit) * unit
    out = torch.empty((rows, np_), dtype=jagged.dtype, device=jagged.device)
    if B > 0 and rows > 0:
        a = _bmm_rows(jagged, kp)
        d = _bmm_dense(dense, kp, np_)
        bf = None
        if bias is not None:
            bf = _bmm_rows(bias.to(device=jagged.device, dtype=torch.float32), np_).contiguous()
        lib = L.lib()
        ws = torch.empty(lib.hstu_jagged_dense_bmm_workspace_bytes(B), dtype=torch.uint8, device=jagged.device)
        with torch.cuda.device(jagged.device):
            L.check(lib.hstu_jagged_dense_bmm_fwd(a.data_ptr(), a.stride(0), d.data_ptr(), d.stride(0), d.stride(1), d.stride(2),
                                                  _vp(bf), np_, out.data_ptr(), out.stride(0), seq_offsets.data_ptr(), rows, B,
                                                  kp, np_, ws.data_ptr(), L.torch_dtype_code(jagged.dtype),
                                                  L.index_dtype_code(seq_offsets), L.current_stream_ptr(jagged.device)))
    return out if np_ == N else out[:, :N].contiguous()


def jagged_dense_bmm_wgrad(jagged: torch.Tensor, d_out: torch.Tensor, seq_offsets: torch.Tensor,
                           want_bias: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(d_dense (B, K, N) in jagged's dtype, d_bias (B, N) fp32 or None) of jagged_dense_bmm_fwd (hstu_jagged_dense_bmm_wgrad):
    fixed summation order, every slab written (zeros for an empty user)."""
    _bmm_check(jagged, d_out, seq_offsets, "jagged")
    seq_offsets = _idx(seq_offsets)
    rows, K = jagged.shape
    N = d_out.shape[1]
    B = seq_offsets.numel() - 1
    unit = _bmm_unit(jagged.dtype)
    kp, np_ = -(-K // unit) * unit, -(-N // unit) * unit
    dd = torch.empty((B, kp, np_), dtype=jagged.dtype, device=jagged.device)
    db = torch.empty((B, np_), dtype=torch.float32, device=jagged.device) if want_bias else None
    if B > 0:
        a = _bmm_rows(jagged, kp)
        g = _bmm_rows(d_out, np_)
        with torch.cuda.device(jagged.device):
            L.check(L.lib().hstu_jagged_dense_bmm_wgrad(a.data_ptr(), a.stride(0), g.data_ptr(), g.stride(0), dd.data_ptr(),
                                                        dd.stride(0), dd.stride(1), _vp(db), np_, seq_offsets.data_ptr(), rows, B,
                                                        kp, np_, L.torch_dtype_code(jagged.dtype),
                                                        L.index_dtype_code(seq_offsets), L.current_stream_ptr(jagged.device)))
    if kp != K or np_ != N:
        dd = dd[:, :K, :N].contiguous()
        db = db[:, :N].contiguous() if db is not None else None
    return dd, db


# ----------------------------------------------------------------------------- MIPS top-k
def mips_topk_dim(dim: int, dtype: torch.dtype) -> int:
    """dim rounded up to the kernel's K unit (16 bytes)"""
    unit = _bmm_unit(dtype)
    return -(-dim // unit) * unit


def mips_topk(queries: torch.Tensor, items: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k items with the largest <query, item> for every query row (hstu_mips_topk): queries (B, D), items (X, D') with
    D' >= D (columns past D are zero padding) -> (scores (B, k) in the inputs' dtype, indices (B, k) int32 into ``items``), sorted
    by score descending, then index ascending.  No (B, X) tensor exists at any point; stream-ordered, no host sync.  Rows that
    are not 16-byte aligned are zero-padded here (exact); a table padded once by the caller (``mips_topk_dim``) is used as is."""
    L.require_gpu_tensor(queries, "queries")
    L.require_gpu_tensor(items, "items")
    if queries.dim() != 2 or items.dim() != 2 or queries.shape[1] > items.shape[1]:
        raise RuntimeError(f"mips_topk: queries (B, D) and items (X, D) expected, got {tuple(queries.shape)} and {tuple(items.shape)}")
    if queries.dtype not in (torch.bfloat16, torch.float16, torch.float32) or items.dtype != queries.dtype:
        raise RuntimeError(f"mips_topk: queries and items must share a bf16 / fp16 / fp32 dtype, got {queries.dtype} and {items.dtype}")
    if items.device != queries.device:
        raise RuntimeError(f"mips_topk: queries are on {queries.device}, items on {items.device}")
    B, X = queries.shape[0], items.shape[0]
    k = int(k)
    dp = mips_topk_dim(items.shape[1], items.dtype)
    scores = torch.empty((B, k if k > 0 else 0), dtype=queries.dtype, device=queries.device)
    indices = torch.empty((B, k if k > 0 else 0), dtype=torch.int32, device=queries.device)
    lib = L.lib()
    if B > 0 and X > 0:
        q, t = _bmm_rows(queries, dp), _bmm_rows(items, dp)
        ws = torch.empty(lib.hstu_mips_topk_workspace_bytes(B, max(k, 0)), dtype=torch.uint8, device=queries.device)
        args = (q.data_ptr(), q.stride(0), t.data_ptr(), t.stride(0), scores.data_ptr(), indices.data_ptr(), ws.data_ptr())
    else:       # nothing to launch; the library still judges the shape
        args = (None, dp, None, dp, None, None, None)
    with torch.cuda.device(queries.device):
        L.check(lib.hstu_mips_topk(*args, B, X, dp, k, L.torch_dtype_code(queries.dtype), L.current_stream_ptr(queries.device)))
    return scores, indices


# ----------------------------------------------------------------------------- Mixture-of-Logits
MOL_MAX_LOGITS, MOL_MAX_DIM, MOL_MAX_HIDDEN = 64, 128, 256       # HSTU_MOL_MAX_* of include/hstu_hip.h
MOL_COMBINATIONS = {"glu_silu": 0, "glu_silu_ln": 1}


def mol_scores(qc: torch.Tensor, xc: torch.Tensor, gq: torch.Tensor, gi: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor],
               w2: Optional[torch.Tensor], b2: torch.Tensor, inv_temperature: float, combination: str) -> torch.Tensor:
    """Mixture-of-Logits scores of every (query, item) pair (hstu_mol_scores): qc (B, P_Q, D), xc (X, P_X, D), gq (B, L),
    gi (X, L), the gating MLP w1 (H, L), b1 (H), w2 (L, H), b2 (L) -- or one layer w1 (L, L), b2 (L) with b1 = w2 = None -- all
    of one bf16 / fp16 / fp32 dtype -> (B, X) fp32.  Contiguous operands are used as they are; the library judges the shape."""
    names = ("qc", "xc", "gq", "gi", "w1", "b1", "w2", "b2")
    tensors = (qc, xc, gq, gi, w1, b1, w2, b2)
    for name, t in zip(names, tensors):
        if t is None:
            continue
        L.require_gpu_tensor(t, name)
        if t.dtype != qc.dtype or t.device != qc.device:
            raise RuntimeError(f"mol_scores: {name} is {t.dtype} on {t.device}, qc is {qc.dtype} on {qc.device}")
    if combination not in MOL_COMBINATIONS:
        raise RuntimeError(f"mol_scores: combination {combination!r} has no kernel (built: {sorted(MOL_COMBINATIONS)})")
    if qc.dim() != 3 or xc.dim() != 3 or qc.shape[2] != xc.shape[2]:
        raise RuntimeError(f"mol_scores: qc (B, P_Q, D) and xc (X, P_X, D) expected, got {tuple(qc.shape)} and {tuple(xc.shape)}")
    B, PQ, D = qc.shape
    X, PX, _ = xc.shape
    nl = PQ * PX
    H = w1.shape[0] if w2 is not None else 0
    if ((b1 is None) != (w2 is None) or gq.shape != (B, nl) or gi.shape != (X, nl) or b2.shape != (nl,)
            or w1.shape != ((H, nl) if H else (nl, nl)) or (H and (w2.shape != (nl, H) or b1.shape != (H,)))):
        raise RuntimeError(f"mol_scores: operand shapes do not fit P_Q = {PQ}, P_X = {PX}, H = {H}")
    out = torch.empty((B, X), dtype=torch.float32, device=qc.device)
    ptr = [t.contiguous() if t is not None else None for t in tensors]
    args = [t.data_ptr() if t is not None else None for t in ptr]
    with torch.cuda.device(qc.device):
        L.check(L.lib().hstu_mol_scores(*args, out.data_ptr(), B, X, PQ, PX, D, H, float(inv_temperature), MOL_COMBINATIONS[combination],
                                        L.torch_dtype_code(qc.dtype), L.current_stream_ptr(qc.device)))
    return out


# ----------------------------------------------------------------------------- norms
def _f32(n, device):
    return torch.empty(n, dtype=torch.float32, device=device)


def layer_norm_fwd(x, weight, bias, eps):
    L.require_gpu_tensor(x, "x")
    x = x.contiguous()
    rows, dim = x.shape
    y = torch.empty_like(x)
    mean, rstd = _f32(rows, x.device), _f32(rows, x.device)
    w, b = weight.to(x.dtype).contiguous(), bias.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_layer_norm_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                            rstd.data_ptr(), rows, dim, float(eps), L.torch_dtype_code(x.dtype),
                                            L.current_stream_ptr(x.device)))
    return y, mean, rstd


def swish_layer_norm_fwd(x, weight, bias, eps):
    """y = x * sigmoid(LayerNorm(x)) (hstu_swish_layer_norm_fwd): returns (y, mean, rstd)"""
    L.require_gpu_tensor(x, "x")
    x = x.contiguous()
    rows, dim = x.shape
    y = torch.empty_like(x)
    mean, rstd = _f32(rows, x.device), _f32(rows, x.device)
    w, b = weight.to(x.dtype).contiguous(), bias.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_swish_layer_norm_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                                  rstd.data_ptr(), rows, dim, float(eps), L.torch_dtype_code(x.dtype),
                                                  L.current_stream_ptr(x.device)))
    return y, mean, rstd


def swish_layer_norm_bwd(dy, x, weight, bias, mean, rstd):
    """dx, dweight (fp32), dbias (fp32) of swish_layer_norm_fwd"""
    dy, x = dy.contiguous(), x.contiguous()
    rows, dim = x.shape
    dx = torch.empty_like(x)
    dw, db = _f32(dim, x.device), _f32(dim, x.device)
    ws = torch.empty(L.lib().hstu_norm_bwd_workspace_bytes(rows, dim), dtype=torch.uint8, device=x.device)
    w, b = weight.to(x.dtype).contiguous(), bias.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_swish_layer_norm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                                  rstd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                                  rows, dim, L.torch_dtype_code(x.dtype), L.current_stream_ptr(x.device)))
    return dx, dw, db


def rms_norm_fwd(x, weight, eps):
    """y = x * rstd * weight (hstu_rms_norm_fwd): returns (y, rstd)"""
    L.require_gpu_tensor(x, "x")
    x = x.contiguous()
    rows, dim = x.shape
    y = torch.empty_like(x)
    rstd = _f32(rows, x.device)
    w = weight.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_rms_norm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), rows, dim, float(eps),
                                          L.torch_dtype_code(x.dtype), L.current_stream_ptr(x.device)))
    return y, rstd


def rms_norm_bwd(dy, x, weight, rstd):
    """dx, dweight (fp32) of rms_norm_fwd"""
    dy, x = dy.contiguous(), x.contiguous()
    rows, dim = x.shape
    dx = torch.empty_like(x)
    dw = _f32(dim, x.device)
    ws = torch.empty(L.lib().hstu_norm_bwd_workspace_bytes(rows, dim), dtype=torch.uint8, device=x.device)
    w = weight.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_rms_norm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                          ws.data_ptr(), rows, dim, L.torch_dtype_code(x.dtype), L.current_stream_ptr(x.device)))
    return dx, dw


def ln_linear_supported(x, n):
    """whether the fused LayerNorm + projection kernel takes (rows, k) activations and n output columns"""
    return bool(x.is_cuda and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16) and
                L.lib().hstu_ln_linear_fwd_supported(x.shape[0], x.shape[1], n, L.torch_dtype_code(x.dtype)))


def ln_linear_fwd(x, ln_weight, ln_bias, eps, w_nk, bias, want_normed=False):
    """y = LayerNorm(x) @ w_nk.T + bias in one kernel (csrc/hstu_ln_linear.cuh): returns (y, normed_x or None, mean, rstd).
    ``w_nk``: the (n, k) K-contiguous weight in x's dtype."""
    L.require_gpu_tensor(x, "x")
    x = x.contiguous()
    rows, k = x.shape
    n = w_nk.shape[0]
    torch._assert(w_nk.shape[1] == k and w_nk.is_contiguous() and w_nk.dtype == x.dtype, "w_nk must be a contiguous (n, k) tensor of x's dtype")
    y = torch.empty((rows, n), dtype=x.dtype, device=x.device)
    normed = torch.empty_like(x) if want_normed else None
    mean, rstd = _f32(rows, x.device), _f32(rows, x.device)
    w, b = ln_weight.to(x.dtype).contiguous(), ln_bias.to(x.dtype).contiguous()
    pb = None if bias is None else bias.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_ln_linear_fwd(x.data_ptr(), k, w.data_ptr(), b.data_ptr(), float(eps), w_nk.data_ptr(),
                                           None if pb is None else pb.data_ptr(), y.data_ptr(), n,
                                           None if normed is None else normed.data_ptr(), k, mean.data_ptr(), rstd.data_ptr(),
                                           rows, k, n, L.torch_dtype_code(x.dtype), L.current_stream_ptr(x.device)))
    return y, normed, mean, rstd


def linear_k512_supported(x, n):
    """whether hstu_linear_k512 takes (rows, 512) activations (last dimension contiguous, row stride a multiple of 8) and n output columns"""
    return bool(x.is_cuda and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16) and x.stride(1) == 1 and
                x.stride(0) % 8 == 0 and x.stride(0) >= x.shape[1] and x.data_ptr() % 16 == 0 and
                L.lib().hstu_linear_k512_supported(x.shape[0], x.shape[1], n, L.torch_dtype_code(x.dtype)))


def linear_k512(x, w_nk, bias=None):
    """y = x @ w_nk.T (+ bias) with a contraction length of 512 (csrc/hstu_ln_linear.cuh without the LayerNorm): the output
    stage's d y = d out . W_out^T, whose (n, k) operand is the layer's ``_output_weight`` as stored."""
    L.require_gpu_tensor(x, "x")
    rows, k = x.shape
    n = w_nk.shape[0]
    torch._assert(w_nk.shape[1] == k and w_nk.is_contiguous() and w_nk.dtype == x.dtype, "w_nk must be a contiguous (n, k) tensor of x's dtype")
    torch._assert(x.stride(1) == 1, "x must have a contiguous last dimension")
    y = torch.empty((rows, n), dtype=x.dtype, device=x.device)
    pb = None if bias is None else bias.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_linear_k512(x.data_ptr(), x.stride(0), w_nk.data_ptr(), None if pb is None else pb.data_ptr(),
                                         y.data_ptr(), n, rows, k, n, L.torch_dtype_code(x.dtype), L.current_stream_ptr(x.device)))
    return y


def quantize_rows_fp8(src):
    """(codes, scale) of the rows of a 2-D bf16 / fp16 / fp32 tensor (hstu_quantize_rows_fp8): codes e4m3 (rows, k) contiguous,
    scale fp32 per row = amax / 448 (1 for a zero row), codes = e4m3(clamp(src / scale, -448, 448))"""
    L.require_gpu_tensor(src, "src")
    torch._assert(src.dim() == 2 and src.stride(1) == 1, "src must be 2-D with a contiguous last dimension")
    rows, k = src.shape
    q = torch.empty((rows, k), dtype=torch.float8_e4m3fn, device=src.device)
    scale = _f32(rows, src.device)
    with torch.cuda.device(src.device):
        L.check(L.lib().hstu_quantize_rows_fp8(src.data_ptr(), src.stride(0), rows, k, L.torch_dtype_code(src.dtype), q.data_ptr(),
                                               scale.data_ptr(), L.current_stream_ptr(src.device)))
    return q, scale


def ln_linear_fp8_supported(x, n):
    """whether the row-wise e4m3 LayerNorm + projection kernel takes (rows, k) activations and n output columns"""
    return bool(x.is_cuda and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16) and
                L.lib().hstu_ln_linear_fp8_supported(x.shape[0], x.shape[1], n, L.torch_dtype_code(x.dtype)))


def ln_linear_fp8_fwd(x, ln_weight, ln_bias, eps, wq, w_scale, bias, want_q=False):
    """y = (q(LayerNorm(x)) @ wq.T) * x_scale[:, None] * w_scale + bias in one kernel (csrc/hstu_ln_linear_fp8.cuh): returns
    (y, xq or None, x_scale or None, mean, rstd).  ``(wq, w_scale)``: quantize_rows_fp8 of the (n, k) K-contiguous weight."""
    L.require_gpu_tensor(x, "x")
    x = x.contiguous()
    rows, k = x.shape
    n = wq.shape[0]
    torch._assert(wq.shape[1] == k and wq.is_contiguous() and wq.dtype == torch.float8_e4m3fn, "wq must be a contiguous (n, k) e4m3 tensor")
    torch._assert(w_scale.shape == (n,) and w_scale.dtype == torch.float32 and w_scale.is_contiguous(), "w_scale must be n fp32 values")
    y = torch.empty((rows, n), dtype=x.dtype, device=x.device)
    xq = torch.empty((rows, k), dtype=torch.float8_e4m3fn, device=x.device) if want_q else None
    x_scale = _f32(rows, x.device) if want_q else None
    mean, rstd = _f32(rows, x.device), _f32(rows, x.device)
    w, b = ln_weight.to(x.dtype).contiguous(), ln_bias.to(x.dtype).contiguous()
    pb = None if bias is None else bias.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_ln_linear_fp8_fwd(x.data_ptr(), k, w.data_ptr(), b.data_ptr(), float(eps), wq.data_ptr(), w_scale.data_ptr(),
                                               None if pb is None else pb.data_ptr(), y.data_ptr(), n,
                                               None if xq is None else xq.data_ptr(), None if x_scale is None else x_scale.data_ptr(),
                                               mean.data_ptr(), rstd.data_ptr(), rows, k, n, L.torch_dtype_code(x.dtype),
                                               L.current_stream_ptr(x.device)))
    return y, xq, x_scale, mean, rstd


def linear_fp8_rowwise(xq, x_scale, wq, w_scale, bias=None, out_dtype=torch.bfloat16):
    """y = (xq @ wq.T) * x_scale[:, None] * w_scale (+ bias) on e4m3 codes with row-wise scales (the fp8 kernel without its
    LayerNorm): xq (rows, 512), wq (n, 512) contiguous e4m3, scales fp32"""
    L.require_gpu_tensor(xq, "xq")
    rows, k = xq.shape
    n = wq.shape[0]
    torch._assert(xq.is_contiguous() and wq.is_contiguous() and xq.dtype == torch.float8_e4m3fn and wq.dtype == torch.float8_e4m3fn and
                  wq.shape[1] == k, "xq and wq must be contiguous e4m3 tensors with the same k")
    torch._assert(x_scale.shape == (rows,) and w_scale.shape == (n,) and x_scale.dtype == torch.float32 and w_scale.dtype == torch.float32 and
                  x_scale.is_contiguous() and w_scale.is_contiguous(), "x_scale / w_scale must be fp32, one per row")
    y = torch.empty((rows, n), dtype=out_dtype, device=xq.device)
    pb = None if bias is None else bias.to(out_dtype).contiguous()
    with torch.cuda.device(xq.device):
        L.check(L.lib().hstu_linear_fp8_rowwise(xq.data_ptr(), x_scale.data_ptr(), wq.data_ptr(), w_scale.data_ptr(),
                                                None if pb is None else pb.data_ptr(), y.data_ptr(), n, rows, k, n,
                                                L.torch_dtype_code(out_dtype), L.current_stream_ptr(xq.device)))
    return y


_ADDMM_LT = os.environ.get("HSTU_ADDMM_LT", "1") != "0"      # 0: torch.addmm (copy + in-place GEMM), the comparator
_ADDMM_WS: dict = {}          # device -> hipBLASLt workspace (32 MiB, as PyTorch's own), allocated once


def addmm_residual_supported(c, a, b) -> bool:
    """whether ``c + a @ b`` can run as ONE hipBLASLt launch with separate C and D buffers (hstu_addmm_residual): 2-D 16-bit CUDA
    operands of one dtype, c of the result's shape, rows contiguous and 16-byte aligned"""
    if not (_ADDMM_LT and a.is_cuda and a.dim() == 2 and b.dim() == 2 and c.dim() == 2 and a.dtype in (torch.bfloat16, torch.float16)
            and b.dtype == a.dtype and c.dtype == a.dtype and c.shape == (a.shape[0], b.shape[1]) and a.shape[1] == b.shape[0]):
        return False
    for t in (a, b, c):
        if t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.stride(0) % 8 or t.data_ptr() % 16:
            return False
    return a.shape[0] > 0 and bool(L.lib().hstu_addmm_residual_supported())


def addmm_residual(c, a, b):
    """``c + a @ b`` (fp32 accumulation) without the copy of c that torch.addmm makes: hipBLASLt reads c and writes the result"""
    L.require_gpu_tensor(a, "a")
    m, k = a.shape
    n = b.shape[1]
    d = torch.empty((m, n), dtype=a.dtype, device=a.device)
    ws = _ADDMM_WS.get(a.device)
    if ws is None:
        ws = _ADDMM_WS[a.device] = torch.empty(32 << 20, dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        L.check(L.lib().hstu_addmm_residual(c.data_ptr(), c.stride(0), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), d.data_ptr(), n,
                                            m, n, k, L.torch_dtype_code(a.dtype), ws.data_ptr(), ws.numel(), L.current_stream_ptr(a.device)))
    return d


def layer_norm_bwd(dy, x, weight, mean, rstd, dresidual=None):
    """``dresidual``: a gradient that reaches x around the norm; added inside the kernel (dx = LN'(dy) + dresidual)."""
    dy, x = dy.contiguous(), x.contiguous()
    dres = None if dresidual is None else dresidual.contiguous()
    rows, dim = x.shape
    dx = torch.empty_like(x)
    dw, db = _f32(dim, x.device), _f32(dim, x.device)
    ws = torch.empty(L.lib().hstu_norm_bwd_workspace_bytes(rows, dim), dtype=torch.uint8, device=x.device)
    w = weight.to(x.dtype).contiguous()
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_layer_norm_bwd_residual(dy.data_ptr(), x.data_ptr(), w.data_ptr(), mean.data_ptr(),
                                                     rstd.data_ptr(), None if dres is None else dres.data_ptr(),
                                                     dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), rows, dim,
                                                     L.torch_dtype_code(x.dtype), L.current_stream_ptr(x.device)))
    return dx, dw, db


def _rows_view(t: torch.Tensor) -> torch.Tensor:
    """a 2-D tensor whose rows are contiguous (a column slice of a wider buffer stays a view)"""
    return t if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def norm_mul_fwd(attn, u, weight, bias, eps, num_heads, head_dim, group_norm, concat_ux, dropout_ratio=0.0, seed=0,
                 u_is_preactivation=False):
    """``dropout_ratio > 0``: the fused output-stage dropout (hstu_norm_mul_dropout_fwd); the mask is a function of
    (seed, element index) -- pass the same seed to norm_mul_bwd (and to a recompute of y).
    ``u_is_preactivation``: u is what goes INTO SiLU (e.g. the u slice of the uvqk buffer, read in place through its row
    stride); the kernel applies SiLU on the fly (hstu_norm_mul_silu_fwd)."""
    L.require_gpu_tensor(attn, "attn")
    attn, u = attn.contiguous(), _rows_view(u)
    rows, dim = attn.shape
    y = torch.empty((rows, 3 * dim if concat_ux else dim), dtype=attn.dtype, device=attn.device)
    ng = num_heads if group_norm else 1
    mean, rstd = _f32(rows * ng, attn.device), _f32(rows * ng, attn.device)
    w, b = weight.to(attn.dtype).contiguous(), bias.to(attn.dtype).contiguous()
    with torch.cuda.device(attn.device):
        L.check(L.lib().hstu_norm_mul_silu_fwd(attn.data_ptr(), u.data_ptr(), u.stride(0), int(bool(u_is_preactivation)),
                                               w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows,
                                               num_heads, head_dim, float(eps), int(group_norm), int(concat_ux),
                                               float(dropout_ratio), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                               L.torch_dtype_code(attn.dtype), L.current_stream_ptr(attn.device)))
    return y, mean, rstd


def norm_mul_bwd(dy, attn, u, weight, bias, mean, rstd, num_heads, head_dim, group_norm, concat_ux, dropout_ratio=0.0,
                 seed=0, u_is_preactivation=False, du=None):
    """``u_is_preactivation``: as in norm_mul_fwd; the returned du is then the gradient of the PRE-activation
    (d u * SiLU').  ``du``: where to write it (a column slice of a wider buffer is fine: the u slice of d uvqk)."""
    dy, attn, u = dy.contiguous(), attn.contiguous(), _rows_view(u)
    rows, dim = attn.shape
    dattn = torch.empty_like(attn)
    if du is None:
        du = torch.empty((rows, dim), dtype=attn.dtype, device=attn.device)
    assert du.shape == (rows, dim) and du.stride(1) == 1 and du.dtype == attn.dtype
    width = num_heads if group_norm else dim
    dw, db = _f32(width, attn.device), _f32(width, attn.device)
    ws = torch.empty(L.lib().hstu_norm_bwd_workspace_bytes(rows, dim), dtype=torch.uint8, device=attn.device)
    w, b = weight.to(attn.dtype).contiguous(), bias.to(attn.dtype).contiguous()
    with torch.cuda.device(attn.device):
        L.check(L.lib().hstu_norm_mul_silu_bwd(dy.data_ptr(), attn.data_ptr(), u.data_ptr(), u.stride(0),
                                               int(bool(u_is_preactivation)), w.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                               rstd.data_ptr(), dattn.data_ptr(), du.data_ptr(), du.stride(0), dw.data_ptr(),
                                               db.data_ptr(), ws.data_ptr(), rows, num_heads, head_dim, int(group_norm),
                                               int(concat_ux), float(dropout_ratio), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                               L.torch_dtype_code(attn.dtype), L.current_stream_ptr(attn.device)))
    return dattn, du, dw, db


def silu_fwd(x: torch.Tensor) -> torch.Tensor:
    """silu over a 2-D (possibly column-sliced) tensor -> new contiguous tensor."""
    L.require_gpu_tensor(x, "x")
    assert x.dim() == 2 and x.stride(1) == 1
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_silu_fwd(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], x.stride(0),
                                      out.stride(0), L.torch_dtype_code(x.dtype), L.current_stream_ptr(x.device)))
    return out


def silu_bwd(dout: torch.Tensor, x: torch.Tensor, din: Optional[torch.Tensor] = None) -> torch.Tensor:
    """din = dout * silu'(x); ``din`` may be a column slice of a larger buffer."""
    dout = dout if dout.stride(1) == 1 else dout.contiguous()
    assert x.stride(1) == 1
    if din is None:
        din = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_silu_bwd(dout.data_ptr(), x.data_ptr(), din.data_ptr(), x.shape[0], x.shape[1],
                                      dout.stride(0), x.stride(0), din.stride(0), L.torch_dtype_code(x.dtype),
                                      L.current_stream_ptr(x.device)))
    return din


# ----------------------------------------------------------------------------- glue around the projections (ABI v10)
def cast_params(tensors, dtype, transpose_index: Optional[int] = None):
    """fp32 CUDA parameters -> ``dtype`` (bf16 / fp16) copies in ONE launch (hstu_cast_params); the tensor at
    ``transpose_index`` (2-D) comes back as its transposed, contiguous (cols, rows) copy.  All copies are views of one flat
    buffer (each starts 16-byte aligned)."""
    n = len(tensors)
    torch._assert(0 < n <= L.CAST_MAX_ITEMS, "cast_params: 1..8 tensors")
    dev = tensors[0].device
    srcs = []
    sizes = []
    for t in tensors:
        L.require_gpu_tensor(t, "parameter")
        torch._assert(t.dtype == torch.float32 and t.device == dev, "cast_params: fp32 tensors on one device")
        srcs.append(t.detach().contiguous())
        sizes.append((t.numel() + 7) // 8 * 8)
    flat = torch.empty(sum(sizes), dtype=dtype, device=dev)
    items = (L.HstuCastItem * n)()
    outs = []
    pos = 0
    for i, (t, sz) in enumerate(zip(srcs, sizes)):
        dst = flat[pos : pos + t.numel()]
        pos += sz
        items[i].src, items[i].dst, items[i].numel = t.data_ptr(), dst.data_ptr(), t.numel()
        if i == transpose_index:
            torch._assert(t.dim() == 2, "cast_params: the transposed item must be 2-D")
            items[i].rows, items[i].cols, items[i].transpose = t.shape[0], t.shape[1], 1
            outs.append(dst.view(t.shape[1], t.shape[0]))
        else:
            items[i].rows = items[i].cols = items[i].transpose = 0
            outs.append(dst.view(t.shape))
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_cast_params(items, n, L.torch_dtype_code(dtype), L.current_stream_ptr(dev)))
    return outs


def column_sum(x: torch.Tensor, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 column sums of a 2-D bf16 / fp16 tensor with contiguous rows (hstu_column_sum: fixed summation order)"""
    L.require_gpu_tensor(x, "x")
    torch._assert(x.dim() == 2 and x.stride(1) == 1, "column_sum: a 2-D tensor with contiguous rows")
    rows, cols = x.shape
    if out is None:
        out = _f32(cols, x.device)
    if workspace is None:
        workspace = torch.empty(max(16, L.lib().hstu_column_sum_workspace_bytes(rows, cols)), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_column_sum(x.data_ptr(), x.stride(0) if rows > 1 else max(cols, x.stride(0)), rows, cols, out.data_ptr(),
                                        workspace.data_ptr(), L.torch_dtype_code(x.dtype), L.current_stream_ptr(x.device)))
    return out


def column_sum_supported(x: torch.Tensor) -> bool:
    # (stride(0) >= columns: an expanded / broadcast gradient -- row stride 0 -- is torch's to sum)
    return bool(x.is_cuda and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16) and x.stride(1) == 1 and
                x.shape[1] % 8 == 0 and x.stride(0) % 8 == 0 and x.stride(0) >= x.shape[1] and x.data_ptr() % 16 == 0)


def calib_mfma_stream(device, iters: int = 4096):
    """(launch, flop per launch): the MFMA calibration stream of bench.py (hstu_calib_mfma_stream)"""
    sink = _f32(4, device)
    flops = C.c_double(0.0)

    def launch():
        with torch.cuda.device(device):
            L.check(L.lib().hstu_calib_mfma_stream(int(iters), sink.data_ptr(), C.byref(flops), L.current_stream_ptr(device)))

    launch()
    return launch, flops.value


def calib_read_stream(src: torch.Tensor):
    """launch(): one non-temporal read of ``src`` (hstu_calib_read_stream)"""
    sink = _f32(4, src.device)
    nbytes = src.numel() * src.element_size()

    def launch():
        with torch.cuda.device(src.device):
            L.check(L.lib().hstu_calib_read_stream(src.data_ptr(), nbytes, sink.data_ptr(), L.current_stream_ptr(src.device)))

    return launch


# ----------------------------------------------------------------------------- row L2 normalisation
def l2_norm_fwd(x: torch.Tensor, eps: float) -> torch.Tensor:
    L.require_gpu_tensor(x, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    rows = x.numel() // x.shape[-1] if x.numel() else 0
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_l2_norm_fwd(x.data_ptr(), y.data_ptr(), rows, x.shape[-1], float(eps), L.torch_dtype_code(x.dtype),
                                         L.current_stream_ptr(x.device)))
    return y


def l2_norm_bwd(dy: torch.Tensor, x: torch.Tensor, eps: float) -> torch.Tensor:
    dy, x = dy.contiguous(), x.contiguous()
    dx = torch.empty_like(x)
    rows = x.numel() // x.shape[-1] if x.numel() else 0
    with torch.cuda.device(x.device):
        L.check(L.lib().hstu_l2_norm_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), rows, x.shape[-1], float(eps),
                                         L.torch_dtype_code(x.dtype), L.current_stream_ptr(x.device)))
    return dx


# ----------------------------------------------------------------------------- sampled-softmax loss
def _ss_rows(t: torch.Tensor, name: str) -> torch.Tensor:
    L.require_gpu_tensor(t, name)
    if t.dim() != 2:
        raise RuntimeError(f"{name} must be 2-D, got {tuple(t.shape)}")
    return t if t.stride(1) == 1 else t.contiguous()


def sampled_softmax_fwd(q, pos_emb, pos_ids, neg_rows, neg_ids, table, temperature, pos_l2_norm, table_l2_norm, eps):
    """-> (row_loss, lse), fp32 (n_rows)."""
    q, pos_emb, table = _ss_rows(q, "output_embeddings"), _ss_rows(pos_emb, "supervision_embeddings"), _ss_rows(table, "table")
    if not (q.dtype == pos_emb.dtype == table.dtype):
        raise RuntimeError(f"embeddings must share one dtype, got {q.dtype}, {pos_emb.dtype}, {table.dtype}")
    n, D = q.shape
    neg_rows, neg_ids, pos_ids = neg_rows.contiguous(), neg_ids.contiguous(), pos_ids.contiguous()
    if neg_rows.dtype != torch.int64 or neg_ids.dtype != torch.int64 or pos_ids.dtype != torch.int64:
        raise RuntimeError("ids must be int64")
    if neg_rows.shape != neg_ids.shape or neg_rows.dim() != 2 or neg_rows.shape[0] != n or pos_ids.shape != (n,):
        raise RuntimeError("sampled ids must be (rows, num_negatives), supervision ids (rows,)")
    row_loss = torch.empty(n, dtype=torch.float32, device=q.device)
    lse = torch.empty_like(row_loss)
    with torch.cuda.device(q.device):
        L.check(L.lib().hstu_sampled_softmax_fwd(
            q.data_ptr(), q.stride(0), pos_emb.data_ptr(), pos_emb.stride(0), pos_ids.data_ptr(), neg_rows.data_ptr(),
            neg_ids.data_ptr(), table.data_ptr(), table.stride(0), table.shape[0], n, neg_rows.shape[1], D, float(temperature),
            int(pos_l2_norm), int(table_l2_norm), float(eps), row_loss.data_ptr(), lse.data_ptr(), L.torch_dtype_code(q.dtype),
            L.current_stream_ptr(q.device)))
    return row_loss, lse


def sampled_softmax_bwd(g_row, lse, q, pos_emb, pos_ids, neg_rows, neg_ids, table, temperature, pos_l2_norm, table_l2_norm, eps):
    """-> (dq, dpos_emb) in the embedding dtype, dtable fp32 (table_rows, dim)."""
    q, pos_emb, table = _ss_rows(q, "output_embeddings"), _ss_rows(pos_emb, "supervision_embeddings"), _ss_rows(table, "table")
    n, D = q.shape
    neg_rows, neg_ids, pos_ids = neg_rows.contiguous(), neg_ids.contiguous(), pos_ids.contiguous()
    g_row = g_row.to(torch.float32).contiguous()
    dq, dpos = torch.empty_like(q), torch.empty_like(pos_emb)
    dtable = torch.zeros(table.shape[0], D, dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        L.check(L.lib().hstu_sampled_softmax_bwd(
            q.data_ptr(), q.stride(0), pos_emb.data_ptr(), pos_emb.stride(0), pos_ids.data_ptr(), neg_rows.data_ptr(),
            neg_ids.data_ptr(), table.data_ptr(), table.stride(0), table.shape[0], n, neg_rows.shape[1], D, float(temperature),
            int(pos_l2_norm), int(table_l2_norm), float(eps), lse.data_ptr(), g_row.data_ptr(), dq.data_ptr(), dq.stride(0),
            dpos.data_ptr(), dpos.stride(0), dtable.data_ptr(), L.torch_dtype_code(q.dtype), L.current_stream_ptr(q.device)))
    return dq, dpos, dtable



# ---- multitask prediction head (hstu_multitask_head_fwd / _bwd) --------------------------------------------------------
MULTITASK_MAX_TASKS = 8          # HSTU_MULTITASK_MAX_TASKS
MULTITASK_MAX_BLOCKS = 1024      # HSTU_MULTITASK_MAX_BLOCKS: grid cap of the row kernels
MULTITASK_ROWS_PER_BLOCK = 4     # HSTU_MULTITASK_ROWS_PER_BLOCK: one row per wavefront


def _rows_2d(x: torch.Tensor) -> torch.Tensor:
    """(rows, dim) with unit column stride; a column slice of a wider buffer is passed as it is (row stride)"""
    return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


def multitask_head_supported(x: torch.Tensor, num_tasks: int) -> bool:
    """whether the fused head takes (rows, dim) activations and num_tasks tasks: the dim limits of swish_layer_norm"""
    if not (x.is_cuda and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float16, torch.float32)):
        return False
    if not 1 <= num_tasks <= MULTITASK_MAX_TASKS or x.shape[1] < 1:
        return False
    es = x.element_size()
    xr = x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else None
    vec = x.shape[1] % (16 // es) == 0 and (xr is None or (xr.data_ptr() % 16 == 0 and (xr.stride(0) * es) % 16 == 0))
    return x.shape[1] <= (4096 if vec else 2048)


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.to(torch.float32).contiguous()


def multitask_head_fwd(x, ln_weight, ln_bias, eps, weight, bias, labels, weights, num_binary_tasks, loss_scale):
    """Returns (logits, preds, mean, rstd, loss, weight_sum): logits / preds (T, rows) fp32, loss / weight_sum (T) fp32 or
    None without labels (the inference form)."""
    L.require_gpu_tensor(x, "x")
    x = _rows_2d(x)
    rows, dim = x.shape
    tasks = weight.shape[0]
    dev = x.device
    g, b = ln_weight.to(x.dtype).contiguous(), ln_bias.to(x.dtype).contiguous()
    w, c = _f32c(weight), _f32c(bias)
    labels, weights = _f32c(labels), _f32c(weights)
    logits = torch.empty((tasks, rows), dtype=torch.float32, device=dev)
    preds = torch.empty((tasks, rows), dtype=torch.float32, device=dev)
    mean, rstd = _f32(rows, dev), _f32(rows, dev)
    loss = wsum = ws = None
    if labels is not None:
        loss, wsum = _f32(tasks, dev), _f32(tasks, dev)
        ws = torch.empty(L.lib().hstu_multitask_head_workspace_bytes(dim, tasks), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_multitask_head_fwd(x.data_ptr(), x.stride(0), g.data_ptr(), b.data_ptr(), float(eps), w.data_ptr(),
                                                c.data_ptr(), _vp(labels), _vp(weights), logits.data_ptr(), preds.data_ptr(),
                                                mean.data_ptr(), rstd.data_ptr(), _vp(loss), _vp(wsum), _vp(ws), rows, dim, tasks,
                                                int(num_binary_tasks), float(loss_scale), L.torch_dtype_code(x.dtype),
                                                L.current_stream_ptr(dev)))
    return logits, preds, mean, rstd, loss, wsum


def multitask_head_bwd(grad_loss, grad_pred, x, ln_weight, ln_bias, weight, labels, weights, logits, mean, rstd, weight_sum,
                       num_binary_tasks, loss_scale):
    """dx (x's dtype), dweight (T, dim), dbias (T), dln_weight, dln_bias (dim), the last four fp32"""
    x = _rows_2d(x)
    rows, dim = x.shape
    tasks = weight.shape[0]
    dev = x.device
    g, b = ln_weight.to(x.dtype).contiguous(), ln_bias.to(x.dtype).contiguous()
    w = _f32c(weight)
    labels, weights, grad_loss, grad_pred = _f32c(labels), _f32c(weights), _f32c(grad_loss), _f32c(grad_pred)
    dx = torch.empty((rows, dim), dtype=x.dtype, device=dev)
    dw = torch.empty((tasks, dim), dtype=torch.float32, device=dev)
    dc, dg, db = _f32(tasks, dev), _f32(dim, dev), _f32(dim, dev)
    ws = torch.empty(L.lib().hstu_multitask_head_workspace_bytes(dim, tasks), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_multitask_head_bwd(_vp(grad_loss), _vp(grad_pred), x.data_ptr(), x.stride(0), g.data_ptr(), b.data_ptr(),
                                                w.data_ptr(), _vp(labels), _vp(weights), logits.data_ptr(), mean.data_ptr(),
                                                rstd.data_ptr(), _vp(weight_sum), dx.data_ptr(), dx.stride(0), dw.data_ptr(),
                                                dc.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), rows, dim, tasks,
                                                int(num_binary_tasks), float(loss_scale), L.torch_dtype_code(x.dtype),
                                                L.current_stream_ptr(dev)))
    return dx, dw, dc, dg, db


# ---- input preprocessors (hstu_action_encode_* / hstu_combine_embeddings_*) ------------------------------------------
ACTION_ENCODE_MAX_TYPES = 64     # HSTU_ACTION_ENCODE_MAX_TYPES
COMBINE_SUM, COMBINE_INTERLEAVE_ALL, COMBINE_INTERLEAVE_UIH = 0, 1, 2     # HSTU_COMBINE_*
MAX_ROWS = 2**31 - 1


def _host_i64(values):
    """a host int64 array that travels as kernel arguments (kept alive by the caller for the duration of the call)"""
    values = [int(v) for v in values]
    return (C.c_int64 * max(len(values), 1))(*values)


def _i64_rows(t: Optional[torch.Tensor], name: str, rows: int) -> Optional[torch.Tensor]:
    if t is None:
        return None
    L.require_gpu_tensor(t, name)
    if t.dtype != torch.int64:
        raise RuntimeError(f"{name} must be int64, got {t.dtype}")
    if t.numel() != rows:
        raise RuntimeError(f"{name} has {t.numel()} values, {rows} expected")
    return t.contiguous().view(-1)


def _offset_pair(a: torch.Tensor, b: torch.Tensor, what: str):
    """two offset / count vectors in ONE integer type (that of the first)"""
    a = _idx(a)
    b = _idx(b)
    if b.dtype != a.dtype:
        b = b.to(a.dtype)
    if a.device != b.device:
        raise RuntimeError(f"{what}: the offset tensors live on different devices")
    return a, b


def _check_action_args(weights, thresholds, total_uih_len, total_targets) -> None:
    if not 1 <= len(weights) <= ACTION_ENCODE_MAX_TYPES:
        raise RuntimeError(f"action_encode: 1..{ACTION_ENCODE_MAX_TYPES} action types, got {len(weights)}")
    if total_uih_len < 0 or total_targets < 0 or total_uih_len + total_targets > MAX_ROWS:
        raise RuntimeError(f"action_encode: {total_uih_len} + {total_targets} rows: 0 .. 2^31 - 1 are supported")
    if len(thresholds) > len(weights):
        raise RuntimeError("action_encode: more watchtime thresholds than action types")


def action_encode_fwd(actions, watchtimes, uih_offsets, target_offsets, table, target_table, weights, thresholds,
                      total_uih_len: int, total_targets: int, dtype: torch.dtype) -> torch.Tensor:
    """(total_uih_len + total_targets, T * Da) in `dtype`.  weights: the T combined action weights (python ints);
    thresholds: [(threshold, weight)] of the watchtime rule."""
    L.require_gpu_tensor(table, "table")
    _check_action_args(weights, thresholds, total_uih_len, total_targets)
    T, da = table.shape
    if T != len(weights) or target_table.numel() != T * da:
        raise RuntimeError(f"action_encode: table {tuple(table.shape)}, target_table {tuple(target_table.shape)} and "
                           f"{len(weights)} weights do not fit together")
    dev = table.device
    actions = _i64_rows(actions, "actions", total_uih_len)
    watchtimes = _i64_rows(watchtimes, "watchtimes", total_uih_len) if thresholds else None
    uo, to = _offset_pair(uih_offsets, target_offsets, "action_encode")
    L.require_gpu_tensor(uo, "uih_offsets")
    tab, ttab = _f32c(table), _f32c(target_table)
    out = torch.empty((total_uih_len + total_targets, T * da), dtype=dtype, device=dev)
    w, th, tw = _host_i64(weights), _host_i64([t for t, _ in thresholds]), _host_i64([x for _, x in thresholds])
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_action_encode_fwd(_vp(actions), _vp(watchtimes), uo.data_ptr(), to.data_ptr(), tab.data_ptr(),
                                               ttab.data_ptr(), w, T, th, tw, len(thresholds), out.data_ptr(), total_uih_len,
                                               total_targets, uo.numel() - 1, da, L.torch_dtype_code(dtype),
                                               L.index_dtype_code(uo), L.current_stream_ptr(dev)))
    return out


def action_encode_bwd(d_out, actions, watchtimes, uih_offsets, target_offsets, weights, thresholds, total_uih_len: int,
                      total_targets: int, embedding_dim: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """d_table (T, Da) and d_target_table (1, T * Da), fp32, summed in a fixed order"""
    L.require_gpu_tensor(d_out, "d_out")
    T, da, dev = len(weights), int(embedding_dim), d_out.device
    d_out = d_out.contiguous()
    actions = _i64_rows(actions, "actions", total_uih_len)
    watchtimes = _i64_rows(watchtimes, "watchtimes", total_uih_len) if thresholds else None
    uo, to = _offset_pair(uih_offsets, target_offsets, "action_encode")
    d_table = torch.empty((T, da), dtype=torch.float32, device=dev)
    d_target = torch.empty((1, T * da), dtype=torch.float32, device=dev)
    ws = torch.empty(L.lib().hstu_action_encode_bwd_workspace_bytes(total_uih_len + total_targets, T * da), dtype=torch.uint8,
                     device=dev)
    w, th, tw = _host_i64(weights), _host_i64([t for t, _ in thresholds]), _host_i64([x for _, x in thresholds])
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_action_encode_bwd(d_out.data_ptr(), _vp(actions), _vp(watchtimes), uo.data_ptr(), to.data_ptr(), w, T,
                                               th, tw, len(thresholds), d_table.data_ptr(), d_target.data_ptr(), ws.data_ptr(),
                                               total_uih_len, total_targets, uo.numel() - 1, da,
                                               L.torch_dtype_code(d_out.dtype), L.index_dtype_code(uo),
                                               L.current_stream_ptr(dev)))
    return d_table, d_target


def combine_out_rows(mode: int, total_uih_len: int, total_targets: int, batch: int, contextual_len: int) -> int:
    """the number of output rows, from the integers the caller already holds (no device read)"""
    seq = {COMBINE_SUM: total_uih_len + total_targets, COMBINE_INTERLEAVE_ALL: 2 * (total_uih_len + total_targets),
           COMBINE_INTERLEAVE_UIH: 2 * total_uih_len + total_targets}
    if mode not in seq:
        raise RuntimeError(f"combine_embeddings: unknown mode {mode}")
    return batch * contextual_len + seq[mode]


def _check_combine(total_uih_len, total_targets, out_rows):
    if total_uih_len < 0 or total_targets < 0 or out_rows > MAX_ROWS:
        raise RuntimeError(f"combine_embeddings: {total_uih_len} + {total_targets} rows in, {out_rows} out: 0 .. 2^31 - 1 "
                           "are supported")


def combine_embeddings_fwd(content, action, contextual, timestamps, seq_offsets, num_targets, out_offsets, mode: int,
                           total_uih_len: int, total_targets: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out rows, D) embeddings and (out rows) int64 timestamps; contextual (B, C, D) or None, action (rows, D) or None"""
    L.require_gpu_tensor(content, "content_embeddings")
    L.require_gpu_tensor(timestamps, "seq_timestamps")
    if timestamps.dtype != torch.int64:
        raise RuntimeError(f"seq_timestamps must be int64, got {timestamps.dtype}")
    for name, t in (("action_embeddings", action), ("contextual_embeddings", contextual)):
        if t is not None and (t.dtype != content.dtype or t.device != content.device):
            raise RuntimeError(f"{name} is {t.dtype} on {t.device}, content_embeddings {content.dtype} on {content.device}")
    total, D = content.shape
    batch = seq_offsets.numel() - 1
    C_len = 0 if contextual is None else contextual.shape[1]
    out_rows = combine_out_rows(mode, total_uih_len, total_targets, batch, C_len)
    _check_combine(total_uih_len, total_targets, out_rows)
    if total != total_uih_len + total_targets or timestamps.numel() != total or (action is not None and action.shape != content.shape):
        raise RuntimeError(f"combine_embeddings: content {tuple(content.shape)}, {timestamps.numel()} timestamps and "
                           f"total_uih_len + total_targets = {total_uih_len + total_targets} do not fit together")
    if contextual is not None and tuple(contextual.shape) != (batch, C_len, D):
        raise RuntimeError(f"contextual_embeddings must be (B, C, D) = ({batch}, {C_len}, {D}), got {tuple(contextual.shape)}")
    so, oo = _offset_pair(seq_offsets, out_offsets, "combine_embeddings")
    nt = None if num_targets is None else _offset_pair(so, num_targets, "combine_embeddings")[1]
    content, timestamps = content.contiguous(), timestamps.contiguous()
    action = None if action is None else action.contiguous()
    contextual = None if contextual is None else contextual.contiguous()
    dev = content.device
    out = torch.empty((out_rows, D), dtype=content.dtype, device=dev)
    out_ts = torch.empty((out_rows,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_combine_embeddings_fwd(content.data_ptr(), _vp(action), _vp(contextual), timestamps.data_ptr(),
                                                    so.data_ptr(), _vp(nt), oo.data_ptr(), out.data_ptr(), out_ts.data_ptr(),
                                                    total_uih_len, total_targets, batch, C_len, D, mode,
                                                    L.torch_dtype_code(content.dtype), L.index_dtype_code(so),
                                                    L.current_stream_ptr(dev)))
    return out, out_ts


def combine_embeddings_bwd(d_out, seq_offsets, num_targets, out_offsets, mode: int, total_uih_len: int, total_targets: int,
                           contextual_len: int, want_action: bool):
    """(d_content, d_action or None, d_contextual (B, C, D) or None) in d_out's dtype: every row read from the output row
    that copied it"""
    L.require_gpu_tensor(d_out, "d_out")
    d_out = d_out.contiguous()
    D, dev = d_out.shape[1], d_out.device
    batch = seq_offsets.numel() - 1
    total = total_uih_len + total_targets
    so, oo = _offset_pair(seq_offsets, out_offsets, "combine_embeddings")
    nt = None if num_targets is None else _offset_pair(so, num_targets, "combine_embeddings")[1]
    d_content = torch.empty((total, D), dtype=d_out.dtype, device=dev)
    d_action = torch.empty((total, D), dtype=d_out.dtype, device=dev) if want_action else None
    d_ctx = torch.empty((batch, contextual_len, D), dtype=d_out.dtype, device=dev) if contextual_len > 0 else None
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_combine_embeddings_bwd(d_out.data_ptr(), so.data_ptr(), _vp(nt), oo.data_ptr(), d_content.data_ptr(),
                                                    _vp(d_action), _vp(d_ctx), total_uih_len, total_targets, batch,
                                                    contextual_len, D, mode, L.torch_dtype_code(d_out.dtype),
                                                    L.index_dtype_code(so), L.current_stream_ptr(dev)))
    return d_content, d_action, d_ctx


# ---- research-path input preprocessors (hstu_input_preprocess_*) ------------------------------------------------------
PREPROCESS_PLAIN, PREPROCESS_CONCAT, PREPROCESS_INTERLEAVE = 0, 1, 2     # HSTU_PREPROCESS_*
PREPROCESS_MAX_DIM = 4096        # HSTU_PREPROCESS_MAX_DIM


def input_preprocess_dims(layout: int, past_ids, past_embeddings, ratings, pos_table, rating_table):
    """(B, N, N', Di, Dr, Do, P, R) of a call, or RuntimeError -- from the shapes alone, before any tensor is touched"""
    if layout not in (PREPROCESS_PLAIN, PREPROCESS_CONCAT, PREPROCESS_INTERLEAVE):
        raise RuntimeError(f"input_preprocess: unknown layout {layout}")
    if past_ids.dim() != 2 or past_embeddings.dim() != 3 or tuple(past_embeddings.shape[:2]) != tuple(past_ids.shape):
        raise RuntimeError(f"input_preprocess: past_ids (B, N) and past_embeddings (B, N, Di) expected, got "
                           f"{tuple(past_ids.shape)} and {tuple(past_embeddings.shape)}")
    if pos_table.dim() != 2:
        raise RuntimeError(f"input_preprocess: the position table is (P, Do), got {tuple(pos_table.shape)}")
    B, N, Di = past_embeddings.shape
    P = pos_table.shape[0]
    Dr = R = 0
    if layout != PREPROCESS_PLAIN:
        if ratings is None or rating_table is None:
            raise RuntimeError("input_preprocess: the rated layouts need ratings and the rating table")
        if tuple(ratings.shape) != (B, N) or rating_table.dim() != 2:
            raise RuntimeError(f"input_preprocess: ratings (B, N) and a rating table (R, Dr) expected, got "
                               f"{tuple(ratings.shape)} and {tuple(rating_table.shape)}")
        R, Dr = rating_table.shape
        if layout == PREPROCESS_INTERLEAVE and Dr != Di:
            raise RuntimeError(f"input_preprocess: interleaving needs rating rows as wide as the item rows, got {Dr} and {Di}")
    Do = Di + Dr if layout == PREPROCESS_CONCAT else Di
    n_out = 2 * N if layout == PREPROCESS_INTERLEAVE else N
    if pos_table.shape[1] != Do:
        raise RuntimeError(f"input_preprocess: the position table has {pos_table.shape[1]} columns, the output rows {Do}")
    if n_out > P:
        raise RuntimeError(f"input_preprocess: {n_out} output positions but the position table has {P} rows")
    if Do > PREPROCESS_MAX_DIM:
        raise RuntimeError(f"input_preprocess: rows of at most {PREPROCESS_MAX_DIM} columns, got {Do}")
    if B * n_out > MAX_ROWS:
        raise RuntimeError(f"input_preprocess: {B} x {n_out} output rows: at most 2^31 - 1 are supported")
    return B, N, n_out, Di, Dr, Do, P, R


def _preprocess_ints(past_ids, ratings):
    if past_ids.dtype != torch.int64:
        past_ids = past_ids.to(torch.int64)
    return past_ids.contiguous(), (None if ratings is None else _idx(ratings))


def input_preprocess_fwd(layout: int, past_ids, past_embeddings, ratings, pos_table, rating_table, dropout_ratio: float,
                         seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out (B, N', Do) in result_type(past_embeddings, pos_table), valid_mask (B, N', 1) fp32)"""
    B, N, n_out, Di, Dr, Do, P, R = input_preprocess_dims(layout, past_ids, past_embeddings, ratings, pos_table, rating_table)
    for t, name in ((past_embeddings, "past_embeddings"), (past_ids, "past_ids"), (pos_table, "pos_table")):
        L.require_gpu_tensor(t, name)
    if layout != PREPROCESS_PLAIN:
        L.require_gpu_tensor(ratings, "ratings")
        L.require_gpu_tensor(rating_table, "rating_table")
    dev = past_embeddings.device
    out_dtype = torch.result_type(past_embeddings, pos_table)
    emb = past_embeddings.contiguous()
    if emb.dtype != out_dtype and out_dtype != torch.float32:       # bf16 against fp16: torch promotes both to fp32
        raise RuntimeError(f"input_preprocess: {emb.dtype} embeddings into a {pos_table.dtype} table")
    pos = pos_table.detach().to(out_dtype).contiguous()
    rat = None if layout == PREPROCESS_PLAIN else rating_table.detach().to(out_dtype).contiguous()
    ids, rt = _preprocess_ints(past_ids, ratings if layout != PREPROCESS_PLAIN else None)
    out = torch.empty((B, n_out, Do), dtype=out_dtype, device=dev)
    valid = torch.empty((B, n_out, 1), dtype=torch.float32, device=dev)
    if B == 0 or N == 0:
        return out, valid
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_input_preprocess_fwd(ids.data_ptr(), emb.data_ptr(), _vp(rt), pos.data_ptr(), _vp(rat), out.data_ptr(),
                                                  valid.data_ptr(), B, N, Di, Dr, P, R, layout, float(dropout_ratio), int(seed),
                                                  L.torch_dtype_code(emb.dtype), L.torch_dtype_code(out_dtype),
                                                  L.index_dtype_code(rt) if rt is not None else L.HSTU_INDEX_I64,
                                                  L.current_stream_ptr(dev)))
    return out, valid


def input_preprocess_bwd(layout: int, d_out, past_ids, ratings, emb_dtype: torch.dtype, item_dim: int, num_positions: int,
                         rating_shape: Optional[Tuple[int, int]], dropout_ratio: float, seed: int, need_emb: bool = True,
                         need_pos: bool = True, need_rating: bool = True):
    """(d_past_embeddings in `emb_dtype`, d_pos (P, Do) fp32, d_rating (R, Dr) fp32); what is not needed is None.  The table
    gradients are fp32 sums in a fixed order."""
    L.require_gpu_tensor(d_out, "d_out")
    dev = d_out.device
    d_out = d_out.contiguous()
    B, N = past_ids.shape
    Do = d_out.shape[-1]
    R, Dr = rating_shape if layout != PREPROCESS_PLAIN else (0, 0)
    need_rating = need_rating and layout != PREPROCESS_PLAIN
    ids, rt = _preprocess_ints(past_ids, ratings if layout != PREPROCESS_PLAIN else None)
    if not (need_emb or need_pos or need_rating):
        return None, None, None
    d_emb = torch.empty((B, N, item_dim), dtype=emb_dtype, device=dev) if need_emb else None
    d_pos = torch.empty((num_positions, Do), dtype=torch.float32, device=dev) if need_pos else None
    d_rat = torch.empty((R, Dr), dtype=torch.float32, device=dev) if need_rating else None
    ws = None
    if need_pos or need_rating:
        ws = torch.empty(max(32, L.lib().hstu_input_preprocess_bwd_workspace_bytes(B, N, item_dim, Dr, R, layout)),
                         dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_input_preprocess_bwd(d_out.data_ptr(), ids.data_ptr(), _vp(rt), _vp(d_emb), _vp(d_pos), _vp(d_rat),
                                                  _vp(ws), B, N, item_dim, Dr, num_positions, R, layout, float(dropout_ratio),
                                                  int(seed), L.torch_dtype_code(emb_dtype), L.torch_dtype_code(d_out.dtype),
                                                  L.index_dtype_code(rt) if rt is not None else L.HSTU_INDEX_I64,
                                                  L.current_stream_ptr(dev)))
    return d_emb, d_pos, d_rat


# ---- timestamp postprocessor (hstu_time_features / hstu_time_ln_*) ---------------------------------------------------
TIME_LN_MAX_PERIODS = 4          # HSTU_TIME_LN_MAX_PERIODS


def _periods(period_units: torch.Tensor, units_per_period: torch.Tensor, device):
    """the module's (1, F) buffers as two contiguous fp32 device arrays of F numbers"""
    pu = period_units.detach().reshape(-1).to(device=device, dtype=torch.float32).contiguous()
    upp = units_per_period.detach().reshape(-1).to(device=device, dtype=torch.float32).contiguous()
    torch._assert(pu.numel() == upp.numel(), "period_units and units_per_period must have one entry per period")
    return pu, upp


def time_ln_supported(dim: int, num_periods: int, dtype: torch.dtype) -> bool:
    """whether the fused row pass takes rows of ``dim`` elements with ``num_periods`` periods: contiguous rows of fresh
    allocations are 16-byte aligned, so the class is the vector one whenever dim is a multiple of the piece"""
    if dtype not in (torch.bfloat16, torch.float16, torch.float32) or not 1 <= num_periods <= TIME_LN_MAX_PERIODS or dim < 1:
        return False
    piece = 4 if dtype == torch.float32 else 8
    return dim <= (4096 if dim % piece == 0 else 2048)


def time_features(timestamps: torch.Tensor, period_units: torch.Tensor, units_per_period: torch.Tensor) -> torch.Tensor:
    """(rows, 2F) fp32 [cos, sin] per period of int64 timestamps: the reference's fp32 arithmetic (hstu_time_features)"""
    L.require_gpu_tensor(timestamps, "timestamps")
    t = timestamps.reshape(-1).to(torch.int64).contiguous()
    pu, upp = _periods(period_units, units_per_period, t.device)
    out = torch.empty((t.numel(), 2 * pu.numel()), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        L.check(L.lib().hstu_time_features(t.data_ptr(), pu.data_ptr(), upp.data_ptr(), pu.numel(), out.data_ptr(), t.numel(),
                                           L.current_stream_ptr(t.device)))
    return out


def time_ln_fwd(z0, timestamps, period_units, units_per_period, b, wt, ln_weight, ln_bias, eps):
    """y = LayerNorm(z0 + b + tf(timestamps) @ wt) ln_weight + ln_bias in one row pass: returns (y, mean, rstd).  ``wt``
    (2F, dim), ``b``, ``ln_weight``, ``ln_bias`` are fp32."""
    L.require_gpu_tensor(z0, "z0")
    z0 = z0.contiguous()
    rows, dim = z0.shape
    t = timestamps.reshape(-1).to(torch.int64).contiguous()
    torch._assert(t.numel() == rows, "one timestamp per row")
    pu, upp = _periods(period_units, units_per_period, z0.device)
    b, wt, g, h = _f32c(b), _f32c(wt), _f32c(ln_weight), _f32c(ln_bias)
    torch._assert(wt.shape == (2 * pu.numel(), dim), "wt must be (2F, dim)")
    y = torch.empty_like(z0)
    mean, rstd = _f32(rows, z0.device), _f32(rows, z0.device)
    with torch.cuda.device(z0.device):
        L.check(L.lib().hstu_time_ln_fwd(z0.data_ptr(), t.data_ptr(), pu.data_ptr(), upp.data_ptr(), pu.numel(), b.data_ptr(),
                                         wt.data_ptr(), g.data_ptr(), h.data_ptr(), float(eps), y.data_ptr(), mean.data_ptr(),
                                         rstd.data_ptr(), rows, dim, L.torch_dtype_code(z0.dtype), L.current_stream_ptr(z0.device)))
    return y, mean, rstd


def time_ln_bwd(dy, z0, timestamps, period_units, units_per_period, b, wt, ln_weight, mean, rstd):
    """dz (z0's dtype) and the fp32 column sums dln_weight, dln_bias, db (dim), dwt (2F, dim) of time_ln_fwd"""
    dy, z0 = dy.contiguous(), z0.contiguous()
    rows, dim = z0.shape
    dev = z0.device
    t = timestamps.reshape(-1).to(torch.int64).contiguous()
    pu, upp = _periods(period_units, units_per_period, dev)
    b, wt, g = _f32c(b), _f32c(wt), _f32c(ln_weight)
    dz = torch.empty_like(z0)
    dg, dh, db = _f32(dim, dev), _f32(dim, dev), _f32(dim, dev)
    dwt = torch.empty((2 * pu.numel(), dim), dtype=torch.float32, device=dev)
    ws = torch.empty(L.lib().hstu_time_ln_workspace_bytes(dim, pu.numel()), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().hstu_time_ln_bwd(dy.data_ptr(), z0.data_ptr(), t.data_ptr(), pu.data_ptr(), upp.data_ptr(), pu.numel(),
                                         b.data_ptr(), wt.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dz.data_ptr(),
                                         dg.data_ptr(), dh.data_ptr(), db.data_ptr(), dwt.data_ptr(), ws.data_ptr(), rows, dim,
                                         L.torch_dtype_code(z0.dtype), L.current_stream_ptr(dev)))
    return dz, dg, dh, db, dwt


# ------------------------------------------------------------------ jagged causal softmax attention (the SASRec baseline)
SOFTMAX_ATTN_MAX_HEAD_DIM = 64
SOFTMAX_ATTN_MAX_SEQ_LEN = 512


def softmax_attn_supported(dtype: torch.dtype, head_dim: int, max_seq_len: int) -> bool:
    """whether the fused kernels take this (dtype, REAL head dim, max_seq_len): hstu_softmax_attn_supported"""
    if dtype not in (torch.bfloat16, torch.float16, torch.float32):
        return False
    return 1 <= int(head_dim) <= SOFTMAX_ATTN_MAX_HEAD_DIM and 1 <= int(max_seq_len) <= SOFTMAX_ATTN_MAX_SEQ_LEN


def _softmax_attn_check(q, k, v, seq_offsets):
    for name, t in (("q", q), ("k", k), ("v", v), ("seq_offsets", seq_offsets)):
        L.require_gpu_tensor(t, name)
    if not (q.dtype == k.dtype == v.dtype):
        raise RuntimeError("q, k, v must have the same dtype")
    if not (q.dim() == 3 and q.shape == k.shape == v.shape):
        raise RuntimeError(f"q, k, v must be (L, H, d) with one head dim, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")


def softmax_attn_fwd(q, k, v, seq_offsets, max_seq_len, scale, dropout_p=0.0, seed=0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out (L, H, d), lse (L, H) fp32) of the jagged causal softmax attention; q, k, v (L, H, d) with d a multiple of 16
    bytes, any row / head strides (hstu_softmax_attn_fwd).  ``lse`` is taken of the un-dropped scores."""
    _softmax_attn_check(q, k, v, seq_offsets)
    q, k, v = _aligned_rows(q), _aligned_rows(k), _aligned_rows(v)
    seq_offsets = _idx(seq_offsets)
    rows, heads, d = q.shape
    out = torch.empty((rows, heads, d), dtype=q.dtype, device=q.device)
    lse = torch.empty((rows, heads), dtype=torch.float32, device=q.device)
    if rows == 0 or seq_offsets.numel() < 2:
        return out, lse
    if DEBUG_CHECKS:
        _check_attention_metadata(q, seq_offsets, max_seq_len, 0)
    with torch.cuda.device(q.device):
        L.check(L.lib().hstu_softmax_attn_fwd(
            q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(), v.stride(0), v.stride(1),
            out.data_ptr(), lse.data_ptr(), seq_offsets.data_ptr(), rows, seq_offsets.numel() - 1, heads, d, int(max_seq_len),
            float(scale), float(dropout_p), int(seed), L.torch_dtype_code(q.dtype), L.index_dtype_code(seq_offsets),
            L.current_stream_ptr(q.device)))
    return out, lse


def softmax_attn_bwd(dout, q, k, v, out, lse, seq_offsets, max_seq_len, scale, dropout_p=0.0, seed=0):
    """(dq, dk, dv), contiguous (L, H, d), of softmax_attn_fwd; P is recomputed from q, k and ``lse`` and the dropout mask
    from ``seed``.  No float atomics: bit-identical run to run (hstu_softmax_attn_bwd)."""
    _softmax_attn_check(q, k, v, seq_offsets)
    q, k, v = _aligned_rows(q), _aligned_rows(k), _aligned_rows(v)
    seq_offsets = _idx(seq_offsets)
    dout, out, lse = dout.contiguous(), out.contiguous(), lse.contiguous()
    rows, heads, d = q.shape
    dq, dk, dv = (torch.empty((rows, heads, d), dtype=q.dtype, device=q.device) for _ in range(3))
    if rows == 0 or seq_offsets.numel() < 2:
        return dq, dk, dv
    delta = torch.empty((rows, heads), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        L.check(L.lib().hstu_softmax_attn_bwd(
            dout.data_ptr(), q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(),
            v.stride(0), v.stride(1), out.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(),
            dv.data_ptr(), seq_offsets.data_ptr(), rows, seq_offsets.numel() - 1, heads, d, int(max_seq_len), float(scale),
            float(dropout_p), int(seed), L.torch_dtype_code(q.dtype), L.index_dtype_code(seq_offsets),
            L.current_stream_ptr(q.device)))
    return dq, dk, dv
