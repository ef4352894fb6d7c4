"""CPU tests of the fp8 (e4m3) attention forward's host side: the C ABI's dtype code, dispatch names and argument checks, the
Meta kernels of the hstu:: operators on fp8 inputs, and the quantizer's specification on the torch expression.  No kernel is
launched."""

import ctypes as C

import numpy as np
import pytest
import torch

FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    return _lib.lib()


def test_dtype_code_and_header_constant():
    import os

    from generative_recommenders_amd import _lib

    assert _lib.torch_dtype_code(FP8) == _lib.HSTU_DTYPE_FP8_E4M3 == 3
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hstu_hip.h")).read()
    assert "HSTU_DTYPE_FP8_E4M3 = 3" in hdr
    with pytest.raises(RuntimeError):
        _lib.torch_dtype_code(torch.float8_e5m2)


def test_kernel_names_for_the_fp8_dtype(lib):
    from generative_recommenders_amd.ops import _launch

    assert _launch.attn_fwd_kernel_name(FP8, 128, 128, 200) == "hstu_attn_fwd_fp8_kernel<fp8,128,128>"
    assert _launch.attn_fwd_kernel_name(FP8, 64, 64, 8192) == "hstu_attn_fwd_fp8_kernel<fp8,64,64>"
    assert _launch.attn_fwd_kernel_name(FP8, 32, 32, 200) == "hstu_attn_fwd_fp8_kernel<fp8,64,64>"   # padded to 64
    for dqk, dv in ((64, 128), (192, 192), (24, 24)):
        with pytest.raises(RuntimeError):
            _launch.attn_fwd_kernel_name(FP8, dqk, dv, 200)
    with pytest.raises(RuntimeError, match="bias"):
        _launch.attn_fwd_kernel_name(FP8, 64, 64, 200, with_bias=True)
    with pytest.raises(RuntimeError, match="fp8"):
        _launch.attn_bwd_kernel_name(FP8, 128, 128, 200)
    # the 16-bit names are unchanged
    assert _launch.attn_fwd_kernel_name(torch.bfloat16, 128, 128, 200) == "hstu_attn_fwd_kernel<bf16,128,128>"


def _params(dtype=3, d=64):
    from generative_recommenders_amd import _lib

    p = _lib.HstuAttnParams()
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 15) & ~15
    p.q = p.k = p.v = p.out = p.seq_offsets = addr
    p.batch, p.heads, p.max_seq_len, p.dqk, p.dv = 1, 1, 8, d, d
    p.q_row_stride = p.k_row_stride = p.v_row_stride = p.o_row_stride = d
    p.q_head_stride = p.k_head_stride = p.v_head_stride = p.o_head_stride = d
    p.dtype = dtype
    p.alpha, p.scale = 1.0, 0.125
    return p, buf


def test_c_abi_validation_without_gpu(lib):
    from generative_recommenders_amd import _lib

    ds = _lib.HstuFp8Descale()
    p, _keep = _params(d=64)
    p.dv = 128
    assert lib.hstu_attn_fwd_fp8(C.byref(p), C.byref(ds), None) == -2 and b"dqk == dv" in lib.hstu_last_error()
    p, _keep = _params(d=24)
    assert lib.hstu_attn_fwd(C.byref(p), None) == -1 and b"multiples of 16" in lib.hstu_last_error()
    p, _keep = _params(d=192)
    assert lib.hstu_attn_fwd(C.byref(p), None) == -2 and b"above 128" in lib.hstu_last_error()
    p, _keep = _params(d=64)
    p.pos_w = p.q
    assert lib.hstu_attn_fwd_fp8(C.byref(p), None, None) == -2 and b"bias" in lib.hstu_last_error()
    p, _keep = _params(d=64)
    p.k_row_stride = 72
    assert lib.hstu_attn_fwd(C.byref(p), None) == -1 and b"16-byte" in lib.hstu_last_error()
    p, _keep = _params(dtype=0, d=64)
    assert lib.hstu_attn_fwd_fp8(C.byref(p), C.byref(ds), None) == -1 and b"FP8" in lib.hstu_last_error()
    # an empty batch launches nothing
    p, _keep = _params(d=64)
    p.batch = 0
    assert lib.hstu_attn_fwd_fp8(C.byref(p), C.byref(ds), None) == 0
    # the backward refuses fp8 by name, before anything else
    bp = _lib.HstuAttnBwdParams()
    bp.fwd, _keep = _params(d=64)
    assert lib.hstu_attn_bwd(C.byref(bp), None) == -2 and b"fp8" in lib.hstu_last_error()
    assert lib.hstu_attn_bwd_workspace_bytes(C.byref(bp)) == 0
    # the quantizer's argument checks
    assert lib.hstu_jagged_quantize_fp8(None, 0, 0, None, None, None, 1, 1, 8, 0, 1, None) == -1
    buf = (C.c_char * 64)()
    a = C.addressof(buf)
    assert lib.hstu_jagged_quantize_fp8(a, 8, 8, a, a, a, 1, 1, 8, 3, 1, None) == -1 and b"bf16, fp16 or fp32" in lib.hstu_last_error()
    assert lib.hstu_jagged_quantize_fp8(a, 8, 8, a, a, a, 0, 1, 8, 0, 1, None) == 0


def test_meta_kernels_return_bf16_for_fp8_inputs():
    from generative_recommenders_amd.ops import torch_library

    torch_library.register()
    m = lambda *shape, dtype=FP8: torch.empty(*shape, dtype=dtype, device="meta")  # noqa: E731
    q, off = m(10, 2, 64), m(3, dtype=torch.int64)
    ds = m(2, 2, dtype=torch.float32)
    o = torch.ops.hstu.hstu_mha_fwd(20, 0.25, q, q, q, off, True, None, None, 0, 0, 0, ds, ds, ds, 0)
    assert o.shape == (10, 2, 64) and o.dtype == torch.bfloat16
    o = torch.ops.hstu.hstu_mha(20, 0.25, q, q, q, off, True, None, None, 0, 0, 0, None, None, None, False, False, 0)
    assert o.shape == (10, 2, 64) and o.dtype == torch.bfloat16
    qd = m(3, 20, 2, 128)
    o = torch.ops.hstu.hstu_mha_fwd(20, 0.25, qd, qd, qd, None, True, None, None, 0, 0, 0, None, None, None, 0)
    assert o.shape == (3, 20, 2, 128) and o.dtype == torch.bfloat16
    # 16-bit inputs keep their dtype
    b = m(10, 2, 64, dtype=torch.bfloat16)
    assert torch.ops.hstu.hstu_mha_fwd(20, 0.25, b, b, b, off, True, None, None, 0, 0, 0, None, None, None, 0).dtype == torch.bfloat16


def test_python_entry_points_refuse_cpu_tensors_and_bad_dtypes():
    from generative_recommenders_amd.ops import fp8

    x = torch.randn(10, 2, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        fp8.quantize_jagged_fp8(x, torch.tensor([0, 4, 10]))
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fp8.hstu_mha_fp8(10, 0.1, x, x, x, torch.tensor([0, 4, 10]))


def _spec_quantize(x: torch.Tensor, offsets: torch.Tensor):
    """the quantizer's contract as a torch expression (what the GPU kernel must equal bit for bit)"""
    B, H = offsets.numel() - 1, x.shape[1]
    ds = torch.ones(B, H)
    for b in range(B):
        s, e = int(offsets[b]), int(offsets[b + 1])
        if e > s:
            amax = x[s:e].float().abs().amax(dim=(0, 2))
            ds[b] = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    rows = torch.repeat_interleave(ds, offsets[1:] - offsets[:-1], dim=0)
    return (x.float() / rows[:, :, None]).clamp(-448, 448).to(FP8), ds


def test_quantizer_spec_on_the_torch_expression():
    rng = np.random.default_rng(0)
    lengths = [0, 5, 31, 0, 2]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]))
    x = torch.from_numpy(rng.standard_normal((int(off[-1]), 3, 32)) * 50).to(torch.bfloat16)
    x[5:36, 2] = 0
    x8, ds = _spec_quantize(x, off)
    assert ds.shape == (5, 3) and bool((ds[0] == 1).all()) and bool((ds[3] == 1).all()) and float(ds[2, 2]) == 1.0
    y = x8.float()
    assert bool(torch.isfinite(y).all())                      # clamping first: torch's cast turns overflow into NaN
    assert float(y.abs().max()) == 448.0                      # every (user, head) amax lands on e4m3's largest finite value
    assert torch.isnan(torch.tensor([500.0]).to(FP8).float()).all()
    # dequantized error: half an e4m3 ulp (3 mantissa bits) of the value, or half the subnormal quantum
    rows = torch.repeat_interleave(ds, off[1:] - off[:-1], dim=0)[:, :, None]
    err = (y * rows - x.float()).abs()
    bound = torch.maximum(x.float().abs() * 2.0**-4, 2.0**-10 * rows) * (1 + 1e-6)
    assert bool((err <= bound).all())
    # round to nearest even at a tie: 1 + 1/16 lies half-way between 1 and 1.125
    assert float(torch.tensor([1.0625, 1.1875]).to(FP8).float()[0]) == 1.0
    assert float(torch.tensor([1.0625, 1.1875]).to(FP8).float()[1]) == 1.25
