"""CPU tests of the row-wise e4m3 UVQK projection's host side: the restatement of its quantizer against torch's own e4m3
conversion, every refusal of the four C entry points (before any launch: no GPU is present here), the shape sweep of
_supported, and the ABI.  No kernel is launched."""

import ctypes as C

import pytest
import torch

import fp8_linear_ref as R

BF16, F16, F32 = 1, 2, 0


@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def codes():
    from generative_recommenders_amd import _lib

    return {torch.bfloat16: _lib.torch_dtype_code(torch.bfloat16), torch.float16: _lib.torch_dtype_code(torch.float16),
            torch.float32: _lib.torch_dtype_code(torch.float32)}


def test_reference_quantizer_is_torchs_e4m3_rule_bit_for_bit():
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        src = (torch.randn(37, 512, generator=g) * (0.1 + 10 * torch.rand(37, 1, generator=g))).to(dtype)
        src[5] = 0                       # a zero row: scale 1.0, codes 0
        src[7, :-1] *= 0.01              # amax in the last column
        src[7, -1] = 3.0
        q, scale = R.quantize_rows(src)
        amax = src.float().abs().amax(dim=1)
        assert scale[5].item() == 1.0 and torch.equal(q[5].view(torch.uint8), torch.zeros(512, dtype=torch.uint8))
        assert scale[7].item() == (torch.tensor(3.0, dtype=dtype).float() / 448.0).item()
        want_scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        assert torch.equal(scale, want_scale) and scale.dtype == torch.float32
        want = (src.float() / want_scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
        assert torch.equal(q.view(torch.uint8), want.view(torch.uint8))
        # every row's amax lands on +-448 exactly
        assert torch.equal(q.float().abs().amax(dim=1)[amax > 0], torch.full((36,), 448.0))


def test_abi_is_still_13_and_the_symbols_are_there(lib):
    import os

    assert lib.hstu_abi_version() == 13
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hstu_hip.h")).read()
    assert "#define HSTU_ABI_VERSION 13" in hdr
    for name in ("hstu_quantize_rows_fp8", "hstu_ln_linear_fp8_fwd", "hstu_linear_fp8_rowwise", "hstu_ln_linear_fp8_supported"):
        assert hasattr(lib, name) and name + "(" in hdr, name


def test_supported_sweep(lib, codes):
    for k in (0, 16, 256, 448, 511, 512, 513, 1024):
        for n in (-32, 0, 16, 31, 32, 33, 96, 2048, 4064, 4096, 4128, 8192):
            for dt in (torch.bfloat16, torch.float16, torch.float32):
                want = dt != torch.float32 and k == 512 and 0 < n <= 4096 and n % 32 == 0
                assert bool(lib.hstu_ln_linear_fp8_supported(1000, k, n, codes[dt])) == want, (k, n, dt)
    assert not lib.hstu_ln_linear_fp8_supported(1000, 512, 2048, 3)      # e4m3 itself is no I/O type
    assert not lib.hstu_ln_linear_fp8_supported(1000, 512, 2048, 99)


def _buf(nbytes=1 << 16):
    b = (C.c_char * (nbytes + 64))()
    a = (C.addressof(b) + 63) & ~63
    return b, a


def test_quantize_rows_refusals(lib, codes):
    keep, a = _buf()
    bf = codes[torch.bfloat16]
    assert lib.hstu_quantize_rows_fp8(a, 512, 0, 512, bf, a, a, None) == 0                    # no rows: nothing to do
    assert lib.hstu_quantize_rows_fp8(None, 512, 4, 512, bf, a, a, None) == -1
    assert lib.hstu_quantize_rows_fp8(a, 512, 4, 512, bf, None, a, None) == -1
    assert lib.hstu_quantize_rows_fp8(a, 512, 4, 512, bf, a, None, None) == -1 and b"NULL" in lib.hstu_last_error()
    assert lib.hstu_quantize_rows_fp8(a, 512, 4, 512, 3, a, a, None) == -1 and b"bf16, fp16 or fp32" in lib.hstu_last_error()
    for k in (0, 8, 24, 4112, 8192, -16):
        assert lib.hstu_quantize_rows_fp8(a, 8192, 4, k, bf, a, a, None) == -2, k
    assert b"multiple of 16" in lib.hstu_last_error()
    assert lib.hstu_quantize_rows_fp8(a, 256, 4, 512, bf, a, a, None) == -1                   # ld < k
    assert lib.hstu_quantize_rows_fp8(a, 512, -1, 512, bf, a, a, None) == -1
    assert lib.hstu_quantize_rows_fp8(a + 2, 512, 4, 512, bf, a, a, None) == -1 and b"aligned" in lib.hstu_last_error()
    assert lib.hstu_quantize_rows_fp8(a, 516, 4, 512, bf, a, a, None) == -1                   # rows of 1032 bytes
    assert lib.hstu_quantize_rows_fp8(a, 512, 4, 512, bf, a + 8, a, None) == -1
    assert lib.hstu_quantize_rows_fp8(a, 514, 4, 512, codes[torch.float32], a, a, None) == -1
    del keep


def _fused(lib, a, dt, **kw):
    p = dict(x=a, ldx=512, lw=a, lb=a, eps=1e-6, wq=a, ws=a, bias=a, y=a, ldy=2048, xq=a, xs=a, mean=a, rstd=a, rows=8, k=512,
             n=2048, dtype=dt)
    p.update(kw)
    return lib.hstu_ln_linear_fp8_fwd(p["x"], p["ldx"], p["lw"], p["lb"], p["eps"], p["wq"], p["ws"], p["bias"], p["y"], p["ldy"],
                                      p["xq"], p["xs"], p["mean"], p["rstd"], p["rows"], p["k"], p["n"], p["dtype"], None)


def test_ln_linear_fp8_fwd_refusals(lib, codes):
    keep, a = _buf()
    bf = codes[torch.bfloat16]
    assert _fused(lib, a, bf, rows=0) == 0
    for name in ("x", "lw", "lb", "wq", "ws", "y"):
        assert _fused(lib, a, bf, **{name: None}) == -1 and b"NULL" in lib.hstu_last_error(), name
    for kw in (dict(k=256), dict(k=1024), dict(n=0), dict(n=48), dict(n=4128), dict(dtype=codes[torch.float32]), dict(dtype=3)):
        assert _fused(lib, a, bf, **kw) == -2, kw
        assert b"k == 512" in lib.hstu_last_error()
    for kw in (dict(rows=-1), dict(ldx=256), dict(ldy=1024), dict(ldx=516), dict(ldy=2052), dict(x=a + 2), dict(wq=a + 4),
               dict(y=a + 8), dict(xq=a + 1)):
        assert _fused(lib, a, bf, **kw) == -1, kw
    del keep


def _plain(lib, a, dt, **kw):
    p = dict(xq=a, xs=a, wq=a, ws=a, bias=a, y=a, ldy=2048, rows=8, k=512, n=2048, dtype=dt)
    p.update(kw)
    return lib.hstu_linear_fp8_rowwise(p["xq"], p["xs"], p["wq"], p["ws"], p["bias"], p["y"], p["ldy"], p["rows"], p["k"], p["n"],
                                       p["dtype"], None)


def test_linear_fp8_rowwise_refusals(lib, codes):
    keep, a = _buf()
    f16 = codes[torch.float16]
    assert _plain(lib, a, f16, rows=0) == 0
    for name in ("xq", "xs", "wq", "ws", "y"):
        assert _plain(lib, a, f16, **{name: None}) == -1 and b"NULL" in lib.hstu_last_error(), name
    for kw in (dict(k=256), dict(n=16), dict(n=8192), dict(dtype=codes[torch.float32]), dict(dtype=3)):
        assert _plain(lib, a, f16, **kw) == -2, kw
    for kw in (dict(rows=-3), dict(ldy=64), dict(ldy=2052), dict(xq=a + 4), dict(wq=a + 8), dict(y=a + 2)):
        assert _plain(lib, a, f16, **kw) == -1, kw
    del keep


def test_flag_on_a_shape_the_kernel_does_not_take_raises_on_the_cpu():
    """CPU tensors: the limit is named, nothing falls back to 16 bits"""
    from generative_recommenders_amd.ops.hstu_compute import hstu_compute_uqvk

    x = torch.randn(4, 512).bfloat16()
    w = torch.randn(512, 256).bfloat16()
    with pytest.raises(ValueError, match="fp8_in_addmm_fwd needs CUDA"):
        hstu_compute_uqvk(x, torch.ones(512), torch.zeros(512), 1e-6, 1, 64, 64, w, torch.zeros(256), fp8_in_addmm_fwd=True)


def test_config_field_defaults_off():
    from generative_recommenders_amd.modules.stu import STULayerConfig

    c = STULayerConfig(embedding_dim=512, num_heads=4, hidden_dim=128, attention_dim=128)
    assert c.fp8_in_addmm_fwd is False
