"""RMS norm on the GPU: every dispatch class of the kernels against fp64, the reference's own RMSNorm (fixture), autograd wiring.

The rows of tests/rms_norm_cases.py -- each labelled with the instantiation it reaches, which tests/test_rms_norm_host.py
verifies on the CPU -- run through the C ABI with raw pointers in the layout of tests/test_norm_classes_gpu.py: every tensor
of a call sits alone inside a sentinel-filled allocation, PAD elements in, one more when the row misaligns it, so that the
results are compared with an fp64 evaluation of the formulas (never with another kernel), everything outside the tensor must
still hold the sentinel, and a refused call must have written nothing.

Tolerances are the project's layer-norm ones, restated from tests/test_norm_classes_gpu.py: GATE (relative Frobenius) and ELEM
(element tolerance) for y and dx, WGRAD_F32 / WGRAD_16 for dweight."""

import os
import zlib

import numpy as np
import pytest
import torch

import rms_norm_cases as T
from conftest import GOLDEN, record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77.0          # exactly representable in bf16 / fp16 / fp32; no kernel output of these inputs comes near it
EPS = 1e-5

# relative Frobenius gate by dtype and element tolerance (rtol, atol as a fraction of max|ref|): test_norm_classes_gpu's
GATE = {torch.float32: 1.5e-6, torch.bfloat16: 2.8e-3, torch.float16: 3.2e-4}
ELEM = {torch.float32: (1e-3, 2e-5), torch.bfloat16: (2e-2, 4e-3), torch.float16: (2e-2, 4e-3)}
# weight gradients: fp32 outputs of fp32 math on exact inputs (the C ABI) are held to the fp32 bar; through autograd with a
# 16-bit parameter dweight comes back rounded to the parameter's dtype: the 16-bit bar
WGRAD_F32 = (torch.float32, 1e-3, 1e-4)
WGRAD_16 = (None, 3e-2, 1e-2)


def _lib():
    from generative_recommenders_amd import _lib as L

    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """a (rows, cols) tensor `off` elements into its own sentinel-filled allocation"""

    def __init__(self, rows, cols, dtype, off=T.PAD, data=None, fill=SENT):
        self.rows, self.cols, self.off = rows, cols, off
        n = off + rows * cols + T.PAD
        self.buf = torch.full((n,), fill, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 256 == 0      # what the layout of rms_norm_cases (and the CPU test of it) assumes
        self.view = self.buf[off: off + rows * cols].view(rows, cols)
        if data is not None:
            self.view.copy_(data.reshape(rows, cols).to(dtype))
        self.fill = fill

    @property
    def ptr(self):
        return self.view.data_ptr()

    def outside_untouched(self, what):
        flat = self.buf.float()
        n = self.rows * self.cols
        out = torch.cat([flat[: self.off], flat[self.off + n:]])
        assert bool((out == self.fill).all()), f"{what}: {int((out != self.fill).sum())} elements outside the tensor were written"

    def all_untouched(self, what):
        assert bool((self.buf.float() == self.fill).all()), f"{what}: a refused call wrote to its output"


def _check(got, ref, what, gate_dtype=None, rtol=None, atol_scale=None):
    """relative Frobenius gate + element tolerance, each figure printed before it is asserted"""
    gate_dtype = gate_dtype or got.dtype
    g = got.detach().double().cpu().numpy()
    ref = np.asarray(ref, dtype=np.float64).reshape(g.shape)
    r0, a0 = ELEM[gate_dtype]
    rtol, atol_scale = rtol or r0, atol_scale or a0
    m = record_parity(what, g, ref, str(got.dtype).replace("torch.", ""))
    print(f"{what}: rel_fro {m['rel_fro']:.3e} (gate {GATE[gate_dtype]:.1e})")
    assert np.isfinite(g).all(), f"{what}: non-finite output"
    assert m["rel_fro"] <= GATE[gate_dtype], f"{what}: relative Frobenius error {m['rel_fro']:.3e} (gate {GATE[gate_dtype]})"
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(g - ref)
    bad = err > rtol * np.abs(ref) + atol_scale * scale
    assert not bad.any(), f"{what}: {bad.sum()}/{bad.size} out of tolerance, max err {err.max():.3e}, scale {scale:.3e}"


def _rng(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()) & 0x7FFFFFFF)


def _randn(g, *shape, dtype, scale=1.0, shift=0.0):
    """values of `dtype` (so the fp64 reference sees exactly what the kernel reads), as a CPU tensor of that dtype"""
    return (scale * torch.randn(*shape, generator=g) + shift).to(dtype)


def rms64(x, w, eps):
    """the formulas of the op in fp64: y, rstd"""
    rstd = 1.0 / np.sqrt((x * x).mean(axis=1) + eps)
    return x * rstd[:, None] * w[None, :], rstd


def rms_bwd64(dy, x, w, eps):
    rstd = 1.0 / np.sqrt((x * x).mean(axis=1) + eps)
    xhat = x * rstd[:, None]
    wdy = w[None, :] * dy
    c1 = (xhat * wdy).mean(axis=1)
    return (wdy - xhat * c1[:, None]) * rstd[:, None], (dy * xhat).sum(axis=0)


def _expect_refusal(code, outs, what):
    assert code != 0, f"{what}: accepted"
    msg = _lib().lib().hstu_last_error().decode()
    assert "exceeds" in msg, f"{what}: {msg}"
    torch.cuda.synchronize()
    for b in outs:
        b.all_untouched(what)


def _params():
    return [pytest.param(c, getattr(torch, name), id=f"{T.case_id(c)}-{name}") for c in T.RMS_CASES for name in T.DTYPES[c["dt"]]]


@pytest.mark.parametrize("c,dtype", _params())
def test_rms_norm_classes(c, dtype):
    L = _lib()
    lib, code = L.lib(), L.torch_dtype_code(dtype)
    cid, rows, dim = T.case_id(c), c["rows"], c["dim"]
    g = _rng(cid)
    x = _randn(g, rows, dim, dtype=dtype, shift=0.3)
    w = _randn(g, dim, dtype=dtype, scale=0.1, shift=1.0)
    dy = _randn(g, rows, dim, dtype=dtype)
    off = lambda r: T.offset(c, r)
    X, W, Y = Buf(rows, dim, dtype, off("x"), data=x), Buf(1, dim, dtype, off("w"), data=w), Buf(rows, dim, dtype, off("y"))
    RSTD = Buf(1, rows, torch.float32)
    rc = lib.hstu_rms_norm_fwd(X.ptr, W.ptr, Y.ptr, None if c["null_rstd"] else RSTD.ptr, rows, dim, EPS, code, _stream())
    x64, w64, dy64 = x.double().numpy(), w.double().numpy(), dy.double().numpy()
    y64, rstd64 = rms64(x64, w64, EPS)
    if c["fwd"] == T.REF:
        _expect_refusal(rc, (Y, RSTD), f"{cid} fwd")
    else:
        L.check(rc)
        torch.cuda.synchronize()
        _check(Y.view, y64, f"{cid} y")
        Y.outside_untouched(f"{cid} y")
        if c["null_rstd"]:
            RSTD.all_untouched(f"{cid} rstd")
        else:
            _check(RSTD.view, rstd64, f"{cid} rstd")
            RSTD.outside_untouched(f"{cid} rstd")

    DY, DX = Buf(rows, dim, dtype, off("dy"), data=dy), Buf(rows, dim, dtype, off("dx"))
    DW = Buf(1, dim, torch.float32)
    RSTD_IN = Buf(1, rows, torch.float32, data=torch.from_numpy(rstd64))
    ws = torch.empty(max(lib.hstu_norm_bwd_workspace_bytes(rows, dim), 16), dtype=torch.uint8, device=DEV)
    rc = lib.hstu_rms_norm_bwd(DY.ptr, X.ptr, W.ptr, RSTD_IN.ptr, DX.ptr, DW.ptr, ws.data_ptr(), rows, dim, code, _stream())
    if c["bwd"] == T.REF:
        _expect_refusal(rc, (DX, DW), f"{cid} bwd")
        return
    L.check(rc)
    torch.cuda.synchronize()
    dx64, dw64 = rms_bwd64(dy64, x64, w64, EPS)
    _check(DX.view, dx64, f"{cid} dx")
    gd, rt, at = WGRAD_F32
    _check(DW.view, dw64, f"{cid} dweight", gd, rt, at)
    DX.outside_untouched(f"{cid} dx"), DW.outside_untouched(f"{cid} dweight")


def test_backward_of_no_rows_zero_fills_dweight():
    """rows == 0: dweight, prefilled with NaN, comes back as zeros (and nothing around it is written); the forward is a no-op"""
    L = _lib()
    lib, dim = L.lib(), 96
    DW = Buf(1, dim, torch.float32)
    DW.view.fill_(float("nan"))
    p = torch.zeros(64, dtype=torch.bfloat16, device=DEV).data_ptr()     # never dereferenced with rows == 0
    L.check(lib.hstu_rms_norm_bwd(p, p, p, p, p, DW.ptr, p, 0, dim, L.HSTU_DTYPE_BF16, _stream()))
    Y = Buf(1, dim, torch.bfloat16)
    L.check(lib.hstu_rms_norm_fwd(p, p, Y.ptr, None, 0, dim, EPS, L.HSTU_DTYPE_BF16, _stream()))
    torch.cuda.synchronize()
    assert bool((DW.view == 0).all())
    DW.outside_untouched("dweight"), Y.all_untouched("y")


@pytest.mark.parametrize("dtype,rows,dim", [(torch.bfloat16, 8195, 512), (torch.float32, 1031, 1028), (torch.float16, 777, 37)],
                         ids=["bf16-vec-one", "fp32-wide", "fp16-scalar"])
def test_two_backward_calls_give_identical_bits(dtype, rows, dim):
    """no locks, no atomics: the partial rows are summed in a fixed order"""
    from generative_recommenders_amd.ops import _launch

    g = _rng(f"det-{rows}-{dim}")
    x, dy = _randn(g, rows, dim, dtype=dtype).to(DEV), _randn(g, rows, dim, dtype=dtype).to(DEV)
    w = _randn(g, dim, dtype=dtype, scale=0.1, shift=1.0).to(DEV)
    _, rstd = _launch.rms_norm_fwd(x, w, EPS)
    dx1, dw1 = _launch.rms_norm_bwd(dy, x, w, rstd)
    junk = torch.full((1 << 22,), 3.0, device=DEV)            # the second call's workspace starts from other contents
    dx2, dw2 = _launch.rms_norm_bwd(dy, x, w, rstd)
    del junk
    assert torch.equal(dx1, dx2) and torch.equal(dw1, dw2)
    assert dw1.dtype == torch.float32 and bool(torch.isfinite(dw1).all())


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "rms_norm", "rms_norm.npz"), allow_pickle=False)
    cases = [{k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(f"c{i}:")} for i in range(int(z["n_cases"]))]
    assert [c["x"].shape for c in cases] == [(7, 37), (33, 520)]
    return cases


@pytest.mark.parametrize("through", ["function", "module"])
def test_fp32_matches_the_reference_fixture(golden, through):
    """tests/golden/rms_norm/rms_norm.npz: the unmodified reference's RMSNorm (PyTorch branch, fp32, CPU), y and dx, dw of sum(y * g)"""
    from generative_recommenders_amd.ops.layer_norm import RMSNorm, rms_norm

    for i, c in enumerate(golden):
        x = torch.from_numpy(c["x"]).to(DEV).requires_grad_()
        g = torch.from_numpy(c["g"]).to(DEV)
        eps = float(c["eps"])
        if through == "module":
            m = RMSNorm(x.shape[1], eps=eps).to(DEV)
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(c["w"]))
            w, y = m.weight, m(x)
        else:
            w = torch.from_numpy(c["w"]).to(DEV).requires_grad_()
            y = rms_norm(x, w, eps)
        assert y.dtype == torch.float32 and y.shape == x.shape
        (y * g).sum().backward()
        _check(y, c["y"], f"golden {i} {through} y")
        _check(x.grad, c["dx"], f"golden {i} {through} dx")
        gd, rt, at = WGRAD_F32
        _check(w.grad, c["dw"], f"golden {i} {through} dweight", gd, rt, at)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_module_autograd_16bit(dtype):
    """(5, 3, 64) input: leading dims flattened and restored; dweight in the parameter's dtype"""
    from generative_recommenders_amd.ops.layer_norm import RMSNorm

    g = _rng(f"autograd-{dtype}")
    x = _randn(g, 5, 3, 64, dtype=dtype, shift=0.3)
    w = _randn(g, 64, dtype=dtype, scale=0.1, shift=1.0)
    dy = _randn(g, 5, 3, 64, dtype=dtype)
    m = RMSNorm(64).to(DEV).to(dtype)
    with torch.no_grad():
        m.weight.copy_(w)
    xd = x.to(DEV).requires_grad_()
    y = m(xd)
    assert y.shape == (5, 3, 64) and y.dtype == dtype
    y.backward(dy.to(DEV))
    assert m.weight.grad.dtype == dtype and xd.grad.shape == x.shape and xd.grad.dtype == dtype
    x64, w64, dy64 = x.double().numpy().reshape(15, 64), w.double().numpy(), dy.double().numpy().reshape(15, 64)
    y64, _ = rms64(x64, w64, m._eps)
    dx64, dw64 = rms_bwd64(dy64, x64, w64, m._eps)
    _check(y.reshape(15, 64), y64, f"module {dtype} y")
    _check(xd.grad.reshape(15, 64), dx64, f"module {dtype} dx")
    _, rt, at = WGRAD_16
    _check(m.weight.grad, dw64, f"module {dtype} dweight", dtype, rt, at)
    # an fp32 master weight next to 16-bit activations: the gradient comes back in fp32
    m32 = RMSNorm(64).to(DEV)
    m32(x.to(DEV)).backward(dy.to(DEV))
    assert m32.weight.grad.dtype == torch.float32


def test_cpu_tensor_raises():
    from generative_recommenders_amd.ops.layer_norm import RMSNorm, rms_norm

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rms_norm(torch.zeros(4, 8), torch.ones(8, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RMSNorm(8)(torch.zeros(4, 8))
