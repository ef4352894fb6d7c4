"""Every dispatch class of the row-norm kernels (csrc/norm_ops.hip, norm_kernels.inc) against fp64.

The rows of tests/norm_class_cases.py -- each labelled with the instantiation it reaches, which
tests/test_norm_dispatch_host.py verifies on the CPU -- run here through the C ABI with raw pointers: every tensor of a
call sits alone inside a sentinel-filled allocation, one element off 16-byte alignment when the row says so, so that
  * the results are compared with the fp64 oracle (never with another kernel),
  * everything outside the tensor (in front, behind, in the gaps of a row stride) must still hold the sentinel, and
  * a refused call must have written nothing.

Tolerances are the project's: the relative-Frobenius gates and element tolerances of test_compute_gpu._close
(profiles/r02_parity_errors.md), the weight-gradient tolerances of test_layer_norm_sweep / test_norm_mul_wide_rows, the L2
norm bands of test_postprocess_gpu.test_l2_norm_vs_oracle, SiLU fp32 rtol 1e-5 / atol 1e-6.  16-bit SiLU has no project
number: gated at twice the largest error measured on MI355X in units of the output type's ulp (SILU_ULP below,
profiles/silu_16bit_ulp.md)."""

import zlib

import numpy as np
import pytest
import torch

import norm_class_cases as T
from conftest import record_parity
from oracle import hstu_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77.0          # exactly representable in bf16 / fp16 / fp32; no kernel output of these inputs comes near it
EPS = 1e-5
SEED = 0x1234567887654321

# relative Frobenius gate by dtype (test_compute_gpu._close) and element tolerance (rtol, atol as a fraction of max|ref|)
GATE = {torch.float32: 1.5e-6, torch.bfloat16: 2.8e-3, torch.float16: 3.2e-4}
ELEM = {torch.float32: (1e-3, 2e-5), torch.bfloat16: (2e-2, 4e-3), torch.float16: (2e-2, 4e-3)}
# weight gradients (fp32 outputs): from exact inputs in fp32 math they are held to the fp32 bar of test_norm_mul_wide_rows;
# where the kernel rounds SiLU(u) to a 16-bit type on the way (u_is_preactivation) to the 16-bit bar of test_layer_norm_sweep
WGRAD_F32 = (torch.float32, 1e-3, 1e-4)
WGRAD_16 = (None, 3e-2, 1e-2)
# 16-bit SiLU: largest |got - fp64| measured on MI355X in ulps of the output type at the fp64 value (profiles/silu_16bit_ulp.md);
# the gate is twice that -- the hardware exp2 / rcp path is not bit-reproducible across compiler versions
# measured: bf16 0.500018 (forward and backward, vector and scalar kernel), fp16 0.500 forward / 0.52595 backward
SILU_ULP_MEASURED = {torch.bfloat16: 0.50002, torch.float16: 0.526}
MANT = {torch.bfloat16: 7, torch.float16: 10}
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}


def _lib():
    from generative_recommenders_amd import _lib as L

    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """a (rows, cols) tensor, rows `stride` elements apart, `off` elements into its own sentinel-filled allocation"""

    def __init__(self, rows, cols, dtype, off=T.PAD, stride=None, data=None, fill=SENT):
        self.rows, self.cols, self.stride, self.off = rows, cols, stride or cols, off
        n = off + max(rows - 1, 0) * self.stride + cols + T.PAD
        self.buf = torch.full((n,), fill, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 256 == 0      # what the layout of norm_class_cases (and the CPU test of it) assumes
        self.view = self.buf[off:].as_strided((rows, cols), (self.stride, 1))
        if data is not None:
            self.view.copy_(data.reshape(rows, cols).to(dtype))
        self.fill = fill

    @property
    def ptr(self):
        return self.view.data_ptr()

    def outside_untouched(self, what):
        flat = self.buf.float().cpu().numpy()
        inside = np.zeros(flat.size, dtype=bool)
        for r in range(self.rows):
            inside[self.off + r * self.stride: self.off + r * self.stride + self.cols] = True
        assert (flat[~inside] == self.fill).all(), f"{what}: {(flat[~inside] != self.fill).sum()} elements outside the tensor were written"

    def all_untouched(self, what):
        assert bool((self.buf.float() == self.fill).all()), f"{what}: a refused call wrote to its output"

    def f64(self):
        return self.view.detach().double().cpu().numpy()


def _check(got, ref, what, gate_dtype=None, rtol=None, atol_scale=None):
    """test_compute_gpu._close with the gate's dtype explicit: relative Frobenius gate + element tolerance"""
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


def _expect_refusal(code, outs, what):
    L = _lib()
    assert code != 0, f"{what}: accepted"
    msg = L.lib().hstu_last_error().decode()
    assert "exceeds" in msg, f"{what}: {msg}"
    torch.cuda.synchronize()
    for b in outs:
        b.all_untouched(what)


def _params():
    out = []
    for c in T.CASES:
        for name in T.DTYPES[c["dt"]]:
            out.append(pytest.param(c, getattr(torch, name), id=f"{T.case_id(c)}-{name}"))
    return out


def _cases(op):
    return [p for p in _params() if p.values[0]["op"] == op]


# ------------------------------------------------------------------------------------------------ layer norm, swish layer norm
def _ln_stats(x64):
    mean = x64.mean(axis=1)
    rstd = 1.0 / np.sqrt(((x64 - mean[:, None]) ** 2).mean(axis=1) + EPS)
    return mean, rstd


@pytest.mark.parametrize("c,dtype", _cases("ln") + _cases("swish"))
def test_layer_norm_classes(c, dtype):
    L = _lib()
    lib, code = L.lib(), L.torch_dtype_code(dtype)
    cid, rows, dim, swish = T.case_id(c), c["rows"], c["dim"], c["op"] == "swish"
    g = _rng(cid)
    x = _randn(g, rows, dim, dtype=dtype, shift=0.3)
    w = _randn(g, dim, dtype=dtype, scale=0.1, shift=1.0)
    b = _randn(g, dim, dtype=dtype, scale=0.1)
    dy = _randn(g, rows, dim, dtype=dtype)
    dres = _randn(g, rows, dim, dtype=dtype) if c["res"] else None
    off = lambda r: T.offset(c, r)
    X, W, B = Buf(rows, dim, dtype, off("x"), data=x), Buf(1, dim, dtype, off("w"), data=w), Buf(1, dim, dtype, off("b"), data=b)
    Y = Buf(rows, dim, dtype, off("y"))
    MEAN, RSTD = Buf(1, rows, torch.float32), Buf(1, rows, torch.float32)
    fwd = lib.hstu_swish_layer_norm_fwd if swish else lib.hstu_layer_norm_fwd
    stats = (None, None) if c["null_stats"] else (MEAN.ptr, RSTD.ptr)
    rc = fwd(X.ptr, W.ptr, B.ptr, Y.ptr, *stats, rows, dim, EPS, code, _stream())
    x64, w64, b64 = x.double().numpy(), w.double().numpy(), b.double().numpy()
    mean64, rstd64 = _ln_stats(x64)
    if c["fwd"] == T.REF:
        _expect_refusal(rc, (Y, MEAN, RSTD), f"{cid} fwd")
    else:
        L.check(rc)
        torch.cuda.synchronize()
        ref = (O.swish_layer_norm_fwd if swish else O.layer_norm_fwd)(x64, w64, b64, EPS)
        _check(Y.view, ref, f"{cid} y")
        Y.outside_untouched(f"{cid} y")
        if c["null_stats"]:
            MEAN.all_untouched(f"{cid} mean"), RSTD.all_untouched(f"{cid} rstd")
        else:
            _check(MEAN.view, mean64, f"{cid} mean"), _check(RSTD.view, rstd64, f"{cid} rstd")
            MEAN.outside_untouched(f"{cid} mean"), RSTD.outside_untouched(f"{cid} rstd")

    DY, DX = Buf(rows, dim, dtype, off("dy"), data=dy), Buf(rows, dim, dtype, off("dx"))
    DRES = Buf(rows, dim, dtype, off("dres"), data=dres) if c["res"] else None
    DW, DB = Buf(1, dim, torch.float32), Buf(1, dim, torch.float32)
    MEAN_IN = Buf(1, rows, torch.float32, data=torch.from_numpy(mean64))
    RSTD_IN = Buf(1, rows, torch.float32, data=torch.from_numpy(rstd64))
    ws = torch.empty(max(lib.hstu_norm_bwd_workspace_bytes(rows, dim), 16), dtype=torch.uint8, device=DEV)
    if swish:
        rc = lib.hstu_swish_layer_norm_bwd(DY.ptr, X.ptr, W.ptr, B.ptr, MEAN_IN.ptr, RSTD_IN.ptr, DX.ptr, DW.ptr, DB.ptr, ws.data_ptr(),
                                           rows, dim, code, _stream())
    elif c["res"]:
        rc = lib.hstu_layer_norm_bwd_residual(DY.ptr, X.ptr, W.ptr, MEAN_IN.ptr, RSTD_IN.ptr, DRES.ptr, DX.ptr, DW.ptr, DB.ptr,
                                              ws.data_ptr(), rows, dim, code, _stream())
    else:
        rc = lib.hstu_layer_norm_bwd(DY.ptr, X.ptr, W.ptr, MEAN_IN.ptr, RSTD_IN.ptr, DX.ptr, DW.ptr, DB.ptr, ws.data_ptr(), rows, dim,
                                     code, _stream())
    if c["bwd"] == T.REF:
        _expect_refusal(rc, (DX, DW, DB), f"{cid} bwd")
        return
    L.check(rc)
    torch.cuda.synchronize()
    dy64 = dy.double().numpy()
    if swish:
        dx64, dw64, db64 = O.swish_layer_norm_bwd(dy64, x64, w64, b64, EPS)
    else:
        dx64, dw64, db64 = O.layer_norm_bwd(dy64, x64, w64, EPS)
    if c["res"]:
        dx64 = dx64 + dres.double().numpy()
    _check(DX.view, dx64, f"{cid} dx")
    gd, rt, at = WGRAD_F32
    _check(DW.view, dw64, f"{cid} dweight", gd, rt, at), _check(DB.view, db64, f"{cid} dbias", gd, rt, at)
    for bf, nm_ in ((DX, "dx"), (DW, "dweight"), (DB, "dbias")):
        bf.outside_untouched(f"{cid} {nm_}")


# ------------------------------------------------------------------------------------------------ u * Norm(attn)
def _silu64(x):
    return x / (1.0 + np.exp(-x))


def _nm_reference_bwd(c, dtype, attn, u_in, w, b, dy, keep, scale):
    """fp64 torch autograd on the CPU of the same formula (as test_norm_mul_wide_rows): returns dattn, du, dweight, dbias.
    u_is_preactivation: the two rounding points of the documented contract of hstu_norm_mul_silu_* are restated -- SiLU(u)
    enters rounded to `dtype` where hstu_silu_fwd would have stored it, and d u is rounded to `dtype` before it is
    multiplied by SiLU' -- everything else is fp64."""
    rows, dim, heads, hd = c["rows"], c["dim"], c["heads"], c["hd"]
    a64 = attn.double().requires_grad_()
    w64, b64 = w.double().requires_grad_(), b.double().requires_grad_()
    pre = u_in.double()
    uu = (torch.nn.functional.silu(pre).to(dtype).double() if c["silu"] else pre).requires_grad_()
    if c["gn"]:
        xh = a64.view(rows, heads, hd)
        n = (xh - xh.mean(-1, keepdim=True)) / torch.sqrt(xh.var(-1, unbiased=False, keepdim=True) + EPS)
        n = (n * w64.view(1, heads, 1) + b64.view(1, heads, 1)).reshape(rows, dim)
    else:
        n = torch.nn.functional.layer_norm(a64, (dim,), w64, b64, EPS)
    y = uu * n
    if c["concat"]:
        y = torch.cat([uu, a64, y], dim=1)
    if keep is not None:
        y = y * torch.from_numpy(keep.astype(np.float64) * scale)
    y.backward(dy.double())
    du = uu.grad
    if c["silu"]:
        sg = torch.sigmoid(pre)
        du = du.to(dtype).double() * sg * (1.0 + pre * (1.0 - sg))
    return a64.grad.numpy(), du.numpy(), w64.grad.numpy(), b64.grad.numpy()


@pytest.mark.parametrize("c,dtype", _cases("nm"))
def test_norm_mul_classes(c, dtype):
    L = _lib()
    lib, code = L.lib(), L.torch_dtype_code(dtype)
    cid, rows, dim, heads, hd, gn = T.case_id(c), c["rows"], c["dim"], c["heads"], c["hd"], c["gn"]
    ostride = 3 * dim if c["concat"] else dim
    width, ngroups = (heads, heads) if gn else (dim, 1)
    g = _rng(cid)
    attn = _randn(g, rows, dim, dtype=dtype, shift=0.3)
    u = _randn(g, rows, dim, dtype=dtype)
    w = _randn(g, width, dtype=dtype, scale=0.1, shift=1.0)
    b = _randn(g, width, dtype=dtype, scale=0.1)
    dy = _randn(g, rows, ostride, dtype=dtype)
    off = lambda r: T.offset(c, r)
    A, U = Buf(rows, dim, dtype, off("attn"), data=attn), Buf(rows, dim, dtype, off("u"), stride=c["ustride"], data=u)
    W, B = Buf(1, width, dtype, off("w"), data=w), Buf(1, width, dtype, off("b"), data=b)
    Y = Buf(rows, ostride, dtype, off("y"))
    MEAN, RSTD = Buf(1, rows * ngroups, torch.float32), Buf(1, rows * ngroups, torch.float32)
    rc = lib.hstu_norm_mul_silu_fwd(A.ptr, U.ptr, c["ustride"], int(c["silu"]), W.ptr, B.ptr, Y.ptr, MEAN.ptr, RSTD.ptr, rows, heads, hd,
                                    EPS, int(gn), int(c["concat"]), c["drop"], SEED, code, _stream())
    if c["fwd"] == T.REF:
        _expect_refusal(rc, (Y, MEAN, RSTD), f"{cid} fwd")
    else:
        L.check(rc)
        torch.cuda.synchronize()
    a64, w64, b64 = attn.double().numpy(), w.double().numpy(), b.double().numpy()
    u64 = u.double().numpy()
    if c["silu"]:
        u64 = torch.from_numpy(_silu64(u64)).to(dtype).double().numpy()      # rounded where hstu_silu_fwd would have stored it
    keep, scale = O.dropout_keep_mask(SEED, rows, ostride, c["drop"]) if c["drop"] else (None, 1.0)
    grp = a64.reshape(rows * ngroups, -1)
    mean64, rstd64 = _ln_stats(grp)
    if c["fwd"] != T.REF:
        ref = O.norm_mul(a64, u64, w64, b64, EPS, c["concat"], gn, heads, hd)
        if keep is not None:
            ref = ref * keep * scale
            got0 = Y.f64() == 0
            ref0 = torch.from_numpy(ref).to(dtype).double().numpy() == 0
            assert np.array_equal(got0, ~keep | ref0), f"{cid}: the zeros of y are not the oracle's dropout mask"
        _check(Y.view, ref, f"{cid} y")
        _check(MEAN.view, mean64, f"{cid} mean"), _check(RSTD.view, rstd64, f"{cid} rstd")
        for bf, nm_ in ((Y, "y"), (MEAN, "mean"), (RSTD, "rstd")):
            bf.outside_untouched(f"{cid} {nm_}")

    DY, DA = Buf(rows, ostride, dtype, off("dy"), data=dy), Buf(rows, dim, dtype, off("dattn"))
    DU = Buf(rows, dim, dtype, off("du"), stride=c["dustride"])
    DW, DB = Buf(1, width, torch.float32), Buf(1, width, torch.float32)
    MEAN_IN = Buf(1, rows * ngroups, torch.float32, data=torch.from_numpy(mean64))
    RSTD_IN = Buf(1, rows * ngroups, torch.float32, data=torch.from_numpy(rstd64))
    ws = torch.empty(max(lib.hstu_norm_bwd_workspace_bytes(rows, dim), 16), dtype=torch.uint8, device=DEV)
    rc = lib.hstu_norm_mul_silu_bwd(DY.ptr, A.ptr, U.ptr, c["ustride"], int(c["silu"]), W.ptr, B.ptr, MEAN_IN.ptr, RSTD_IN.ptr, DA.ptr,
                                    DU.ptr, c["dustride"], DW.ptr, DB.ptr, ws.data_ptr(), rows, heads, hd, int(gn), int(c["concat"]),
                                    c["drop"], SEED, code, _stream())
    if c["bwd"] == T.REF:
        _expect_refusal(rc, (DA, DU, DW, DB), f"{cid} bwd")
        return
    L.check(rc)
    torch.cuda.synchronize()
    dattn64, du64, dw64, db64 = _nm_reference_bwd(c, dtype, attn, u, w, b, dy, keep, scale)
    _check(DA.view, dattn64, f"{cid} dattn"), _check(DU.view, du64, f"{cid} du")
    gd, rt, at = (dtype, *WGRAD_16[1:]) if (c["silu"] and dtype != torch.float32) else WGRAD_F32
    _check(DW.view, dw64, f"{cid} dweight", gd, rt, at), _check(DB.view, db64, f"{cid} dbias", gd, rt, at)
    for bf, nm_ in ((DA, "dattn"), (DU, "du"), (DW, "dweight"), (DB, "dbias")):
        bf.outside_untouched(f"{cid} {nm_}")


def test_group_norm_refuses_more_than_16_heads():
    L = _lib()
    lib = L.lib()
    heads, hd, rows, dtype = T.GN_TOO_MANY_HEADS["heads"], T.GN_TOO_MANY_HEADS["hd"], 5, torch.bfloat16
    dim = heads * hd
    A, U, W, B = (Buf(rows, dim, dtype, data=torch.randn(rows, dim)), Buf(rows, dim, dtype, data=torch.randn(rows, dim)),
                  Buf(1, heads, dtype, data=torch.ones(heads)), Buf(1, heads, dtype, data=torch.zeros(heads)))
    Y, MEAN, RSTD = Buf(rows, dim, dtype), Buf(1, rows * heads, torch.float32), Buf(1, rows * heads, torch.float32)
    rc = lib.hstu_norm_mul_fwd(A.ptr, U.ptr, W.ptr, B.ptr, Y.ptr, MEAN.ptr, RSTD.ptr, rows, heads, hd, EPS, 1, 0, L.HSTU_DTYPE_BF16, _stream())
    assert rc != 0 and "at most 16 heads" in lib.hstu_last_error().decode()
    DA, DU, DW, DB = Buf(rows, dim, dtype), Buf(rows, dim, dtype), Buf(1, heads, torch.float32), Buf(1, heads, torch.float32)
    ws = torch.empty(lib.hstu_norm_bwd_workspace_bytes(rows, dim), dtype=torch.uint8, device=DEV)
    rc = lib.hstu_norm_mul_bwd(Y.ptr, A.ptr, U.ptr, W.ptr, B.ptr, MEAN.ptr, RSTD.ptr, DA.ptr, DU.ptr, DW.ptr, DB.ptr, ws.data_ptr(), rows,
                               heads, hd, 1, 0, L.HSTU_DTYPE_BF16, _stream())
    assert rc != 0 and "at most 16 heads" in lib.hstu_last_error().decode()
    torch.cuda.synchronize()
    for bf in (Y, MEAN, RSTD, DA, DU, DW, DB):
        bf.all_untouched("17 heads")


@pytest.mark.parametrize("op", ["ln", "ln_res", "swish", "nm_ln", "nm_gn"])
def test_backward_of_no_rows_zero_fills_the_weight_gradients(op):
    """rows == 0: dweight / dbias, prefilled with NaN, come back as zeros (and nothing around them is written)"""
    L = _lib()
    lib = L.lib()
    heads, hd = 4, 24
    dim = heads * hd
    width = heads if op == "nm_gn" else dim
    nan = float("nan")
    DW, DB = Buf(1, width, torch.float32, fill=SENT), Buf(1, width, torch.float32, fill=SENT)
    DW.view.fill_(nan), DB.view.fill_(nan)
    p = torch.zeros(64, dtype=torch.bfloat16, device=DEV).data_ptr()     # never dereferenced with rows == 0
    code = L.HSTU_DTYPE_BF16
    if op == "ln":
        rc = lib.hstu_layer_norm_bwd(p, p, p, p, p, p, DW.ptr, DB.ptr, p, 0, dim, code, _stream())
    elif op == "ln_res":
        rc = lib.hstu_layer_norm_bwd_residual(p, p, p, p, p, p, p, DW.ptr, DB.ptr, p, 0, dim, code, _stream())
    elif op == "swish":
        rc = lib.hstu_swish_layer_norm_bwd(p, p, p, p, p, p, p, DW.ptr, DB.ptr, p, 0, dim, code, _stream())
    else:
        rc = lib.hstu_norm_mul_bwd(p, p, p, p, p, p, p, p, p, DW.ptr, DB.ptr, p, 0, heads, hd, int(op == "nm_gn"), 1, code, _stream())
    L.check(rc)
    torch.cuda.synchronize()
    for bf in (DW, DB):
        assert bool((bf.view == 0).all()), f"{op}: not zero-filled"
        bf.outside_untouched(op)


# ------------------------------------------------------------------------------------------------ row L2 norm
@pytest.mark.parametrize("c,dtype", _cases("l2"))
def test_l2_norm_classes(c, dtype):
    L = _lib()
    lib, code = L.lib(), L.torch_dtype_code(dtype)
    cid, rows, dim = T.case_id(c), c["rows"], c["dim"]
    eps = 1e-6
    g = _rng(cid)
    x = _randn(g, rows, dim, dtype=dtype)
    clamp_row = 1 if rows > 2 else None
    if clamp_row is not None:
        x[clamp_row] = 0          # the clamped row: y = 0, dx = g / eps
    gy = _randn(g, rows, dim, dtype=dtype)
    off = lambda r: T.offset(c, r)
    X, Y = Buf(rows, dim, dtype, off("x"), data=x), Buf(rows, dim, dtype, off("y"))
    rc = lib.hstu_l2_norm_fwd(X.ptr, Y.ptr, rows, dim, eps, code, _stream())
    x64, g64 = x.double().numpy(), gy.double().numpy()
    if c["fwd"] == T.REF:
        _expect_refusal(rc, (Y,), f"{cid} fwd")
    else:
        L.check(rc)
        torch.cuda.synchronize()
        ref = O.l2_norm_fwd(x64, eps)
        if dtype == torch.float32:
            np.testing.assert_allclose(Y.f64(), ref, rtol=1e-5, atol=1e-6)
        else:
            np.testing.assert_allclose(Y.f64(), ref, rtol=1.6e-2, atol=1e-3)
        record_parity(f"{cid} y", Y.f64(), ref, str(dtype).replace("torch.", ""))
        Y.outside_untouched(f"{cid} y")
    DY, DX = Buf(rows, dim, dtype, off("dy"), data=gy), Buf(rows, dim, dtype, off("dx"))
    rc = lib.hstu_l2_norm_bwd(DY.ptr, X.ptr, DX.ptr, rows, dim, eps, code, _stream())
    if c["bwd"] == T.REF:
        _expect_refusal(rc, (DX,), f"{cid} bwd")
        return
    L.check(rc)
    torch.cuda.synchronize()
    rdx = O.l2_norm_bwd(g64, x64, eps)
    got = DX.f64()
    ok = np.ones(rows, dtype=bool)
    if dtype == torch.float32:
        np.testing.assert_allclose(got, rdx, rtol=1e-4, atol=1e-5)
    else:
        if clamp_row is not None:
            ok[clamp_row] = False     # g / eps = 1e6 g is far outside any 16-bit absolute band: checked on its own below
        np.testing.assert_allclose(got[ok], rdx[ok], rtol=3e-2, atol=3e-3)
        if clamp_row is not None:
            # the clamped row against g / eps formed in fp32 and rounded once to the output type (fp16: overflows to inf alike)
            want = (gy[clamp_row].float() * torch.tensor(1.0, dtype=torch.float32).div(torch.tensor(eps, dtype=torch.float32))).to(dtype)
            np.testing.assert_allclose(got[clamp_row], want.double().numpy(), rtol=2.0 ** -MANT[dtype], atol=0)
    record_parity(f"{cid} dx", got[ok], rdx[ok], str(dtype).replace("torch.", ""))
    DX.outside_untouched(f"{cid} dx")


# ------------------------------------------------------------------------------------------------ SiLU on a column slice
def _ulp_error(got, ref, dtype):
    """|got - ref| in units of the spacing of `dtype` at |ref| (subnormals: the smallest spacing)"""
    e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** MIN_EXP[dtype])))
    return np.abs(got - ref) / 2.0 ** (e - MANT[dtype])


def _silu_check(got, ref, dtype, what):
    if dtype == torch.float32:
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)      # the bar of test_silu_matches_torch, now against fp64
        return
    worst = float(_ulp_error(got, ref, dtype).max())
    print(f"{what}: largest error {worst:.4f} ulp of {dtype}")
    record_parity(what, got, ref, str(dtype).replace("torch.", ""), max_ulp=worst)
    assert worst <= 2 * SILU_ULP_MEASURED[dtype], f"{what}: {worst:.4f} ulp (gate {2 * SILU_ULP_MEASURED[dtype]})"


@pytest.mark.parametrize("c,dtype", _cases("silu"))
def test_silu_classes(c, dtype):
    L = _lib()
    lib, code = L.lib(), L.torch_dtype_code(dtype)
    cid, rows, cols = T.case_id(c), c["rows"], c["dim"]
    g = _rng(cid)
    x = _randn(g, rows, cols, dtype=dtype, scale=3.0)
    gy = _randn(g, rows, cols, dtype=dtype)
    off = lambda r: T.offset(c, r)
    X = Buf(rows, cols, dtype, off("in"), stride=c["ustride"], data=x)
    OUT = Buf(rows, cols, dtype, off("out"), stride=c["dustride"])
    L.check(lib.hstu_silu_fwd(X.ptr, OUT.ptr, rows, cols, c["ustride"], c["dustride"], code, _stream()))
    torch.cuda.synchronize()
    x64, g64 = x.double().numpy(), gy.double().numpy()
    s = 1.0 / (1.0 + np.exp(-x64))
    _silu_check(OUT.f64(), x64 * s, dtype, f"{cid} silu fwd [{c['fwd']}]")
    OUT.outside_untouched(f"{cid} out")
    DOUT = Buf(rows, cols, dtype, off("dout"), data=gy)
    DIN = Buf(rows, cols, dtype, off("din"), stride=c["dustride"])
    L.check(lib.hstu_silu_bwd(DOUT.ptr, X.ptr, DIN.ptr, rows, cols, cols, c["ustride"], c["dustride"], code, _stream()))
    torch.cuda.synchronize()
    _silu_check(DIN.f64(), g64 * s * (1.0 + x64 * (1.0 - s)), dtype, f"{cid} silu bwd [{c['bwd']}]")
    DIN.outside_untouched(f"{cid} din")
