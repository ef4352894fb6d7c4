"""GPU tests of the row-wise e4m3 UVQK projection (csrc/hstu_ln_linear_fp8.cuh; C entries hstu_quantize_rows_fp8,
hstu_ln_linear_fp8_fwd, hstu_linear_fp8_rowwise) against the restatement of its arithmetic in tests/fp8_linear_ref.py.

Tolerances.  The quantizer and the operand mapping are exact (torch.equal).  For the fused kernel: mean / rstd / x_scale
2e-6 relative (the project's tolerance for fp32 row statistics); codes: an fp32 LayerNorm against the fp64 one of the
restatement moves a value across a rounding boundary in ~1e-6 of the elements (measured on the CPU: 8.8e-7 at 20,000 x 512,
each by one step), so differing codes must be NEIGHBOURS and at most 1e-4 of all; the product against the fp64 product of the
kernel's OWN codes and scales leaves the fp32 accumulation and the output rounding: the gates of this kernel family,
2.8e-3 bf16 / 3.2e-4 fp16 relative Frobenius; end to end against the unquantized fp64 product: e_q + gate, e_q being the
restatement's own error against that product (triangle inequality)."""

import pytest
import torch

import fp8_linear_ref as R
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
GATE = {torch.bfloat16: 2.8e-3, torch.float16: 3.2e-4}
EPS = 1e-6


def _launch():
    from generative_recommenders_amd.ops import _launch as L

    return L


def _inputs(rows, n, dtype, seed, mean_shift=0.0, k=512):
    """tests/test_ln_linear_gpu.py's generator, the weight already K-contiguous (n, k)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, k, generator=g) * (0.5 + torch.rand(rows, 1, generator=g)) + mean_shift * torch.randn(rows, 1, generator=g)).to(dtype)
    lw = (1 + 0.1 * torch.randn(k, generator=g)).to(dtype)
    lb = (0.1 * torch.randn(k, generator=g)).to(dtype)
    w_nk = (torch.randn(k, n, generator=g) / k**0.5).to(dtype).t().contiguous()
    b = (0.1 * torch.randn(n, generator=g)).to(dtype)
    return x, lw, lb, w_nk, b


# ---------------------------------------------------------------------------------------------------------- quantizer
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows", [1, 33, 2049])
@pytest.mark.parametrize("k", [16, 512, 4096])
def test_quantize_rows_bit_exact(dtype, rows, k):
    g = torch.Generator().manual_seed(rows * 7 + k)
    src = (torch.randn(rows, k, generator=g) * (0.05 + 20 * torch.rand(rows, 1, generator=g))).to(dtype)
    src[rows // 2, :-1] *= 0.01            # amax in the last column
    src[rows // 2, -1] = -7.0
    if rows > 1:
        src[rows - 1] = 0                  # a zero row: scale 1, codes 0
    q, scale = _launch().quantize_rows_fp8(src.to(DEV))
    rq, rscale = R.quantize_rows(src)
    assert q.dtype == FP8 and q.shape == (rows, k) and scale.dtype == torch.float32
    assert torch.equal(scale.cpu(), rscale)
    assert torch.equal(q.cpu().view(torch.uint8), rq.view(torch.uint8))
    if rows > 1:
        assert scale[rows - 1].item() == 1.0 and int(q[rows - 1].view(torch.uint8).max()) == 0
    assert scale[rows // 2].item() == 7.0 / 448.0


def test_quantize_rows_strided_source():
    """rows of a wider tensor (leading dimension > k)"""
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(70, 1024, generator=g).bfloat16()
    q, scale = _launch().quantize_rows_fp8(wide.to(DEV)[:, 256:768])
    rq, rscale = R.quantize_rows(wide[:, 256:768])
    assert torch.equal(scale.cpu(), rscale) and torch.equal(q.cpu().view(torch.uint8), rq.view(torch.uint8))


# ---------------------------------------------------------------------------------------------------- operand mapping
def _e4m3_table(rows, cols):
    """an asymmetric table of e4m3 values (mantissa 1 + j/8, exponents -2 .. 3, both signs): no two neighbours alike"""
    r = torch.arange(rows)[:, None]
    c = torch.arange(cols)[None, :]
    i = (r * 31 + c * 7 + (r * c) % 5) % 96
    v = (1 + (i % 8).double() / 8) * 2.0 ** ((i // 8) % 6 - 2).double()
    return torch.where(i >= 48, -v, v).float().to(FP8)


def _one_hot(rows, k=512):
    q = torch.zeros(rows, k)
    q[torch.arange(rows), (7 * torch.arange(rows) + 3) % k] = 1.0
    return q.to(FP8)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows", [1, 31, 257])
@pytest.mark.parametrize("n", [32, 96])
@pytest.mark.parametrize("one_hot_x", [True, False])
def test_operand_mapping_exact(dtype, rows, n, one_hot_x):
    """one operand one-hot, the other a table of e4m3 values, scales powers of two (different per row AND per column), no bias:
    every output is one e4m3 value times a power of two -- exact in bf16 and fp16.  A wrong k assignment, rows and columns
    swapped in the store or a scale on the wrong axis changes it."""
    xq = _one_hot(rows) if one_hot_x else _e4m3_table(rows, 512)
    wq = _e4m3_table(n, 512) if one_hot_x else _one_hot(n)
    xs = 2.0 ** ((torch.arange(rows) % 5) - 2).float()
    ws = 2.0 ** ((torch.arange(n) % 3) - 1).float()
    y = _launch().linear_fp8_rowwise(xq.to(DEV), xs.to(DEV), wq.to(DEV), ws.to(DEV), None, out_dtype=dtype)
    want = R.product(xq, xs, wq, ws)
    assert torch.equal(want.to(dtype).double(), want)             # the expectation itself is exact in the I/O type
    assert (want != 0).any(dim=1).all() and (want != 0).any(dim=0).all()
    assert y.dtype == dtype and torch.equal(y.cpu().double(), want)


# -------------------------------------------------------------------------------------------------------- fused kernel
def _check_fused(x, lw, lb, w_nk, b, dtype, tag):
    L = _launch()
    wq, ws = R.quantize_rows(w_nk)
    y, xq, xs, mean, rstd = L.ln_linear_fp8_fwd(x.to(DEV), lw.to(DEV), lb.to(DEV), EPS, wq.to(DEV), ws.to(DEV),
                                                None if b is None else b.to(DEV), want_q=True)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and y.dtype == dtype
    rq, rs, rmean, rrstd = R.ln_quantize(x, lw, lb, EPS)
    # 1. statistics, scales, codes
    torch.testing.assert_close(mean.cpu().double(), rmean, rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(rstd.cpu().double(), rrstd, rtol=2e-6, atol=0)
    torch.testing.assert_close(xs.cpu(), rs, rtol=2e-6, atol=0)
    d = (R.code_order(xq) - R.code_order(rq)).abs()
    share = float((d != 0).double().mean())
    print(f"{tag}: differing codes {share:.3e}, largest step {int(d.max())}")
    assert int(d.max()) <= 1, f"a code differs by {int(d.max())} steps"
    assert share <= 1e-4, share
    # 2. the product of the kernel's own codes
    own = R.product(xq, xs, wq, ws, b)
    e_own = R.rel_fro(y, own)
    # 3. end to end
    exact = R.exact_product(x, lw, lb, EPS, w_nk, b)
    e_q = R.rel_fro(R.product(rq, rs, wq, ws, b), exact)
    name = str(dtype).replace("torch.", "")
    m = record_parity("ln_linear_fp8.y", y.double().cpu().numpy(), exact.numpy(), name, e_q=e_q, e_own=e_own, code_share=share)
    print(f"{tag}: own-product error {e_own:.3e} (gate {GATE[dtype]:.1e}); end to end {m['rel_fro']:.3e}, e_q {e_q:.3e}")
    assert e_own <= GATE[dtype], e_own
    assert m["rel_fro"] <= e_q + GATE[dtype], (m["rel_fro"], e_q)
    return y, xq, xs


@pytest.mark.parametrize("rows,n,dtype", [(1, 32, torch.bfloat16), (31, 96, torch.float16), (33, 32, torch.bfloat16),
                                          (255, 96, torch.bfloat16), (257, 2048, torch.bfloat16), (1000, 2048, torch.float16),
                                          (40000, 96, torch.bfloat16)])
def test_fused_vs_restatement(rows, n, dtype):
    """row counts on both sides of a wave's 32 rows and the workgroup's 256, one tile / an odd number / 2048 columns, and one
    case whose workgroups' runs start in the middle of a row block (40,000 rows = 157 blocks x 3 tiles = 471 units)"""
    x, lw, lb, w_nk, b = _inputs(rows, n, dtype, seed=rows + n)
    _check_fused(x, lw, lb, w_nk, b, dtype, f"{rows}x{n}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fused_rows_far_from_zero_mean_and_a_zero_row(dtype):
    """Row means of ~5 sigma-units (up to ~20 sigma of the row), many of them between 1 and 8 sigma where a one-pass
    variance has lost up to 64x of the sums' precision: the kernel's centred pass has to cover them.  And two all-zero rows:
    their normalised values are ln_b.

    Why 5 and not the 16-bit test's 20: the kernel's mean is an fp32 sum (as hstu_ln_linear_fwd writes it), off by
    ~3 ulp(sum) / 512 ~ 1e-6 |mean| / 4; that offset times rstd moves every normalised value of the row, and a value
    crosses an e4m3 rounding boundary with probability offset x 448 / amax / spacing(8 around 64..128) -- ~2e-5 at
    |mean| ~ 5, but ~1e-4, the cap itself, at |mean| ~ 20."""
    x, lw, lb, w_nk, b = _inputs(300, 96, dtype, seed=5, mean_shift=5.0)
    x[17] = 0
    x[299] = 0
    _check_fused(x, lw, lb, w_nk, b, dtype, "mean_shift")


def test_fused_zero_row_without_ln_bias_has_scale_one():
    x, lw, lb, w_nk, b = _inputs(40, 64, torch.bfloat16, seed=9)
    x[3] = 0
    lb = torch.zeros_like(lb)
    y, xq, xs = _check_fused(x, lw, lb, w_nk, b, torch.bfloat16, "zero row")
    assert xs[3].item() == 1.0 and int(xq[3].view(torch.uint8).cpu().max() & 0x7F) == 0
    assert torch.equal(y[3].cpu(), b)


def test_fused_optional_outputs_and_bias():
    """no codes asked for, no bias: the same y"""
    L = _launch()
    x, lw, lb, w_nk, b = _inputs(130, 64, torch.bfloat16, seed=21)
    wq, ws = (t.to(DEV) for t in R.quantize_rows(w_nk))
    y0, xq, xs, _, _ = L.ln_linear_fp8_fwd(x.to(DEV), lw.to(DEV), lb.to(DEV), EPS, wq, ws, None, want_q=True)
    y1, none_q, none_s, _, _ = L.ln_linear_fp8_fwd(x.to(DEV), lw.to(DEV), lb.to(DEV), EPS, wq, ws, None, want_q=False)
    assert none_q is None and none_s is None and torch.equal(y0, y1)
    assert R.rel_fro(y0, R.product(xq, xs, wq, ws)) <= GATE[torch.bfloat16]


# ----------------------------------------------------------------------------- determinism, row independence, no-LN entry
def test_determinism_row_independence_and_the_plain_entry():
    L = _launch()
    x, lw, lb, w_nk, b = _inputs(300, 2048, torch.bfloat16, seed=77, mean_shift=1.0)
    wq, ws = (t.to(DEV) for t in R.quantize_rows(w_nk))
    xd, lwd, lbd, bd = x.to(DEV), lw.to(DEV), lb.to(DEV), b.to(DEV)
    run = lambda rows: L.ln_linear_fp8_fwd(rows, lwd, lbd, EPS, wq, ws, bd, want_q=True)[:3]
    y, xq, xs = run(xd)
    y2, xq2, xs2 = run(xd)
    assert torch.equal(y, y2) and torch.equal(xq.view(torch.uint8), xq2.view(torch.uint8)) and torch.equal(xs, xs2)
    for lo, hi in ((0, 1), (37, 70), (255, 300), (100, 101)):
        ya, qa, sa = run(xd[lo:hi])
        assert torch.equal(ya, y[lo:hi]), (lo, hi)
        assert torch.equal(qa.view(torch.uint8), xq[lo:hi].view(torch.uint8)) and torch.equal(sa, xs[lo:hi]), (lo, hi)
    # the kernel without its LayerNorm, on the fused kernel's codes and scales: the same bits
    yp = L.linear_fp8_rowwise(xq, xs, wq, ws, bd, out_dtype=torch.bfloat16)
    assert torch.equal(yp, y)


def test_gpu_quantizer_feeds_the_fused_kernel():
    """the production path: weight quantized on the device, then the fused kernel -- equal to the CPU-quantized weight's result"""
    L = _launch()
    x, lw, lb, w_nk, b = _inputs(64, 96, torch.float16, seed=31)
    wq, ws = L.quantize_rows_fp8(w_nk.to(DEV))
    rq, rs = R.quantize_rows(w_nk)
    assert torch.equal(wq.cpu().view(torch.uint8), rq.view(torch.uint8)) and torch.equal(ws.cpu(), rs)
    y = L.ln_linear_fp8_fwd(x.to(DEV), lw.to(DEV), lb.to(DEV), EPS, wq, ws, b.to(DEV))[0]
    y_ref = L.ln_linear_fp8_fwd(x.to(DEV), lw.to(DEV), lb.to(DEV), EPS, rq.to(DEV), rs.to(DEV), b.to(DEV))[0]
    assert torch.equal(y, y_ref)
