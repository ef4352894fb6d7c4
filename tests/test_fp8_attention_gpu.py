"""GPU tests of the fp8 (e4m3) HSTU attention forward and the jagged e4m3 quantizer (ops/fp8.py).

Parity: bf16 inputs drawn like tests/test_attention_gpu.py (uniform(-0.1, 0.1)), but with every (user, head) of q, k and v
scaled by its own magnitude, log-uniform over 1e-3 .. 300 -- so the per-(user, head) descales differ by orders of magnitude
and a descale read for the wrong user or head (or through swapped batch / head strides) is visible -- quantized per (user,
head) with quantize_jagged_fp8, against the fp64 oracle on the DEQUANTIZED inputs (x8 * descale[b, h]).  Gates: those of the
bf16 tests of that file, relative Frobenius <= 3.8e-3 and element-wise <= 2e-2 |ref| + 4e-3 max|ref| over the whole output,
and the element-wise gate again inside every (user, head) block with that block's own max|ref| (the blocks' scales differ
by up to 1e5: the global gate alone would not look at the small ones).  e4m3 values are exact in bf16 and the e4m3 MFMA
accumulates exact products in fp32, so the kernel's only roundings are P and the output, as on the bf16 path.
"""

import numpy as np
import pytest
import torch

from conftest import record_parity
from oracle import hstu_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn


def _fp8():
    from generative_recommenders_amd.ops import fp8, torch_library

    torch_library.register()   # torch.ops.hstu.* (idempotent)
    return fp8


def _check(got: torch.Tensor, ref: np.ndarray, what: str, off=None):
    assert got.dtype == torch.bfloat16, got.dtype
    g = got.detach().double().cpu().numpy()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert np.isfinite(g).all(), f"{what}: non-finite values"
    record_parity(what, g, ref, "bfloat16")
    err = np.abs(g - ref)
    scale = max(np.abs(ref).max(), 1e-30)
    fro = np.linalg.norm(err) / max(np.linalg.norm(ref), 1e-30)
    assert fro <= 3.8e-3, f"{what}: relative Frobenius error {fro:.3e} (gate 3.8e-3)"
    bad = err > 2e-2 * np.abs(ref) + 4e-3 * scale
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} elements out of tolerance, max err {err.max():.3e} (scale {scale:.3e})"
    if off is None:
        return
    for b in range(len(off) - 1):
        for h in range(ref.shape[1]):
            r, e = ref[off[b]:off[b + 1], h], err[off[b]:off[b + 1], h]
            if r.size == 0 or np.abs(r).max() == 0:
                continue
            bad = e > 2e-2 * np.abs(r) + 4e-3 * np.abs(r).max()
            assert not bad.any(), f"{what}: user {b} head {h}: {bad.sum()} / {bad.size} elements out of tolerance, max err {e.max():.3e} (block scale {np.abs(r).max():.3e})"


def _offsets(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lengths)
    return off


def _dequant(x8: torch.Tensor, descale: torch.Tensor, off: np.ndarray) -> np.ndarray:
    """x8 * descale[b, h] on the rows of user b (fp64)"""
    x = x8.double().cpu().numpy()
    d = descale.double().cpu().numpy()
    for b in range(len(off) - 1):
        x[off[b]:off[b + 1]] *= d[b][None, :, None]
    return x


def _draw(rng, off, H, d):
    """uniform(-0.1, 0.1), every (user, head) block scaled by its own magnitude (log-uniform, 1e-3 .. 300), as bf16"""
    x = rng.uniform(-0.1, 0.1, (int(off[-1]), H, d))
    mag = 10.0 ** rng.uniform(-3.0, np.log10(300.0), (len(off) - 1, H))
    for b in range(len(off) - 1):
        x[off[b]:off[b + 1]] *= mag[b][None, :, None]
    return torch.from_numpy(x).to(torch.bfloat16).to(DEV)


CASES = [
    # H, d, lengths, N, options
    (1, 32, [0, 1, 127, 128, 129, 250], 256, dict()),
    (2, 64, [200, 0, 37, 225, 96], 256, dict(targets=True)),
    (4, 128, [129, 64, 230, 1, 160], 256, dict(max_attn_len=40, min_full_attn_seq_len=20)),
    (2, 128, [90, 200, 31, 150], 224, dict(contextual_seq_len=5, targets=True)),
    (2, 64, [2048, 700, 1500], 2048, dict()),
    (1, 128, [1024, 33, 2000], 2048, dict(targets=True, max_attn_len=300)),
    (4, 64, [120, 255, 17], 256, dict(attn_scale=True)),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_fp8_parity_jagged(case):
    H, d, lengths, N, opt = CASES[case]
    rng = np.random.default_rng(100 + case)
    off = _offsets(lengths)
    L = int(off[-1])
    q, k, v = (_draw(rng, off, H, d) for _ in range(3))
    offt = torch.from_numpy(off).to(DEV)
    F = _fp8()
    (q8, qd), (k8, kd), (v8, vd) = (F.quantize_jagged_fp8(x, offt) for x in (q, k, v))
    nt = rng.integers(1, 6, size=len(lengths)).clip(max=np.maximum(np.array(lengths), 1)) if opt.get("targets") else None
    alpha = 1.0 / d**0.5
    kw = dict(max_attn_len=opt.get("max_attn_len", 0), contextual_seq_len=opt.get("contextual_seq_len", 0),
              min_full_attn_seq_len=opt.get("min_full_attn_seq_len", 0))
    ref = O.hstu_mha_fwd(N, alpha, _dequant(q8, qd, off), _dequant(k8, kd, off), _dequant(v8, vd, off), off,
                         num_targets=nt, **kw)
    ntt = None if nt is None else torch.from_numpy(nt).to(DEV)
    if opt.get("attn_scale"):
        # the operator path: attn_scale element 0 replaces 1/N
        out = torch.ops.hstu.hstu_mha_fwd(N, alpha, q8, k8, v8, offt, True, ntt, torch.full((1,), 3.0 / N, device=DEV), kw["max_attn_len"],
                                          kw["min_full_attn_seq_len"], kw["contextual_seq_len"], qd, kd, vd, 0)
        ref = ref * 3.0
    else:
        out = F.hstu_mha_fp8(N, alpha, q8, k8, v8, offt, q_descale=qd, k_descale=kd, v_descale=vd, num_targets=ntt, **kw)
    _check(out, ref, f"fp8 out H={H} d={d}", off)
    # sort_by_length changes the launch order only
    out2 = F.hstu_mha_fp8(N, alpha, q8, k8, v8, offt, q_descale=qd, k_descale=kd, v_descale=vd, num_targets=ntt, sort_by_length=True,
                          **kw)
    if not opt.get("attn_scale"):
        assert torch.equal(out, out2)


def test_fp8_descales_none_and_dense_layout():
    rng = np.random.default_rng(7)
    B, S, H, d = 3, 160, 2, 64
    x = [torch.from_numpy(rng.uniform(-1.0, 1.0, (B, S, H, d))).to(FP8).to(DEV) for _ in range(3)]
    off = np.arange(B + 1, dtype=np.int64) * S
    flat = [t.reshape(B * S, H, d) for t in x]
    alpha = 0.125
    ref = O.hstu_mha_fwd(S, alpha, *(t.double().cpu().numpy() for t in flat), off)
    out = _fp8().hstu_mha_fp8(S, alpha, *flat, torch.from_numpy(off).to(DEV))
    _check(out, ref, "fp8 out, descales None")
    # dense (B, S, H, d) through the operator, no offsets == the jagged call
    od = torch.ops.hstu.hstu_mha_fwd(S, alpha, x[0], x[1], x[2], None, True, None, None, 0, 0, 0, None, None, None, 0)
    assert od.shape == (B, S, H, d) and od.dtype == torch.bfloat16
    assert torch.equal(od.reshape(B * S, H, d), out)
    # the 16-bit entry point takes fp8 too (every descale 1, bf16 out)
    oh = _fp8_hstu_mha(S, alpha, flat, torch.from_numpy(off).to(DEV))
    assert torch.equal(oh, out)


@pytest.mark.parametrize("subnormal", [False, True])
def test_fp8_exact_integer_data_and_subnormals(subnormal):
    """The operand maps, pinned with exactly representable data: q, k small integers (every product and every dot product exact,
    so S is exact and a K / Q slot mis-pairing of the e4m3 MFMA moves whole integers), v integers (a wrong byte / word order in
    the widening of V to bf16 moves whole integers between columns).  subnormal=True: the same integers times 2^-9, i.e. e4m3
    subnormals (|m| 2^-9, |m| <= 7) through the e4m3 MFMA and the V widening."""
    rng = np.random.default_rng(21 + subnormal)
    H, d = 2, 128
    lengths = [96, 33, 0, 64]
    off = _offsets(lengths)
    L, N = int(off[-1]), 96
    unit = 2.0**-9 if subnormal else 1.0
    lim = 7 if subnormal else 3
    q, k = (rng.integers(-lim, lim + 1, (L, H, d)) * unit for _ in range(2))
    v = rng.integers(-7, 8, (L, H, d)) * unit
    t8 = [torch.from_numpy(x).to(FP8).to(DEV) for x in (q, k, v)]
    assert all(np.array_equal(t.double().cpu().numpy(), x) for t, x in zip(t8, (q, k, v)))   # exact in e4m3
    alpha = 2.0**11 if subnormal else 2.0**-6       # alpha S of order 1
    ref = O.hstu_mha_fwd(N, alpha, q, k, v, off)
    out = _fp8().hstu_mha_fp8(N, alpha, *t8, torch.from_numpy(off).to(DEV))
    _check(out, ref, f"fp8 integer data{' (subnormals)' if subnormal else ''}", off)


def _fp8_hstu_mha(N, alpha, qkv, off):
    from generative_recommenders_amd.ops.hstu_attention import hstu_mha

    return hstu_mha(N, alpha, *qkv, off)


def test_fp8_delta_attention():
    from generative_recommenders_amd.ops.hstu_attention import delta_hstu_mha

    rng = np.random.default_rng(11)
    B, H, d, delta = 5, 2, 128, 40
    lengths = [300, 40, 129, 256, 77]
    off = _offsets(lengths)
    N = max(lengths)
    offt = torch.from_numpy(off).to(DEV)
    F = _fp8()
    k, v = _draw(rng, off, H, d), _draw(rng, off, H, d)
    doff = np.arange(B + 1, dtype=np.int64) * delta
    dq = _draw(rng, doff, H, d)
    (k8, kd), (v8, vd) = F.quantize_jagged_fp8(k, offt), F.quantize_jagged_fp8(v, offt)
    q8, qd = F.quantize_jagged_fp8(dq, torch.from_numpy(doff).to(DEV))
    nt = np.array([3, 1, 40, 2, 5])
    alpha = 1.0 / d**0.5
    ref = O.delta_hstu_mha_fwd(N, alpha, _dequant(q8, qd, doff), _dequant(k8, kd, off), _dequant(v8, vd, off), off, num_targets=nt)
    out = F.hstu_mha_fp8(N, alpha, q8, k8, v8, offt, q_descale=qd, k_descale=kd, v_descale=vd,
                         num_targets=torch.from_numpy(nt).to(DEV), delta=True)
    _check(out, ref, "fp8 delta out", doff)
    # delta_hstu_mha on fp8 inputs: descale 1, bf16 out
    raw = lambda n: torch.from_numpy(rng.uniform(-1.0, 1.0, (n, H, d))).to(FP8).to(DEV)  # noqa: E731
    qr, kr, vr = raw(B * delta), raw(int(off[-1])), raw(int(off[-1]))
    ref1 = O.delta_hstu_mha_fwd(N, alpha, qr.double().cpu().numpy(), kr.double().cpu().numpy(), vr.double().cpu().numpy(), off)
    out1 = delta_hstu_mha(N, alpha, qr, kr, vr, offt)
    _check(out1, ref1, "fp8 delta_hstu_mha")


def test_fp8_operator_strided_descales_and_determinism():
    rng = np.random.default_rng(3)
    H, d = 4, 128
    lengths = [200, 150, 0, 199, 37]     # B = 5 != H = 4: a batch / head stride swap reads other (user, head) pairs
    off = _offsets(lengths)
    offt = torch.from_numpy(off).to(DEV)
    F = _fp8()
    q, k, v = (_draw(rng, off, H, d) for _ in range(3))
    (q8, qd), (k8, kd), (v8, vd) = (F.quantize_jagged_fp8(x, offt) for x in (q, k, v))
    ref = F.hstu_mha_fp8(200, 0.1, q8, k8, v8, offt, q_descale=qd, k_descale=kd, v_descale=vd)
    _check(ref, O.hstu_mha_fwd(200, 0.1, _dequant(q8, qd, off), _dequant(k8, kd, off), _dequant(v8, vd, off), off), "fp8 out", off)
    o1 = torch.ops.hstu.hstu_mha_fwd(200, 0.1, q8, k8, v8, offt, True, None, None, 0, 0, 0, qd, kd, vd, 0)
    o2 = torch.ops.hstu.hstu_mha_fwd(200, 0.1, q8, k8, v8, offt, True, None, None, 0, 0, 0, qd, kd, vd, 0)
    assert torch.equal(o1, ref) and torch.equal(o1, o2)
    # strided (B, H) descales: the .t() of (H, B) tensors
    st = [t.t().contiguous().t() for t in (qd, kd, vd)]
    assert st[0].stride() == (1, len(lengths))
    o3 = torch.ops.hstu.hstu_mha_fwd(200, 0.1, q8, k8, v8, offt, True, None, None, 0, 0, 0, *st, 0)
    assert torch.equal(o3, ref)
    # torch.ops.hstu.hstu_mha (the autograd-aware op) returns the same forward
    o4 = torch.ops.hstu.hstu_mha(200, 0.1, q8, k8, v8, offt, True, None, None, 0, 0, 0, qd, kd, vd, False, False, 0)
    assert torch.equal(o4, ref)


def test_fp8_kernel_name_and_memory_stays_fp8():
    from generative_recommenders_amd.ops import _launch

    assert "fp8" in _launch.attn_fwd_kernel_name(FP8, 128, 128, 200)
    assert "fp8" in _launch.attn_fwd_kernel_name(FP8, 32, 32, 200)
    B, L, H, d = 2048, 200, 4, 128
    off = torch.arange(B + 1, device=DEV, dtype=torch.int64) * L
    g = torch.Generator(device=DEV).manual_seed(0)
    q8, k8, v8 = ((torch.rand(B * L, H, d, device=DEV, generator=g) - 0.5).to(FP8) for _ in range(3))
    descale = torch.full((B, H), 0.01, device=DEV)
    F = _fp8()
    F.hstu_mha_fp8(L, 0.1, q8, k8, v8, off, q_descale=descale, k_descale=descale, v_descale=descale)   # (warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = F.hstu_mha_fp8(L, 0.1, q8, k8, v8, off, q_descale=descale, k_descale=descale, v_descale=descale)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    out_bytes = out.numel() * out.element_size()
    assert out.dtype == torch.bfloat16
    assert rise < out_bytes + (1 << 20), (rise, out_bytes)


def test_quantizer_bit_exact():
    F = _fp8()
    rng = np.random.default_rng(5)
    lengths = [0, 3, 130, 0, 57, 1]
    off = _offsets(lengths)
    offt = torch.from_numpy(off).to(DEV)
    L, H, d = int(off[-1]), 3, 64
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        x = torch.from_numpy(rng.standard_normal((L, H, d)) * rng.choice([1e-3, 1.0, 300.0], size=(1, H, 1))).to(dtype).to(DEV)
        x[int(off[2]):int(off[3]), 1] = 0       # an all-zero head of one user
        x8, ds = F.quantize_jagged_fp8(x, offt)
        amax = torch.stack([x[int(off[b]):int(off[b + 1])].float().abs().amax(dim=(0, 2)) if lengths[b] else torch.zeros(H, device=DEV)
                            for b in range(len(lengths))])
        # amax / 448 as an IEEE fp32 division (torch divides by a Python scalar through its reciprocal: one ulp apart at times;
        # the fp64 quotient rounded to fp32 is the correctly rounded one)
        want_ds = torch.where(amax > 0, (amax.double() / 448.0).float(), torch.ones_like(amax))
        assert torch.equal(ds, want_ds), dtype
        assert float(ds[2, 1]) == 1.0
        rows_ds = torch.repeat_interleave(ds, torch.tensor(lengths, device=DEV), dim=0)
        want = (x.float() / rows_ds[:, :, None]).clamp(-448, 448).to(FP8)
        assert torch.equal(x8.view(torch.uint8), want.view(torch.uint8)), dtype
    # strided views (q of a fused uvqk buffer; a row stride that is not 16-byte aligned takes the element path)
    for width in (4 * H * d, 4 * H * d + 1):
        buf = torch.randn(L, width, device=DEV, dtype=torch.bfloat16)
        xv = buf[:, H * d:2 * H * d].view(L, H, d) if width % 8 == 0 else buf[:, 1:H * d + 1].unflatten(1, (H, d))
        x8, ds = F.quantize_jagged_fp8(xv, offt)
        rows_ds = torch.repeat_interleave(ds, torch.tensor(lengths, device=DEV), dim=0)
        want = (xv.float() / rows_ds[:, :, None]).clamp(-448, 448).to(FP8)
        assert torch.equal(x8.view(torch.uint8), want.view(torch.uint8))


def test_fp8_refusals():
    F = _fp8()
    off = torch.tensor([0, 40, 100], device=DEV)
    mk = lambda d, dt=FP8: (torch.rand(100, 2, d, device=DEV) - 0.5).to(dt)  # noqa: E731
    q, k, v = mk(64), mk(64), mk(64)
    ones = torch.ones(2, 2, device=DEV)
    with pytest.raises(RuntimeError, match="bias|fp8"):
        # research-path relative bias: the C ABI refuses fp8 with pos_w
        from generative_recommenders_amd import _lib as L
        from generative_recommenders_amd.ops import _launch
        import ctypes as C

        p = L.HstuAttnParams()
        out = torch.empty(100, 2, 64, device=DEV, dtype=torch.bfloat16)
        _launch._fill_attn_params(p, q, k, v, out, off, None, 60, 0.1, 1 / 60, 0, 0, 0, 0)
        w = torch.zeros(2 * 60, device=DEV)
        p.pos_w = w.data_ptr()
        L.check(L.lib().hstu_attn_fwd(C.byref(p), None))
    with pytest.raises(RuntimeError, match="float8_e4m3fn|fp8"):
        F.hstu_mha_fp8(60, 0.1, q, k, mk(64, torch.bfloat16), off)
    with pytest.raises(RuntimeError, match="float8_e4m3fn|fp8"):
        torch.ops.hstu.hstu_mha_fwd(60, 0.1, q, k, mk(64, torch.bfloat16), off, True, None, None, 0, 0, 0, None, None, None, 0)
    with pytest.raises(RuntimeError, match="dqk == dv"):
        F.hstu_mha_fp8(60, 0.1, q, k, mk(32), off)
    with pytest.raises(RuntimeError, match="dqk == dv"):
        torch.ops.hstu.hstu_mha_fwd(60, 0.1, q, k, mk(32), off, True, None, None, 0, 0, 0, ones, None, None, 0)
    with pytest.raises(RuntimeError, match="above 128"):
        F.hstu_mha_fp8(60, 0.1, mk(192), mk(192), mk(192), off)
    with pytest.raises(RuntimeError, match="multiples of 16"):
        from generative_recommenders_amd.ops import _launch

        _launch.attn_fwd(mk(48)[..., :24], mk(48)[..., :24], mk(48)[..., :24], off, None, 60, 0.1, 1 / 60)
    with pytest.raises(RuntimeError, match="fp8"):     # descales with 16-bit q / k / v
        torch.ops.hstu.hstu_mha_fwd(60, 0.1, mk(64, torch.bfloat16), mk(64, torch.bfloat16), mk(64, torch.bfloat16), off, True, None, None,
                                    0, 0, 0, ones, ones, ones, 0)
    with pytest.raises(RuntimeError, match="fp8"):
        torch.ops.hstu.hstu_mha_bwd(60, 0.1, mk(64, torch.bfloat16), q, k, v, torch.empty_like(q), torch.empty_like(k), torch.empty_like(v),
                                    off, True, None, None, 0, 0, 0, False, False, 0)
    # backward through hstu_mha on fp8 inputs that require grad: the forward runs, .backward() names fp8
    from generative_recommenders_amd.ops.hstu_attention import hstu_mha

    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    out = hstu_mha(60, 0.1, qg, kg, vg, off)
    assert out.dtype == torch.bfloat16
    with pytest.raises(RuntimeError, match="fp8"):
        out.float().sum().backward()
    out2 = torch.ops.hstu.hstu_mha(60, 0.1, qg, kg, vg, off, True, None, None, 0, 0, 0, None, None, None, False, False, 0)
    with pytest.raises(RuntimeError, match="fp8"):
        out2.float().sum().backward()
