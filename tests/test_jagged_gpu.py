"""GPU tests of the jagged helpers through the C ABI: BIT-EXACT against the numpy oracle
and the golden vectors of the reference's PyTorch path (parameter space of
ops/tests/jagged_tensors_test.py:36-64,159-187: B 2-8, lengths 20-100, odd D 10-30,
either side dense, bf16/fp32, backward checked)."""

import numpy as np
import pytest
import torch

from conftest import load_cases
from oracle import hstu_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _jt():
    from generative_recommenders_amd.ops import jagged_tensors

    return jagged_tensors


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 1000, 1024, 1025, 5000])
def test_complete_cumsum(dtype, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 300, (n,), generator=g).to(dtype)
    got = _jt().asynchronous_complete_cumsum(x.to(DEV))
    ref = O.complete_cumsum(x.numpy())
    assert got.dtype == dtype
    assert np.array_equal(got.cpu().numpy(), ref)


@pytest.mark.parametrize("idx", range(4))
def test_golden_concat_split(idx):
    c = load_cases("jagged.npz")[idx]
    da, db = bool(c["dense_a"]), bool(c["dense_b"])
    ma, mb = int(c["ma"]), int(c["mb"])
    oa = None if da else _dev(c["oa"])
    ob = None if db else _dev(c["ob"])
    cat = _jt().concat_2D_jagged(ma + mb, _dev(c["va"]), _dev(c["vb"]), ma, mb, oa, ob)
    assert np.array_equal(cat.cpu().numpy(), c["cat"])
    l, r = _jt().split_2D_jagged(ma + mb, _dev(c["cat"]), None, None, ma if da else None, mb if db else None, oa, ob)
    assert np.array_equal(l.cpu().numpy(), c["split_l"]) and np.array_equal(r.cpu().numpy(), c["split_r"])


def test_golden_l2_prefix():
    c = load_cases("jagged_l2.npz")[0]
    ctx = int(c["ctx"])
    cat = _jt().hstu_concat_l2_embeddings(int(c["mp"]), _dev(c["px"]), _dev(c["op"]), int(c["ml"]), _dev(c["lx"]),
                                          _dev(c["ol"]), ctx)
    assert np.array_equal(cat.cpu().numpy(), c["cat"])
    p, l = _jt().hstu_split_l2_embeddings(int(c["mp"]) + int(c["ml"]), _dev(c["cat"]), _dev(c["op"]), _dev(c["ol"]), ctx)
    assert np.array_equal(p.cpu().numpy(), c["split_p"]) and np.array_equal(l.cpu().numpy(), c["split_l"])


@pytest.mark.parametrize("seed", range(12))
def test_concat_split_sweep_with_backward(seed):
    rng = np.random.default_rng(seed)
    B = int(rng.integers(2, 9))
    ma, mb = int(rng.integers(20, 101)), int(rng.integers(20, 101))
    D = int(rng.integers(10, 31)) if seed % 3 else int(rng.choice([16, 64, 128, 512]))
    dense_a, dense_b = seed % 4 == 1, seed % 4 == 2
    dtype = [torch.float32, torch.bfloat16, torch.float16][seed % 3]
    idt = np.int32 if seed % 2 else np.int64
    la = np.full(B, ma) if dense_a else rng.integers(0, ma + 1, size=B)
    lb = np.full(B, mb) if dense_b else rng.integers(0, mb + 1, size=B)
    oa, ob = O.complete_cumsum(la.astype(idt)), O.complete_cumsum(lb.astype(idt))
    va = torch.randn(int(oa[-1]), D).to(dtype)
    vb = torch.randn(int(ob[-1]), D).to(dtype)
    ref_cat = O.concat_2D_jagged(va.view(torch.int16 if dtype != torch.float32 else torch.int32).numpy(),
                                 vb.view(torch.int16 if dtype != torch.float32 else torch.int32).numpy(), ma, mb,
                                 None if dense_a else oa, None if dense_b else ob)
    vad, vbd = va.to(DEV).requires_grad_(), vb.to(DEV).requires_grad_()
    oad = None if dense_a else _dev(oa)
    obd = None if dense_b else _dev(ob)
    cat = _jt().concat_2D_jagged(ma + mb, vad, vbd, ma, mb, oad, obd)
    bits = cat.detach().view(torch.int16 if dtype != torch.float32 else torch.int32).cpu().numpy()
    assert np.array_equal(bits, ref_cat)
    # backward of concat == split of the incoming gradient (bit-exact copy)
    g = torch.randn_like(cat)
    cat.backward(g)
    gl, gr = O.split_2D_jagged(g.float().cpu().numpy(), ma if dense_a else None, mb if dense_b else None,
                               None if dense_a else oa, None if dense_b else ob)
    assert np.array_equal(vad.grad.float().cpu().numpy(), gl) and np.array_equal(vbd.grad.float().cpu().numpy(), gr)
    # split round trip + its backward
    cat2 = cat.detach().clone().requires_grad_()
    l, r = _jt().split_2D_jagged(ma + mb, cat2, None, None, ma if dense_a else None, mb if dense_b else None, oad, obd)
    assert torch.equal(l, vad.detach()) and torch.equal(r, vbd.detach())
    (l.float().sum() * 2 + r.float().sum() * 3).backward()
    exp = O.concat_2D_jagged(np.full((l.shape[0], D), 2.0), np.full((r.shape[0], D), 3.0), ma, mb,
                             None if dense_a else oa, None if dense_b else ob)
    assert np.array_equal(cat2.grad.float().cpu().numpy(), exp)


@pytest.mark.parametrize("seed", range(6))
def test_padded_dense_roundtrip(seed):
    rng = np.random.default_rng(100 + seed)
    B, N = int(rng.integers(1, 9)), int(rng.integers(1, 70))
    D = int(rng.choice([1, 7, 16, 50, 64, 256]))
    lengths = rng.integers(0, N + 10, size=B)  # some users longer than N: truncated
    off = O.complete_cumsum(lengths.astype(np.int64))
    vals = rng.standard_normal((int(off[-1]), D)).astype(np.float32)
    dense = _jt().jagged_to_padded_dense(_dev(vals), _dev(off), N)
    assert np.array_equal(dense.cpu().numpy(), O.jagged_to_padded_dense(vals, off, N))
    back = _jt().dense_to_jagged(dense, _dev(off), int(off[-1]))
    ref_back = O.dense_to_jagged(O.jagged_to_padded_dense(vals, off, N), off)
    assert np.array_equal(back.cpu().numpy(), ref_back)


def test_padded_dense_3d_values_and_grad():
    rng = np.random.default_rng(5)
    lengths = np.array([3, 0, 5, 2])
    off = O.complete_cumsum(lengths.astype(np.int64))
    vals = torch.randn(int(off[-1]), 2, 8, device=DEV, requires_grad=True)
    dense = _jt().jagged_to_padded_dense(vals, _dev(off), 6)
    assert dense.shape == (4, 6, 2, 8)
    dense.sum().backward()
    assert torch.equal(vals.grad, torch.ones_like(vals))


def test_1d_helpers():
    vals = torch.tensor([1, 2, 3, 4, 5, 6], device=DEV)
    off = torch.tensor([0, 2, 2, 6], device=DEV)
    d = _jt().expand_1d_jagged_to_dense(vals, off, 3)
    assert d.cpu().tolist() == [[1, 2, 2], [0, 0, 0], [3, 4, 5]]
    c = _jt().concat_1d_jagged_jagged(torch.tensor([1, 0, 2], device=DEV), torch.tensor([7, 8, 9], device=DEV),
                                      torch.tensor([2, 1, 0], device=DEV), torch.tensor([1, 2, 3], device=DEV))
    assert c.cpu().tolist() == [7, 1, 2, 3, 8, 9]


@pytest.mark.parametrize("max_len", [1, 64, 65, 200])          # 64 | 65: one | two blocks along the row
@pytest.mark.parametrize("vdtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("odtype", [torch.int32, torch.int64])
def test_expand_1d_jagged_to_dense_vs_oracle(max_len, vdtype, odtype):
    lengths = np.array([0, 1, max_len, max_len + 7, 3, 70])      # empty; its one value repeated; exact; longer than max_len
    off = O.complete_cumsum(lengths)
    rng = np.random.default_rng(max_len)
    hi = 2 ** 31 - 1 if vdtype == torch.int32 else 2 ** 62
    vals = torch.from_numpy(rng.integers(-hi, hi, size=int(off[-1]))).to(vdtype)
    got = _jt().expand_1d_jagged_to_dense(vals.to(DEV), torch.from_numpy(off).to(odtype).to(DEV), max_len)
    ref = O.expand_1d_jagged_to_dense(vals.numpy(), off, max_len)
    assert got.dtype == vdtype and got.shape == ref.shape
    assert np.array_equal(got.cpu().numpy(), ref)
    assert not ref[0].any() and (ref[1] == ref[1, 0]).all()


@pytest.mark.parametrize("vdtype", [torch.int32, torch.int64])
def test_concat_1d_jagged_jagged_vs_oracle(vdtype):
    # more than 128 elements in one user (the block-stride loop), 128 and 129 exactly, empty on either side and on both
    ll = np.array([100, 0, 5, 0, 128, 300, 1])
    lr = np.array([90, 7, 0, 0, 1, 0, 127])
    rng = np.random.default_rng(7)
    hi = 2 ** 31 - 1 if vdtype == torch.int32 else 2 ** 62
    vl = torch.from_numpy(rng.integers(-hi, hi, size=int(ll.sum()))).to(vdtype)
    vr = torch.from_numpy(rng.integers(-hi, hi, size=int(lr.sum()))).to(vdtype)
    got = _jt().concat_1d_jagged_jagged(_dev(ll), vl.to(DEV), _dev(lr), vr.to(DEV))
    ref = O.concat_1d_jagged_jagged(ll, vl.numpy(), lr, vr.numpy())
    assert got.dtype == vdtype
    assert np.array_equal(got.cpu().numpy(), ref)


def test_1d_helpers_refuse_2_byte_values():
    vals = torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int16, device=DEV)
    off = torch.tensor([0, 2, 2, 6], device=DEV)
    with pytest.raises(RuntimeError, match="expand_1d_jagged_to_dense: elem_bytes must be 4 or 8"):
        _jt().expand_1d_jagged_to_dense(vals, off, 3)
    lens = torch.tensor([2, 0, 1], device=DEV)
    with pytest.raises(RuntimeError, match="concat_1d_jagged_jagged: elem_bytes must be 4 or 8"):
        _jt().concat_1d_jagged_jagged(lens, vals[:3], lens, vals[3:])


def test_large_rows_no_int32_overflow():
    """> 2^31 bytes of payload: row offsets are computed in 64 bits (cf. *_large_tensor tests)."""
    B, D = 4, 1024
    la = np.full(B, 300_000)
    off = O.complete_cumsum(la.astype(np.int64))
    a = torch.ones(int(off[-1]), D, device=DEV, dtype=torch.bfloat16)
    b = torch.zeros(B * 2, D, device=DEV, dtype=torch.bfloat16)
    cat = _jt().concat_2D_jagged(300_002, a, b, None, 2, _dev(off), None)
    assert cat.shape[0] == a.shape[0] + b.shape[0]
    assert float(cat[-3].float().sum()) == D and float(cat[-1].float().sum()) == 0.0
