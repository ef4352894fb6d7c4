"""jagged_dense_bmm_broadcast_add on the GPU: every fixture case and larger shapes against the fp64 helper, gated by the
reference's own error on the same inputs (e_hip <= m * e_ref, jagged_bmm_ref.gate_multiplier), and the exact properties
of the kernels (determinism, layout and index-type independence, empty users, user splitting)."""

import numpy as np
import pytest
import torch

from conftest import record_parity
from jagged_bmm_ref import OP_TENSORS, bmm_fp64, gate_multiplier, load_op_case, op_case_files, rel_fro

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _op():
    from generative_recommenders_amd.ops.jagged_tensors import jagged_dense_bmm_broadcast_add

    return jagged_dense_bmm_broadcast_add


def run_hip(max_seq_len, off, jagged, dense, bias, d_out):
    """forward + backward on the GPU; inputs are CPU tensors (dense may be a strided view, kept as such on the device)"""
    j = jagged.to(DEV).requires_grad_()
    if dense.is_contiguous():
        d = dense.to(DEV).requires_grad_()
        dv = d
    else:   # transposed storage: the leaf is the (B, N, K) storage, the op sees its transpose
        d = dense.transpose(1, 2).contiguous().to(DEV).requires_grad_()
        dv = d.transpose(1, 2)
        assert not dv.is_contiguous()
    b = bias.to(DEV).requires_grad_()
    out = _op()(max_seq_len, off.to(DEV), j, dv, b)
    out.backward(d_out.to(DEV))
    torch.cuda.synchronize()
    dd = d.grad if dense.is_contiguous() else d.grad.transpose(1, 2)
    assert out.dtype == jagged.dtype and j.grad.dtype == jagged.dtype and dd.dtype == dense.dtype and b.grad.dtype == bias.dtype
    return dict(out=out.detach().cpu(), d_jagged=j.grad.cpu(), d_dense=dd.cpu(), d_bias=b.grad.cpu())


def gate(tag, dtype_name, got, ref_result, fp64):
    """every tensor: print, record, then require e_hip <= m * e_ref"""
    m = gate_multiplier(dtype_name)
    failures = []
    for name in OP_TENSORS:
        g = got[name].double().numpy()
        assert g.shape == fp64[name].shape, f"{tag}: {name} shape {g.shape}"
        assert np.isfinite(g).all(), f"{tag}: {name} has non-finite values"
        e_ref = rel_fro(ref_result[name], fp64[name])
        e_hip = record_parity(f"jagged_bmm {tag} {name}", g, fp64[name], dtype_name, e_ref=e_ref, gate=m)["rel_fro"]
        print(f"{tag:32s} {name:9s} e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  ratio {e_hip / max(e_ref, 1e-300):.2f} (m = {m})")
        if not e_hip <= m * e_ref:
            failures.append(f"{name}: e_hip {e_hip:.3e} > {m} * e_ref {e_ref:.3e}")
    assert not failures, f"{tag}: " + "; ".join(failures)


@pytest.mark.parametrize("path", op_case_files(), ids=lambda p: p.split("op_")[-1][:-4])
def test_fixture_case(path):
    c = load_op_case(path)
    dt = getattr(torch, c["dtype"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    dense = t(c["dense"])
    if int(c["dense_transposed"]):
        dense = dense.transpose(1, 2).contiguous().transpose(1, 2)
    got = run_hip(int(c["max_seq_len"]), torch.from_numpy(c["seq_offsets"]), t(c["jagged"]), dense, t(c["bias"]), t(c["d_out"]))
    fp64 = bmm_fp64(c["seq_offsets"], c["jagged"], c["dense"], c["bias"], c["d_out"])
    gate(c["name"] + " " + c["dtype"], c["dtype"], got, c, fp64)
    empty = np.flatnonzero(np.diff(c["seq_offsets"]) == 0)
    assert not got["d_dense"][empty].float().any() and not got["d_bias"][empty].float().any()


def test_no_fixture_case_left_out():
    assert len(op_case_files()) == 15


def padded_bmm_reference(max_seq_len, off, jagged, dense, bias, d_out):
    """what the reference computes, restated with plain torch on the CPU: pad to (B, max_seq_len, .), fp32 bmm, one rounding"""
    dt = jagged.dtype
    B, K, N = dense.shape
    lens = (off[1:] - off[:-1]).tolist()

    def pad(x):
        p = torch.zeros(B, max_seq_len, x.shape[1], dtype=torch.float32)
        for u, n in enumerate(lens):
            p[u, :n] = x[off[u]:off[u + 1]].float()
        return p

    def unpad(p):
        return torch.cat([p[u, :n] for u, n in enumerate(lens)], 0) if sum(lens) else p.new_zeros(0, p.shape[2])

    pj, pg, d32 = pad(jagged), pad(d_out), dense.float()
    out = unpad(torch.bmm(pj, d32) + bias.float().unsqueeze(1)).to(dt)
    dj = unpad(torch.bmm(pg, d32.transpose(1, 2))).to(dt)
    dd = torch.bmm(pj.transpose(1, 2), pg).to(dt)
    db = pg.sum(1).to(dt)
    return dict(out=out.float().numpy(), d_jagged=dj.float().numpy(), d_dense=dd.float().numpy(), d_bias=db.float().numpy())


def make_inputs(lengths, K, N, dtype, seed, offsets_dtype=torch.int64):
    g = torch.Generator().manual_seed(seed)
    off = torch.zeros(len(lengths) + 1, dtype=offsets_dtype)
    off[1:] = torch.cumsum(torch.as_tensor(lengths), 0)
    L, B = int(off[-1]), len(lengths)
    jagged = torch.empty(L, K).uniform_(-1, 1, generator=g).to(dtype)
    dense = torch.empty(B, K, N).uniform_(-1, 1, generator=g).to(dtype)
    bias = torch.empty(B, N).uniform_(-1, 1, generator=g).to(dtype)
    d_out = (torch.randn(L, N, generator=g) * 0.01).to(dtype)
    return off, jagged, dense, bias, d_out


def m_jag_lengths(B, max_seq_len, seed):
    """the benchmark's M-jag family: uniform lengths in [max_seq_len / 2, max_seq_len]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(max_seq_len // 2, max_seq_len + 1, (B,), generator=g).tolist()


LARGE = {
    "mjag_B64_256x512_bf16": (lambda: m_jag_lengths(64, 200, 1), 200, 256, 512, torch.bfloat16),
    "long_user_64x64_bf16": (lambda: [32768, 1, 0], 32768, 64, 64, torch.bfloat16),
    "k200_n30_bf16": (lambda: [100, 0, 37, 64, 1, 77], 100, 200, 30, torch.bfloat16),
    "k200_n30_fp16": (lambda: [100, 0, 37, 64, 1, 77], 100, 200, 30, torch.float16),
    "k200_n30_fp32": (lambda: [100, 0, 37, 64, 1, 77], 100, 200, 30, torch.float32),
}


@pytest.mark.parametrize("name", list(LARGE))
def test_larger_shapes(name):
    lengths, max_seq_len, K, N, dtype = LARGE[name]
    off, jagged, dense, bias, d_out = make_inputs(lengths(), K, N, dtype, seed=len(name))
    got = run_hip(max_seq_len, off, jagged, dense, bias, d_out)
    ref = padded_bmm_reference(max_seq_len, off, jagged, dense, bias, d_out)
    fp64 = bmm_fp64(off.numpy(), jagged.float().numpy(), dense.float().numpy(), bias.float().numpy(), d_out.float().numpy())
    gate(name, str(dtype)[6:], got, ref, fp64)


# ---- exact properties ---------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in OP_TENSORS)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_bit_identical_across_runs_index_types_and_dense_layouts(dtype):
    lengths = [70, 0, 1, 64, 129, 33]
    off, jagged, dense, bias, d_out = make_inputs(lengths, 88, 152, dtype, seed=5)
    first = run_hip(129, off, jagged, dense, bias, d_out)
    again = run_hip(129, off, jagged, dense, bias, d_out)
    assert _same(first, again), "two runs differ"
    assert _same(first, run_hip(129, off.to(torch.int32), jagged, dense, bias, d_out)), "int32 and int64 offsets differ"
    transposed = dense.transpose(1, 2).contiguous().transpose(1, 2)
    assert _same(first, run_hip(129, off, jagged, transposed, bias, d_out)), "transposed-storage dense differs"
    # empty user: exact zeros, and nothing anywhere is NaN (LDS is poisoned before every GPU test)
    assert not first["d_dense"][1].float().any() and not first["d_bias"][1].float().any()
    for k in OP_TENSORS:
        assert torch.isfinite(first[k].float()).all(), k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_odd_shapes_take_the_padded_path_bit_identically_across_layouts(dtype):
    off, jagged, dense, bias, d_out = make_inputs([19, 0, 45], 37, 23, dtype, seed=9)
    first = run_hip(45, off, jagged, dense, bias, d_out)
    assert _same(first, run_hip(45, off, jagged, dense.transpose(1, 2).contiguous().transpose(1, 2), bias, d_out))
    assert first["out"].shape == (64, 23) and first["d_dense"].shape == (3, 37, 23)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_identity_dense_and_zero_bias_return_jagged_exactly(dtype):
    lengths, K = [5, 0, 130, 64], 72
    off, jagged, _, _, _ = make_inputs(lengths, K, K, dtype, seed=3)
    dense = torch.eye(K, dtype=dtype).repeat(len(lengths), 1, 1)
    out = _op()(130, off.to(DEV), jagged.to(DEV), dense.to(DEV), torch.zeros(len(lengths), K, dtype=dtype, device=DEV))
    assert torch.equal(out.cpu(), jagged)
    # asymmetric selection: dense[b] routes column (c + 1) % K of jagged to column c (a transposed output map would not)
    perm = torch.roll(torch.eye(K, dtype=dtype), 1, 0).repeat(len(lengths), 1, 1)
    out = _op()(130, off.to(DEV), jagged.to(DEV), perm.to(DEV), torch.zeros(len(lengths), K, dtype=dtype, device=DEV))
    assert torch.equal(out.cpu(), torch.roll(jagged, -1, 1))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_splitting_a_user_leaves_out_and_d_jagged_bit_identical(dtype):
    off, jagged, dense, bias, d_out = make_inputs([150, 40], 96, 136, dtype, seed=11)
    whole = run_hip(150, off, jagged, dense, bias, d_out)
    off2 = torch.tensor([0, 83, 150, 190])          # user 0 split at a row that is no tile boundary
    dense2, bias2 = dense[[0, 0, 1]].contiguous(), bias[[0, 0, 1]].contiguous()
    split = run_hip(150, off2, jagged, dense2, bias2, d_out)
    assert torch.equal(whole["out"], split["out"]) and torch.equal(whole["d_jagged"], split["d_jagged"])


def test_row_strided_views_and_empty_inputs():
    off, jagged, dense, bias, d_out = make_inputs([33, 7], 64, 128, torch.bfloat16, seed=13)
    base = run_hip(33, off, jagged, dense, bias, d_out)
    wide = torch.zeros(40, 96, dtype=torch.bfloat16, device=DEV)
    wide[:, 16:80] = jagged.to(DEV)
    out = _op()(33, off.to(DEV), wide[:, 16:80], dense.to(DEV), bias.to(DEV))        # row stride 96, no copy needed
    assert torch.equal(out.cpu(), base["out"])
    # sum(L) == 0 with users, and B == 0: shapes right, gradients zero, no launch needed
    z = torch.zeros(3, dtype=torch.int64, device=DEV)
    j0 = torch.zeros(0, 64, dtype=torch.bfloat16, device=DEV, requires_grad=True)
    d0 = dense.to(DEV).requires_grad_()
    b0 = bias.to(DEV).requires_grad_()
    o = _op()(5, z, j0, d0, b0)
    assert o.shape == (0, 128)
    o.sum().backward()
    assert not d0.grad.float().any() and not b0.grad.float().any() and j0.grad.shape == (0, 64)
    o = _op()(5, z[:1], j0, d0[:0], b0[:0])
    assert o.shape == (0, 128)


def test_fp32_bias_with_bf16_rows_as_the_module_passes_it():
    """the module hands over an fp32 bias next to 16-bit rows: the bias is added in fp32 either way, so with bf16-representable
    values nothing changes bit for bit, and the bias gradient comes back in fp32, unrounded: against the fp64 column sums it
    may be off by fp32 summation only, at most n * 2^-24 relative to sum |d_out| over the n <= 50 rows of a user"""
    off, jagged, dense, bias, d_out = make_inputs([50, 0, 21], 64, 72, torch.bfloat16, seed=17)
    base = run_hip(50, off, jagged, dense, bias, d_out)
    got = run_hip(50, off, jagged, dense, bias.float(), d_out)
    for k in ("out", "d_jagged", "d_dense"):
        assert torch.equal(base[k], got[k]), k
    assert got["d_bias"].dtype == torch.float32
    g = d_out.double()
    for u in range(3):
        rows = g[off[u]:off[u + 1]]
        err = (got["d_bias"][u].double() - rows.sum(0)).abs()
        assert (err <= 50 * 2.0 ** -24 * rows.abs().sum(0)).all()
