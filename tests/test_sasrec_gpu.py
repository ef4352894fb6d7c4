"""GPU tests of the SASRec baseline: the fused jagged causal softmax attention (forward, backward, dropout, strided inputs,
empty batches), the composition outside the fused range, and the module against the reference-minted fixtures.  Every
comparison is the gate of tests/softmax_attn_ref.py: e_hip <= m e_ref per whole-batch tensor against the fp64 truth."""

import numpy as np
import pytest
import torch

import softmax_attn_ref as R
from sasrec_stubs import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
OP_CASES = R.op_case_names()
MODEL_CASES = R.model_case_names()
DRAWN_LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 200, 210]


def _ops():
    from generative_recommenders_amd.ops import softmax_attention as SA

    return SA.jagged_causal_softmax_attention, SA.jagged_causal_softmax_attention_composed


def _offsets(lengths, dtype=torch.int64):
    return torch.from_numpy(R.offsets_of(lengths)).to(dtype).to(DEV)


def _run(fn, q, k, v, dout, lengths, n, dtype, **kw):
    """dict(out, dq, dk, dv) as float64 numpy of ``fn`` on the GPU"""
    leaves = [torch.from_numpy(np.ascontiguousarray(t)).to(dtype).to(DEV).requires_grad_(True) for t in (q, k, v)]
    out = fn(n, *leaves, _offsets(lengths), **kw)
    out.backward(torch.from_numpy(np.ascontiguousarray(dout)).to(dtype).to(DEV))
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    res.update({g: t.grad for g, t in zip(("dq", "dk", "dv"), leaves)})
    assert all(torch.isfinite(t).all() for t in res.values())
    return {g: t.double().cpu().numpy() for g, t in res.items()}


@pytest.fixture(scope="module")
def op_cases():
    return {n: R.load_op_case(n) for n in OP_CASES}


@pytest.fixture(scope="module")
def drawn():
    """the drawn batch (H 2, d 16, N 210) with its fp64 truth, bf16-exact values"""
    g = np.random.default_rng(20260)
    L = sum(DRAWN_LENGTHS)
    x = [R.round_to(g.standard_normal((L, 2, 16)), torch.bfloat16) for _ in range(4)]
    return {"x": x, "lengths": DRAWN_LENGTHS, "n": 210, "truth": R.restate(*x, DRAWN_LENGTHS)}


def _supported(dtype, d, n):
    from generative_recommenders_amd.ops import _launch

    return _launch.softmax_attn_supported(dtype, d, n)


# ------------------------------------------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("tag", ["bf16", "f32"])
@pytest.mark.parametrize("name", OP_CASES)
def test_fused_op_against_the_fixtures(op_cases, name, tag):
    c = op_cases[name]
    dtype = R.TORCH_DTYPE[tag]
    assert _supported(dtype, c["q"].shape[2], c["max_seq_len"])            # the fused path is what runs
    got = _run(_ops()[0], c["q"], c["k"], c["v"], c["dout"], c["lengths"], c["max_seq_len"], dtype)
    truth = {g: c[f"f64:{g}"] for g in R.GRADS}
    ref = {g: c[f"{tag}:{g}"] for g in R.GRADS}
    assert not R.gate(f"fused {name}", got, ref, truth, R.DTYPE_NAME[tag])


@pytest.mark.parametrize("tag", ["bf16", "f32"])
@pytest.mark.parametrize("name", OP_CASES)
def test_composition_against_the_fixtures(op_cases, name, tag):
    c = op_cases[name]
    got = _run(_ops()[1], c["q"], c["k"], c["v"], c["dout"], c["lengths"], c["max_seq_len"], R.TORCH_DTYPE[tag])
    truth = {g: c[f"f64:{g}"] for g in R.GRADS}
    ref = {g: c[f"{tag}:{g}"] for g in R.GRADS}
    assert not R.gate(f"composed {name}", got, ref, truth, R.DTYPE_NAME[tag])


@pytest.mark.parametrize("name", OP_CASES)
def test_fused_op_in_fp16(op_cases, name):
    c = op_cases[name]
    x = [R.round_to(c[k], torch.float16) for k in ("q", "k", "v", "dout")]
    assert _supported(torch.float16, x[0].shape[2], c["max_seq_len"])
    truth = R.restate(*x, c["lengths"])
    ref = R.math_path(*x, c["lengths"], c["max_seq_len"], torch.float16)
    got = _run(_ops()[0], *x, c["lengths"], c["max_seq_len"], torch.float16)
    assert not R.gate(f"fused fp16 {name}", got, ref, truth, "bfloat16")


@pytest.mark.parametrize("tag", ["bf16", "f32"])
def test_fused_op_on_the_drawn_batch(drawn, tag):
    dtype = R.TORCH_DTYPE[tag]
    assert _supported(dtype, 16, drawn["n"])
    ref = R.math_path(*drawn["x"], drawn["lengths"], drawn["n"], dtype)
    got = _run(_ops()[0], *drawn["x"], drawn["lengths"], drawn["n"], dtype)
    assert not R.gate("fused drawn", got, ref, drawn["truth"], R.DTYPE_NAME[tag])


def test_lse_is_the_log_sum_exp_of_the_undropped_scores(drawn):
    from generative_recommenders_amd.ops import _launch

    q, k, v = (torch.from_numpy(t).to(torch.bfloat16).to(DEV) for t in drawn["x"][:3])
    want = R.lse_of(drawn["x"][0], drawn["x"][1], drawn["lengths"])
    for p in (0.0, 0.5):
        _, lse = _launch.softmax_attn_fwd(q, k, v, _offsets(drawn["lengths"]), drawn["n"], 16 ** -0.5, p, 99)
        assert lse.dtype == torch.float32 and lse.shape == (q.shape[0], 2)
        assert np.abs(lse.double().cpu().numpy() - want).max() <= 2e-5 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_dropout_against_the_restatement_with_the_oracles_mask(drawn, p):
    from generative_recommenders_amd.ops import _launch

    x, lengths, n = drawn["x"], drawn["lengths"], drawn["n"]
    L, H, _ = x[0].shape
    seed = 0x1234_5678_9ABC
    keep, ks = R.keep_mask(seed, L, H, n, p)
    truth = R.restate(*x, lengths, keep=keep, keep_scale=ks)
    ref = R.math_path(*x, lengths, n, torch.bfloat16, keep=keep, keep_scale=ks)
    got = _run(_ops()[0], *x, lengths, n, torch.bfloat16, dropout_pr=p, seed=seed)
    assert not R.gate(f"dropout p={p}", got, ref, truth, "bfloat16")
    # the kept share among the visible elements, within 4 sigma of 1 - p
    offs = R.offsets_of(lengths)
    vis = np.zeros((L, H, n), dtype=bool)
    for b, ln in enumerate(lengths):
        vis[int(offs[b]): int(offs[b]) + ln, :, :ln] = np.tril(np.ones((ln, ln), dtype=bool))[:, None, :]
    share, cnt = keep[vis].mean(), int(vis.sum())
    assert abs(share - (1 - p)) <= 4 * (p * (1 - p) / cnt) ** 0.5, (share, cnt)
    # ... and measured on the kernel: v = 1 in one column makes out the row sum of dropout(P) there; with dO = 0 elsewhere,
    # dv of that column is the column sum of dropout(P): both follow the mask exactly
    q, k = (torch.from_numpy(t).to(torch.bfloat16).to(DEV) for t in x[:2])
    ones = torch.ones((L, H, 16), dtype=torch.bfloat16, device=DEV)
    out, _ = _launch.softmax_attn_fwd(q, k, ones, _offsets(lengths), n, 16 ** -0.5, p, seed)
    one = R.restate(x[0], x[1], np.ones_like(x[2]), x[3], lengths, keep=keep, keep_scale=ks)["out"]
    assert np.abs(out.double().cpu().numpy() - one).max() <= 2e-2 * np.abs(one).max()
    # another seed, another mask
    other = _run(_ops()[0], *x, lengths, n, torch.bfloat16, dropout_pr=p, seed=seed + 1)
    assert not np.array_equal(other["out"], got["out"])


def test_eval_mode_equals_no_dropout_bit_for_bit(drawn):
    x, lengths, n = drawn["x"], drawn["lengths"], drawn["n"]
    a = _run(_ops()[0], *x, lengths, n, torch.bfloat16, dropout_pr=0.5, training=False, seed=3)
    b = _run(_ops()[0], *x, lengths, n, torch.bfloat16, dropout_pr=0.0)
    for g in R.GRADS:
        assert np.array_equal(a[g], b[g]), g


def test_two_backward_calls_are_bit_identical(op_cases):
    c = op_cases["op_3_h4_d64_n130"]
    args = (c["q"], c["k"], c["v"], c["dout"], c["lengths"], c["max_seq_len"], torch.bfloat16)
    a = _run(_ops()[0], *args, dropout_pr=0.2, seed=11)
    b = _run(_ops()[0], *args, dropout_pr=0.2, seed=11)
    for g in R.GRADS:
        assert np.array_equal(a[g], b[g]), g


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_column_slices_of_wider_buffers_give_the_bits_of_contiguous_copies(op_cases, idx_dtype):
    c = op_cases["op_3_h4_d64_n130"]
    fused = _ops()[0]
    L, H, d = c["q"].shape
    n, off = c["max_seq_len"], _offsets(c["lengths"], idx_dtype)
    t = lambda a: torch.from_numpy(a).to(torch.bfloat16).to(DEV)
    qbuf = torch.cat([torch.full((L, 8), 7.0, dtype=torch.bfloat16, device=DEV), t(c["q"]).reshape(L, H * d)], dim=1)
    kvbuf = torch.cat([t(c["k"]).reshape(L, H * d), t(c["v"]).reshape(L, H * d)], dim=1)
    dout = t(c["dout"])
    res = []
    for strided in (True, False):
        qb, kvb = qbuf.clone().requires_grad_(True), kvbuf.clone().requires_grad_(True)
        q, k, v = qb[:, 8:].view(L, H, d), kvb[:, : H * d].view(L, H, d), kvb[:, H * d:].view(L, H, d)
        if strided:
            assert not k.is_contiguous() and not v.is_contiguous() and not q.is_contiguous()
        else:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out = fused(n, q, k, v, off)
        out.backward(dout)
        res.append((out.detach(), qb.grad, kvb.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_empty_inputs_give_empty_outputs_and_zero_gradients():
    fused, composed = _ops()
    for fn in (fused, composed):
        # L = 0 with users, and an all-empty batch
        for lengths in ([0, 0, 0], []):
            q, k, v = (torch.zeros((0, 2, 16), dtype=torch.bfloat16, device=DEV, requires_grad=True) for _ in range(3))
            out = fn(70, q, k, v, _offsets(lengths), dropout_pr=0.2, seed=1)
            assert out.shape == (0, 2, 16)
            out.sum().backward()
            assert all(t.grad is not None and t.grad.shape == (0, 2, 16) for t in (q, k, v))
    # empty users between full ones leave their neighbours alone
    g = np.random.default_rng(3)
    x = [R.round_to(g.standard_normal((40, 2, 16)), torch.bfloat16) for _ in range(4)]
    a = _run(fused, *x, [0, 33, 0, 0, 7, 0], 70, torch.bfloat16)
    b = _run(fused, *x, [33, 7], 70, torch.bfloat16)
    for gname in R.GRADS:
        assert np.array_equal(a[gname], b[gname]), gname


@pytest.mark.parametrize("shape", [(600, 2, 16, [600, 130, 1, 0, 33]), (130, 1, 80, [130, 96, 2])], ids=["n600", "d80"])
def test_outside_the_fused_range_the_composition_runs_and_passes_the_gate(shape):
    n, H, d, lengths = shape
    assert not _supported(torch.bfloat16, d, n)
    g = np.random.default_rng(n + d)
    x = [R.round_to(g.standard_normal((sum(lengths), H, d)), torch.bfloat16) for _ in range(4)]
    truth = R.restate(*x, lengths)
    ref = R.math_path(*x, lengths, n, torch.bfloat16)
    got = _run(_ops()[0], *x, lengths, n, torch.bfloat16)
    assert not R.gate(f"outside {shape[:3]}", got, ref, truth, "bfloat16")


# --------------------------------------------------------------------------------------------------------------- the module
def _model_from(c, dtype, **kw):
    D, H, blocks, hidden, n = (int(x) for x in c["config"])
    model, pre = build_model(D, H, blocks, str(c["activation"]), hidden, n, **kw)
    sd = model.state_dict()
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(c["sd:" + k])).to(sd[k].dtype) for k in sd}, strict=True)
    model = model.to(DEV).to(dtype)
    pre.emb = torch.from_numpy(np.ascontiguousarray(c["emb"])).to(dtype).to(DEV).requires_grad_(True)
    lens = torch.from_numpy(c["lengths"]).to(DEV)
    return model, pre, lens


@pytest.mark.parametrize("tag", ["bf16", "f32"])
@pytest.mark.parametrize("name", MODEL_CASES)
def test_module_against_the_fixtures(name, tag):
    c = R.load_model_case(name)
    dtype = R.TORCH_DTYPE[tag]
    model, pre, lens = _model_from(c, dtype)
    out = model(lens, None, None, {})
    (out * torch.from_numpy(np.ascontiguousarray(c["r"])).to(dtype).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = {"out": out.detach(), "g:emb": pre.emb.grad}
    got.update({"g:" + k: p.grad for k, p in model.named_parameters()})
    names = list(got)
    assert all(v is not None for v in got.values()) and len(names) == 2 + 8 * int(c["config"][2])
    got = {k: v.double().cpu().numpy() for k, v in got.items()}
    truth = {k: np.asarray(c["f64:" + k], dtype=np.float64) for k in names}
    ref = {k: np.asarray(c[f"{tag}:{k}"], dtype=np.float64) for k in names}
    mult = lambda tensor, n_el: R.model_multiplier(R.DTYPE_NAME[tag], tensor, n_el, c["bf16:relu_flips"])
    assert not R.gate(f"module {name}", got, ref, truth, R.DTYPE_NAME[tag], names=names, multiplier=mult)
    # padded rows of the output are exactly zero, and encode is the last valid row of forward
    n = out.shape[1]
    pad = torch.arange(n, device=DEV).view(1, -1) >= lens.view(-1, 1)
    assert float(out.detach()[pad].abs().max()) == 0.0
    with torch.no_grad():
        nz = lens > 0
        enc = model.encode(lens, None, None, {})
        assert torch.equal(enc[nz], out.detach()[nz, lens[nz] - 1])


def test_training_mode_is_finite_reproducible_and_checkpointing_keeps_the_bits():
    c = R.load_model_case(MODEL_CASES[0])
    r = torch.from_numpy(np.ascontiguousarray(c["r"])).to(torch.bfloat16).to(DEV)
    runs = []
    for ckpt in (False, False, True):
        model, pre, lens = _model_from(c, torch.bfloat16, ffn_dropout_rate=0.2, activation_checkpoint=ckpt)
        model.train()
        torch.manual_seed(77)
        out = model(lens, None, None, {})
        (out * r).sum().backward()
        torch.cuda.synchronize()
        res = [out.detach(), pre.emb.grad] + [p.grad for p in model.parameters()]
        assert all(torch.isfinite(t).all() for t in res)
        runs.append(res)
    for a, b, ck in zip(*runs):
        assert torch.equal(a, b) and torch.equal(a, ck)
    model, pre, lens = _model_from(c, torch.bfloat16, ffn_dropout_rate=0.2)
    model.eval()
    with torch.no_grad():
        assert not torch.equal(model(lens, None, None, {}), runs[0][0])          # dropout did act in training mode
