"""GPU tests of the in-backward sparse Adam and SGD (csrc/embedding_optim.hip, ops/embedding.py, the fused mode of
EmbeddingCollection / DlrmHSTU) against the fp64 formulas of embedding_sparse_optim_ref.py.  Tolerances are that helper's
per-element first-order bounds of an fp32 evaluation in any summation order, computed from the inputs; rows outside the batch
must keep their bits in the weight and in every state tensor (compared on the device).  lr, betas and eps are fp32-representable
numbers: the kernels take them as fp32 and the reference takes inputs as the exact values they hold."""

import numpy as np
import pytest
import torch

import dlrm_hstu_ref as R
import embedding_lowp_ref as LR16
import embedding_sparse_optim_ref as SR
from conftest import record_parity
from test_embedding_replicated_gpu import PRELUDE, _run_workers

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, LR_SGD, BETAS, EPS, STEP = SR.f32(1e-3), SR.f32(0.05), (SR.f32(0.95), SR.f32(0.999)), SR.f32(1e-8), 6
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SEED = 0x1234_5678_9ABC_DEF0


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _run_adam(w0, m0, v0, idx, dout, tag, eps=EPS, step=STEP, wdtype=None, seed=None):
    from generative_recommenders_amd.ops.embedding import sparse_adam_update_

    w, m, v, i, d = _dev(w0, m0, v0, idx, dout)
    if wdtype is not None:
        w = w.to(wdtype)
    sparse_adam_update_(w, m, v, i, d.to(DT[tag]), LR, BETAS, eps, step, seed=seed)
    torch.cuda.synchronize()
    return w, m, v


def _run_sgd(w0, idx, dout, tag, wdtype=None, seed=None):
    from generative_recommenders_amd.ops.embedding import sparse_sgd_update_

    w, i, d = _dev(w0, idx, dout)
    if wdtype is not None:
        w = w.to(wdtype)
    sparse_sgd_update_(w, i, d.to(DT[tag]), LR_SGD, seed=seed)
    torch.cuda.synchronize()
    return w


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _untouched_rows_keep_their_bits(what, rows, before, after):
    """on the device: every row outside ``rows`` of every tensor, bit for bit"""
    keep = torch.ones(after[0].shape[0], dtype=torch.bool, device=DEV)
    keep[torch.from_numpy(rows).to(DEV)] = False
    for name, b, a in zip(("weight", "exp_avg", "exp_avg_sq"), before, after):
        b = b if torch.is_tensor(b) else torch.from_numpy(b)
        assert torch.equal(_bits(a)[keep], _bits(b.to(DEV))[keep]), f"{what}: an untouched {name} row changed"


def _within(what, got, ref, keys):
    """touched rows finite and within the bounds; -> the worst error over its bound per key"""
    rows, out = ref["rows"], {}
    for key, t in zip(keys, got):
        g = t[torch.from_numpy(rows).to(DEV)].float().cpu().numpy()
        err = np.abs(g.astype(np.float64) - ref[key][rows])
        out[key] = SR.worst(err, ref["tol_" + key])
        record_parity(f"{what} {key}", g, ref[key][rows], worst_over_bound=out[key])
        assert np.isfinite(g).all() and (err <= ref["tol_" + key]).all(), f"{what}: {key} err/bound {out[key]:.3f}"
    print(f"{what}: " + ", ".join(f"{k} err/bound {o:.3f}" for k, o in out.items()))
    return out


def _check_adam(what, w0, m0, v0, idx, dout, got, eps=EPS, step=STEP, lr=LR):
    ref = SR.sparse_adam_ref(w0, m0, v0, idx, dout, lr, BETAS, eps, step)
    out = _within(what, got, ref, ("weight", "exp_avg", "exp_avg_sq"))
    _untouched_rows_keep_their_bits(what, ref["rows"], (w0, m0, v0), got)
    return out


def _check_sgd(what, w0, idx, dout, w):
    ref = SR.sparse_sgd_ref(w0, idx, dout, LR_SGD)
    _within(what, (w,), ref, ("weight",))
    _untouched_rows_keep_their_bits(what, ref["rows"], (w0,), (w,))


@pytest.mark.parametrize("n,dim,rows,kind,tag", SR.CASES)
def test_adam_against_the_formula_untouched_rows_and_determinism(n, dim, rows, kind, tag):
    idx, dout, w0, m0, v0 = SR.make_problem(n, dim, rows, kind, tag)
    if kind != "equal":
        assert 0 in idx and rows - 1 in idx
    got = _run_adam(w0, m0, v0, idx, dout, tag)
    _check_adam(f"adam n{n} d{dim} rows{rows} {kind} {tag}", w0, m0, v0, idx, dout, got)
    again = _run_adam(w0, m0, v0, idx, dout, tag)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again)), "two runs of the same batch differ"


@pytest.mark.parametrize("n,dim,rows,kind,tag", SR.CASES)
def test_sgd_against_the_formula_untouched_rows_and_determinism(n, dim, rows, kind, tag):
    idx, dout, w0, _, _ = SR.make_problem(n, dim, rows, kind, tag)
    w = _run_sgd(w0, idx, dout, tag)
    _check_sgd(f"sgd n{n} d{dim} rows{rows} {kind} {tag}", w0, idx, dout, w)
    assert torch.equal(_bits(w), _bits(_run_sgd(w0, idx, dout, tag))), "two runs of the same batch differ"


@pytest.mark.parametrize("n,dim,rows,kind,zero_state,step", SR.EPS_CASES)
def test_adam_where_the_place_of_eps_matters(n, dim, rows, kind, zero_state, step):
    """eps = 1e-2: the bounds reject SparseAdam's placement, eps under the square root and a missing bias correction by more
    than 100 x at these two cases (test_embedding_sparse_optim_host.py)"""
    eps = SR.f32(1e-2)
    idx, dout, w0, m0, v0 = SR.make_problem(n, dim, rows, kind, "bf16", zero_state)
    got = _run_adam(w0, m0, v0, idx, dout, "bf16", eps=eps, step=step)
    _check_adam(f"adam eps 1e-2 n{n} d{dim} rows{rows} t{step + 1}", w0, m0, v0, idx, dout, got, eps=eps, step=step)


@pytest.mark.parametrize("tag", ["bf16", "f32"])
def test_hot_id_with_thousands_of_duplicates(tag):
    """5,000 duplicates of one id among 8,192: a segment cut by some 160 chunk boundaries, summed by the combine kernel"""
    rng = np.random.default_rng(7)
    rows, dim, n = 20_011, 256, 8192
    idx = rng.integers(0, rows, n)
    idx[rng.permutation(n)[:5000]] = 13_337
    assert int((idx == 13_337).sum()) >= 5000
    dout = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32)).to(DT[tag]).float().numpy()
    w0, m0, v0 = SR.make_state(rows, dim, rng)
    got = _run_adam(w0, m0, v0, idx, dout, tag)
    _check_adam(f"adam hot id {tag}", w0, m0, v0, idx, dout, got)
    again = _run_adam(w0, m0, v0, idx, dout, tag)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    _check_sgd(f"sgd hot id {tag}", w0, idx, dout, _run_sgd(w0, idx, dout, tag))


def test_two_consecutive_steps_carry_the_moments_and_the_step():
    from generative_recommenders_amd.ops.embedding import sparse_adam_update_

    rng = np.random.default_rng(11)
    rows, dim, n = 1000, 64, 300
    w0, _, _ = SR.make_state(rows, dim, rng)
    z = np.zeros((rows, dim), dtype=np.float32)
    idx1, idx2 = rng.integers(0, 200, n), rng.integers(100, 300, n)           # overlap on [100, 200)
    d1, d2 = (torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32)).bfloat16() for _ in range(2))
    w, m, v = _dev(w0, z, z)
    sparse_adam_update_(w, m, v, *_dev(idx1), d1.to(DEV), LR, BETAS, EPS, 0)
    torch.cuda.synchronize()
    mid = [t.clone() for t in (w, m, v)]
    _check_adam("adam step 1 of 2", w0, z, z, idx1, d1.float().numpy(), mid, step=0)
    sparse_adam_update_(w, m, v, *_dev(idx2), d2.to(DEV), LR, BETAS, EPS, 1)
    torch.cuda.synchronize()
    # the second step from the state the first one left, with t = 2: its own bound holds for that step
    w1, m1, v1 = (t.cpu().numpy() for t in mid)
    _check_adam("adam step 2 of 2", w1, m1, v1, idx2, d2.float().numpy(), (w, m, v), step=1)
    # ... and the two steps together against the formula applied twice in fp64, the two steps' bounds added.  First-step errors
    # pass through the second step (first order, doubled): dW2/dW1 = 1, dm2/dm1 = b1, dv2/dv1 = b2, and with upd = a m / den,
    # den = sqrt(v) / sqrt(bc2) + eps:  |d upd / dm| = a / den,  |d upd / d sqrt(v)| = a |m| / (sqrt(bc2) den^2), |d sqrt(v)| <= dv / (2 sqrt(v))
    r1 = SR.sparse_adam_ref(w0, z, z, idx1, d1.float().numpy(), LR, BETAS, EPS, 0)
    r2 = SR.sparse_adam_ref(r1["weight"], r1["exp_avg"], r1["exp_avg_sq"], idx2, d2.float().numpy(), LR, BETAS, EPS, 1)
    tol = {k: np.zeros((rows, dim)) for k in ("weight", "exp_avg", "exp_avg_sq")}
    for k in tol:
        tol[k][r1["rows"]] = r1["tol_" + k]
    rows2 = r2["rows"]
    b1, b2 = BETAS
    a, bc2 = LR / (1 - b1 ** 2), 1 - b2 ** 2
    m2, v2 = r2["exp_avg"][rows2], r2["exp_avg_sq"][rows2]
    den = np.sqrt(v2) / np.sqrt(bc2) + EPS
    tm, tv = b1 * tol["exp_avg"][rows2], b2 * tol["exp_avg_sq"][rows2]
    with np.errstate(divide="ignore", invalid="ignore"):                    # v2 = 0 (duplicates that cancel): |d sqrt(v)| <= sqrt(tv)
        tsq = np.where(v2 > 0, np.minimum(tv / (2 * np.sqrt(v2)), np.sqrt(tv)), np.sqrt(tv))
    tol["weight"][rows2] += 2 * a * (tm / den + np.abs(m2) * tsq / (np.sqrt(bc2) * den * den)) + r2["tol_weight"]
    tol["exp_avg"][rows2] = 2 * tm + r2["tol_exp_avg"]
    tol["exp_avg_sq"][rows2] = 2 * tv + r2["tol_exp_avg_sq"]
    touched = np.union1d(r1["rows"], rows2)
    for k, t in zip(("weight", "exp_avg", "exp_avg_sq"), (w, m, v)):
        err = np.abs(t.cpu().numpy().astype(np.float64) - r2[k])[touched]
        over = SR.worst(err, tol[k][touched])
        record_parity(f"adam two steps {k}", t.cpu().numpy()[touched], r2[k][touched], worst_over_bound=over)
        assert (err <= tol[k][touched]).all(), (k, over)
    # t = 1 on the second step is far outside: its step size is 1.95 times the right one
    wrong = SR.sparse_adam_ref(r1["weight"], r1["exp_avg"], r1["exp_avg_sq"], idx2, d2.float().numpy(), LR, BETAS, EPS, 0)
    assert SR.worst(np.abs(wrong["weight"][rows2] - r2["weight"][rows2]), tol["weight"][rows2]) > 100


def test_an_empty_batch_changes_nothing_and_does_not_count():
    from generative_recommenders_amd.modules.dlrm_hstu import EmbeddingCollection, EmbeddingConfig, KeyedJaggedTensor

    rng = np.random.default_rng(3)
    w0, m0, v0 = SR.make_state(33, 64, rng)
    none, nothing = np.zeros(0, dtype=np.int64), np.zeros((0, 64), dtype=np.float32)
    got = _run_adam(w0, m0, v0, none, nothing, "bf16")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, _dev(w0, m0, v0)))
    assert torch.equal(_bits(_run_sgd(w0, none, nothing, "bf16")), _bits(_dev(w0)[0]))
    ec = EmbeddingCollection([EmbeddingConfig(33, 64, "t", ["c"]), EmbeddingConfig(33, 64, "h", ["d"], data_type="FP16")]).to(DEV)
    ec.apply_optimizer_in_backward("Adam", LR, betas=BETAS, eps=EPS)
    before = {k: t.clone() for k, t in ec.fused_optimizer_state_dict().items()}
    weights = {t: e.weight.detach().clone() for t, e in ec.embeddings.items()}
    out = ec(KeyedJaggedTensor(["c", "d"], torch.zeros(0, dtype=torch.int64, device=DEV), torch.tensor([0, 0], device=DEV)))
    (out["c"].values().sum() + out["d"].values().float().sum()).backward()
    torch.cuda.synchronize()
    after = ec.fused_optimizer_state_dict()
    assert sorted(after) == ["h.exp_avg", "h.exp_avg_sq", "h.step", "t.exp_avg", "t.exp_avg_sq", "t.step"]
    assert all(torch.equal(after[k], before[k]) for k in before) and int(after["t.step"]) == int(after["h.step"]) == 0
    assert all(torch.equal(_bits(e.weight.detach()), _bits(weights[t])) for t, e in ec.embeddings.items())
    out = ec(KeyedJaggedTensor(["c", "d"], torch.tensor([4, 4, 7], device=DEV), torch.tensor([1, 2], device=DEV)))
    (out["c"].values().sum() + out["d"].values().float().sum()).backward()
    assert int(after["t.step"]) == int(after["h.step"]) == 1


LOWP_CASES = [(65, 256, 8193, "zipf", "bf16"), (257, 8, 2, "zipf", "f16"), (257, 64, 8193, "equal", "f32"), (257, 2048, 2, "zipf", "f16")]


@pytest.mark.parametrize("wtag", ["f16", "bf16"])
@pytest.mark.parametrize("n,dim,rows,kind,tag", LOWP_CASES)
def test_16_bit_tables_round_the_fp32_tables_row_and_share_its_moments(n, dim, rows, kind, tag, wtag):
    """the 16-bit table's result is the fp32-table kernel's row (from the same values held in fp32) rounded by the numpy
    restatement of the rule, bit for bit; exp_avg and exp_avg_sq are the fp32 table's, bit for bit"""
    idx, dout, w0, m0, v0 = SR.make_problem(n, dim, rows, kind, tag)
    w16 = torch.from_numpy(w0).to(DT[wtag])
    held = w16.float().numpy()                                              # the same values in fp32
    touched = np.unique(idx)
    sel = torch.from_numpy(touched).to(DEV)
    w32, m32, v32 = _run_adam(held, m0, v0, idx, dout, tag)
    wl, ml, vl = _run_adam(held, m0, v0, idx, dout, tag, wdtype=DT[wtag], seed=SEED)
    want = LR16.stochastic_round(w32[sel].cpu().numpy(), wtag, SEED, row_ids=touched)
    assert np.array_equal(_bits(wl[sel]).cpu().numpy().view(np.uint16), want), "adam: not the rounded fp32 row"
    assert torch.equal(_bits(ml), _bits(m32)) and torch.equal(_bits(vl), _bits(v32)), "adam: the moments differ from the fp32 table's"
    _untouched_rows_keep_their_bits(f"adam {wtag} table", touched, (w16,), (wl,))
    s32 = _run_sgd(held, idx, dout, tag)
    sl = _run_sgd(held, idx, dout, tag, wdtype=DT[wtag], seed=SEED)
    want = LR16.stochastic_round(s32[sel].cpu().numpy(), wtag, SEED, row_ids=touched)
    assert np.array_equal(_bits(sl[sel]).cpu().numpy().view(np.uint16), want), "sgd: not the rounded fp32 row"
    _untouched_rows_keep_their_bits(f"sgd {wtag} table", touched, (w16,), (sl,))
    # the fp32 rows themselves are held to the formula
    _check_adam(f"adam fp32 twin of the {wtag} table n{n} d{dim}", held, m0, v0, idx, dout, (w32, m32, v32))


@pytest.mark.parametrize("wtag", ["f32", "bf16"])
def test_coalesced_fp32_list_at_8_kib_rows_equals_the_one_shot_update(wtag):
    """what replicated tables rest on: coalescing 16-bit rows and applying the fp32 list (dim 2048: 8 KiB rows, through the same
    entry) gives the bits of the one-shot update on the 16-bit rows -- and a list with duplicate ids (two ranks' lists, one
    after the other) stays within the formula's bounds"""
    from generative_recommenders_amd.ops.embedding import coalesce_row_gradients, sparse_adam_update_, sparse_sgd_update_

    rng = np.random.default_rng(21)
    rows, dim, n = 301, 2048, 200
    idx = rng.integers(0, 40, n) * 7
    dout = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32)).bfloat16()
    w0, m0, v0 = SR.make_state(rows, dim, rng)
    wdtype, seed = (None, None) if wtag == "f32" else (DT[wtag], SEED)
    one = _run_adam(w0, m0, v0, idx, dout.float().numpy(), "bf16", wdtype=wdtype, seed=seed)
    ids, G, count = coalesce_row_gradients(*_dev(idx), dout.to(DEV), rows)
    c = int(count)
    assert c == len(np.unique(idx)) and G.dtype == torch.float32
    w, m, v = _dev(w0, m0, v0)
    w = w if wdtype is None else w.to(wdtype)
    sparse_adam_update_(w, m, v, ids[:c], G[:c], LR, BETAS, EPS, STEP, seed=seed)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(one, (w, m, v))), "adam: coalesce + apply differs from the one-shot update"
    s_one = _run_sgd(w0, idx, dout.float().numpy(), "bf16", wdtype=wdtype, seed=seed)
    s = _dev(w0)[0] if wdtype is None else _dev(w0)[0].to(wdtype)
    sparse_sgd_update_(s, ids[:c], G[:c], LR_SGD, seed=seed)
    assert torch.equal(_bits(s), _bits(s_one)), "sgd: coalesce + apply differs from the one-shot update"
    if wtag == "f32":
        half = n // 2
        a, b = (coalesce_row_gradients(*_dev(idx[s_]), dout[s_].to(DEV), rows) for s_ in (slice(0, half), slice(half, n)))
        ids2 = torch.cat([a[0][:int(a[2])], b[0][:int(b[2])]])
        G2 = torch.cat([a[1][:int(a[2])], b[1][:int(b[2])]])
        assert ids2.numel() > c                                              # ids that both halves hold occur twice
        w, m, v = _dev(w0, m0, v0)
        sparse_adam_update_(w, m, v, ids2, G2, LR, BETAS, EPS, STEP)
        torch.cuda.synchronize()
        _check_adam("adam two coalesced lists d2048", w0, m0, v0, idx, dout.float().numpy(), (w, m, v))


def _three_feature_collection(item_dtype="FP32"):
    from generative_recommenders_amd.modules.dlrm_hstu import EmbeddingCollection, EmbeddingConfig, KeyedJaggedTensor

    torch.manual_seed(5)
    ec = EmbeddingCollection([EmbeddingConfig(500, 64, "item", ["a", "b"], data_type=item_dtype), EmbeddingConfig(300, 64, "user", ["c"])]).to(DEV)
    g = torch.Generator().manual_seed(17)
    ids = {"a": torch.randint(0, 40, (70,), generator=g), "b": torch.randint(20, 60, (50,), generator=g),      # overlap on [20, 40)
           "c": torch.randint(0, 300, (30,), generator=g)}
    feats = KeyedJaggedTensor(["a", "b", "c"], torch.cat([ids[k] for k in "abc"]).to(DEV), torch.tensor([70, 50, 30], device=DEV))
    return ec, ids, feats, g


def test_embedding_collection_adam_and_sgd_tables_one_update_per_table():
    ec, ids, feats, g = _three_feature_collection()
    douts = {k: torch.randn(v.numel(), 64, generator=g).bfloat16() for k, v in ids.items()}
    w0 = {t: e.weight.detach().cpu().numpy().copy() for t, e in ec.embeddings.items()}
    ec.apply_optimizer_in_backward("Adam", LR, betas=BETAS, eps=EPS, rows_dtype=torch.bfloat16, tables=["item"])
    ec.apply_optimizer_in_backward("SGD", LR_SGD, rows_dtype=torch.bfloat16, tables=["user"])
    out = ec(feats)
    assert list(out) == ["a", "b", "c"] and all(out[k].values().dtype == torch.bfloat16 for k in "abc")
    sum((out[k].values() * douts[k].to(DEV)).sum() for k in "abc").backward()
    torch.cuda.synchronize()
    assert all(e.weight.grad is None and e.weight.requires_grad and e.weight.dtype == torch.float32 for e in ec.embeddings.values())
    state = ec.fused_optimizer_state_dict()
    assert sorted(state) == ["item.exp_avg", "item.exp_avg_sq", "item.step"] and int(state["item.step"]) == 1
    z = np.zeros((500, 64), dtype=np.float32)
    idx_item = torch.cat([ids["a"], ids["b"]]).numpy()
    d_item = torch.cat([douts["a"], douts["b"]]).float().numpy()
    got = (ec.embeddings["item"].weight.detach(), state["item.exp_avg"], state["item.exp_avg_sq"])
    _check_adam("collection item (adam)", w0["item"], z, z, idx_item, d_item, got, step=0)
    _check_sgd("collection user (sgd)", w0["user"], ids["c"].numpy(), douts["c"].float().numpy(), ec.embeddings["user"].weight.detach())
    # Adam applied per feature is a different result on the rows both features hold: far outside the bound
    one = SR.sparse_adam_ref(w0["item"], z, z, idx_item, d_item, LR, BETAS, EPS, 0)
    s1 = SR.sparse_adam_ref(w0["item"], z, z, ids["a"].numpy(), douts["a"].float().numpy(), LR, BETAS, EPS, 0)
    s2 = SR.sparse_adam_ref(s1["weight"], s1["exp_avg"], s1["exp_avg_sq"], ids["b"].numpy(), douts["b"].float().numpy(), LR, BETAS, EPS, 1)
    shared = np.intersect1d(ids["a"].numpy(), ids["b"].numpy())
    assert shared.size > 0
    gap = np.abs(got[0].cpu().numpy().astype(np.float64)[shared] - s2["weight"][shared])
    assert (gap.max(axis=1) > 100 * one["tol_weight"][np.searchsorted(one["rows"], shared)].max(axis=1)).all()
    ec.set_learning_rate(0.0)                        # reaches both configs: a later step moves no weight (Adam's moments do move)
    before = {t: e.weight.detach().clone() for t, e in ec.embeddings.items()}
    out = ec(feats)
    (out["a"].values().float().sum() + out["c"].values().float().sum()).backward()
    assert all(torch.equal(before[t], e.weight.detach()) for t, e in ec.embeddings.items()) and int(state["item.step"]) == 2


def test_save_load_continue_equals_an_uninterrupted_run():
    """three steps, the state saved after the first and loaded into a fresh collection: an fp16 Adam table (whose rounding seed
    comes from Adam's step) and an fp32 SGD table end bit-identical to the uninterrupted run"""
    def fresh():
        ec, ids, feats, g = _three_feature_collection("FP16")
        ec.apply_optimizer_in_backward("Adam", LR, betas=BETAS, eps=EPS, tables=["item"], seed=9)
        ec.apply_optimizer_in_backward("SGD", LR_SGD, tables=["user"])
        return ec, feats

    def steps(ec, feats, which):
        for s in which:
            g = torch.Generator().manual_seed(100 + s)
            out = ec(feats)
            sum((out[k].values().float() * torch.randn(out[k].values().shape, generator=g).to(DEV)).sum() for k in "abc").backward()
        torch.cuda.synchronize()

    a, feats = fresh()
    steps(a, feats, range(3))
    b, _ = fresh()
    steps(b, feats, range(1))
    saved = ({k: v.clone() for k, v in b.state_dict().items()}, {k: v.clone() for k, v in b.fused_optimizer_state_dict().items()})
    assert sorted(saved[1]) == ["item.exp_avg", "item.exp_avg_sq", "item.step"] and int(saved[1]["item.step"]) == 1
    c, _ = fresh()
    c.load_state_dict(saved[0])
    c.load_fused_optimizer_state_dict(saved[1])
    steps(c, feats, range(1, 3))
    assert c.embeddings["item"].weight.dtype == torch.float16 and int(c.fused_optimizer_state_dict()["item.step"]) == 3
    for t in ("item", "user"):
        assert torch.equal(_bits(a.embeddings[t].weight.detach()), _bits(c.embeddings[t].weight.detach())), t
    sa, sc = a.fused_optimizer_state_dict(), c.fused_optimizer_state_dict()
    assert all(torch.equal(sa[k], sc[k]) for k in sa)
    assert not torch.equal(a.embeddings["item"].weight.detach(), b.embeddings["item"].weight.detach())


def test_dlrm_hstu_adam_tables_match_the_formula_on_the_unfused_gradients(monkeypatch):
    """Copy A (unfused) gives the table gradients; the fp64 formula on them gives the expected tables and moments.  Copy B (Adam
    in backward) must match them within the helper's bounds, with every other gradient and every output bit-identical to A's.
    The bounds need the duplicates (k and A = sum |dout_i|), which the table gradient no longer shows: hooks on copy A's gathered
    rows record the gradient rows per feature.  The bound's summation term 2k u A is twice the first-order (k - 1) u A of one fp32
    sum, which leaves room for copy A's own fp32 segment sum next to the kernel's."""
    from generative_recommenders_amd.modules.dlrm_hstu import apply_optimizer_in_backward
    from generative_recommenders_amd.ops import position

    monkeypatch.setattr(position, "TIME_BUCKET_CLAMP", "pytorch_path")
    inputs = R.load("model_small")
    names = [n for n, _, _ in R.TASKS]
    row_grads = {}

    def record_row_grads(module, args, out):
        for key, jt in out.items():
            jt.values().register_hook(lambda grad, key=key: row_grads.__setitem__(key, grad.detach().cpu()))

    def step(fused):
        m = R.build(False, inputs).to(DEV)
        m.set_training_dtype(torch.float32)
        if fused:
            apply_optimizer_in_backward(m, "Adam", LR, betas=BETAS, eps=EPS)
        else:
            m._embedding_collection.register_forward_hook(record_row_grads)
        tables0 = {t: e.weight.detach().cpu().clone() for t, e in m._embedding_collection.embeddings.items()}
        out = m(*R.features(inputs, DEV))
        torch.stack([out[2][n] for n in names]).sum().backward()
        torch.cuda.synchronize()
        return m, out, tables0

    a, out_a, tables0 = step(False)
    b, out_b, _ = step(True)
    flat = lambda o: list(o[:2]) + [o[2][n] for n in names] + list(o[3:])
    for x, y in zip(flat(out_a), flat(out_b)):
        assert (x is None and y is None) or torch.equal(x, y), "the fused model's outputs differ"
    params_b = dict(b.named_parameters())
    state = b._embedding_collection.fused_optimizer_state_dict()
    uih, cand = R.features(inputs, "cpu")
    seen_tables = 0
    for name, p in a.named_parameters():
        if not name.startswith("_embedding_collection."):
            assert (p.grad is None) == (params_b[name].grad is None), name
            if p.grad is not None:
                assert torch.equal(p.grad, params_b[name].grad), f"the gradient of {name} differs"
            continue
        table = name.split(".")[2]
        seen_tables += 1
        assert params_b[name].grad is None and int(state[table + ".step"]) == 1
        w0, ga = tables0[table].numpy(), p.grad.detach().cpu()
        z = np.zeros_like(w0)
        rows = torch.nonzero(ga.abs().sum(dim=1) > 0).flatten()
        want = SR.sparse_adam_ref(w0, z, z, rows.numpy(), ga[rows].numpy(), LR, BETAS, EPS, 0)
        keys = [k for k in uih.keys() + cand.keys() if k in R.tables()[table].feature_names]
        ids = torch.cat([(uih if k in uih.keys() else cand)[k].values() for k in keys])
        bound = SR.sparse_adam_ref(w0, z, z, ids.numpy(), torch.cat([row_grads[k] for k in keys]).numpy(), LR, BETAS, EPS, 0)
        touched = bound["rows"]
        assert set(rows.tolist()) <= set(touched.tolist())
        got = {"weight": params_b[name].detach().cpu().numpy(), "exp_avg": state[table + ".exp_avg"].cpu().numpy(),
               "exp_avg_sq": state[table + ".exp_avg_sq"].cpu().numpy()}
        for key, arr in got.items():
            err = np.abs(arr[touched].astype(np.float64) - want[key][touched])
            over = SR.worst(err, bound["tol_" + key])
            record_parity(f"dlrm adam table {table} {key}", arr[touched], want[key][touched], worst_over_bound=over)
            print(f"dlrm adam table {table}: {key} err/bound {over:.3f}")
            assert (err <= bound["tol_" + key]).all(), (table, key, over)
        keep = np.ones(w0.shape[0], dtype=bool)
        keep[touched] = False
        assert np.array_equal(got["weight"][keep], w0[keep]) and not got["exp_avg"][keep].any() and not got["exp_avg_sq"][keep].any()
    assert seen_tables == 2


# ---- replicated: world 2 over gloo, both ranks on device 0, different shards, one empty shard; Adam on an fp32 and an fp16 table
WORKER_ADAM = PRELUDE + r'''
import embedding_lowp_ref as LR16
import embedding_sparse_optim_ref as SR
ROWS, DIM, STEPS = 200, 64, 3
LR, BETAS, EPS = SR.f32(1e-3), (SR.f32(0.95), SR.f32(0.999)), SR.f32(1e-8)

def shard(step, rank):
    g = torch.Generator().manual_seed(1000 * step + rank)
    n = 0 if (step == 1 and rank == 1) else 90 + 40 * rank + 7 * step
    return torch.randint(0, 60 + 30 * rank, (n,), generator=g), torch.randn(n, DIM, generator=g)

torch.manual_seed(5)
ec = EmbeddingCollection([EmbeddingConfig(ROWS, DIM, "t", ["c"]), EmbeddingConfig(ROWS, DIM, "h", ["d"], data_type="FP16")]).to(DEV)
ec.apply_optimizer_in_backward("Adam", LR, betas=BETAS, eps=EPS, replicated=True, seed=3)
if RANK == 1:                                       # rank 1 starts from something else: step 0 is the broadcast
    with torch.no_grad():
        ec.embeddings["t"].weight.add_(1.0)
        ec.fused_optimizer_state_dict()["h.exp_avg"].fill_(0.5)
        ec.fused_optimizer_state_dict()["h.step"].fill_(4)
E.broadcast_fused_tables(ec, src=0)
E.assert_fused_tables_in_sync(ec)

def snapshot():
    st = ec.fused_optimizer_state_dict()
    return {t: tuple(x.detach().float().cpu().numpy().copy() for x in (ec.embeddings[t].weight, st[t + ".exp_avg"], st[t + ".exp_avg_sq"]))
            for t in "th"}

states = [snapshot()]
for s in range(STEPS):
    idx, dout = shard(s, RANK)
    n = torch.tensor([idx.numel()], device=DEV)
    out = ec(KeyedJaggedTensor(["c", "d"], torch.cat([idx, idx]).to(DEV), torch.cat([n, n])))
    out["c"].values().backward(dout.to(DEV))
    out["d"].values().backward(dout.to(DEV).half())
    torch.cuda.synchronize()
    states.append(snapshot())
E.assert_fused_tables_in_sync(ec)
st = ec.fused_optimizer_state_dict()
res = {"rank": RANK, "checksums": E.fused_tables_checksum(ec), "steps": [int(st["t.step"]), int(st["h.step"])], "worst": 0.0}
if RANK == 0:
    for s in range(STEPS):
        parts = [shard(s, r) for r in range(WORLD)]                 # rank order
        idx = torch.cat([p[0] for p in parts]).numpy()
        for t in "th":
            # averaged over the ranks: every row gradient times 1 / 2 (exact); the fp16 table's rows arrive as fp16 gradients
            dout = torch.cat([p[1] if t == "t" else p[1].half().float() for p in parts]).numpy() * (1.0 / WORLD)
            (w0, m0, v0), (w1, m1, v1) = states[s][t], states[s + 1][t]
            ref = SR.sparse_adam_ref(w0, m0, v0, idx, dout, LR, BETAS, EPS, s)
            rows = ref["rows"]
            for key, got in (("exp_avg", m1), ("exp_avg_sq", v1)) + ((("weight", w1),) if t == "t" else ()):
                err = np.abs(got[rows].astype(np.float64) - ref[key][rows])
                res["worst"] = max(res["worst"], SR.worst(err, ref["tol_" + key]))
                assert (err <= ref["tol_" + key]).all(), f"step {s} table {t} {key}"
            if t == "h":                            # stochastically rounded: a neighbour on the fp16 grid of a value within the bound
                lo = LR16.down16(ref["weight"][rows] - ref["tol_weight"], "f16")
                hi = LR16.up16(ref["weight"][rows] + ref["tol_weight"], "f16")
                assert ((w1[rows] >= lo) & (w1[rows] <= hi)).all(), f"step {s} table h weight"
            keep = np.ones(ROWS, dtype=bool)
            keep[rows] = False
            assert keep.any() and all(np.array_equal(x[keep], y[keep]) for x, y in zip(states[s][t], states[s + 1][t])), f"step {s}: untouched rows"
print("RESULT " + json.dumps(res))
dist.barrier()
dist.destroy_process_group()
'''


def test_replicated_adam_two_ranks_over_gloo_stay_in_sync_and_match_the_formula(tmp_path):
    r0, r1 = sorted(_run_workers(tmp_path, WORKER_ADAM, 2, "gloo", 240), key=lambda r: r["rank"])
    print(f"replicated adam over gloo: worst err/bound {r0['worst']:.3f}")
    assert r0["checksums"] == r1["checksums"] and sorted(r0["checksums"]) == ["h", "t"]
    assert r0["steps"] == r1["steps"] == [3, 3]      # every step's concatenated list is non-empty, the empty shard included
    assert 0 < r0["worst"] <= 1.0
