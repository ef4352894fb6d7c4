"""GPU tests of the in-backward sparse row-wise Adagrad (csrc/embedding_optim.hip, ops/embedding.py, the fused mode of
EmbeddingCollection / DlrmHSTU) against the fp64 formula of embedding_optim_ref.py.  Tolerances are that helper's
per-element first-order bounds of an fp32 evaluation in any summation order (constants doubled), computed from the inputs;
rows outside the batch must keep their bits."""

import numpy as np
import pytest
import torch

import dlrm_hstu_ref as R
import embedding_optim_ref as ER
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, EPS = 0.05, 1e-8
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _ids(kind, n, rows, g):
    """n ids in [0, rows); except when all are equal, id 0 and id rows - 1 occur whenever there is room for both"""
    if kind == "equal":
        return torch.full((n,), rows - 1, dtype=torch.int64)
    if kind == "distinct":
        assert 2 <= n <= rows
        inner = 1 + torch.randperm(rows - 2, generator=g)[:n - 2]
        return torch.cat([torch.tensor([0, rows - 1]), inner])[torch.randperm(n, generator=g)]
    # zipf: rank r with probability ~ 1 / (r + 1), the ranks scattered over the table
    p = 1.0 / torch.arange(1, rows + 1, dtype=torch.float64)
    idx = torch.randperm(rows, generator=g)[torch.multinomial(p, n, replacement=True, generator=g)]
    idx[0], idx[-1] = 0, rows - 1
    return idx


def _state(rows, dim, g):
    """random table, positive state, and a NaN-free sentinel pattern on every other row"""
    w = torch.randn(rows, dim, generator=g)
    m1 = torch.rand(rows, generator=g) * 0.1
    w[1::2] = torch.tensor(-12345.671875)
    m1[1::2] = 6789.0625
    return w, m1


def _worst(err, tol):
    """largest error over its bound (a bound of exactly 0 -- a zero gradient on zero state -- admits only an error of 0)"""
    live = tol > 0
    return float((err[live] / tol[live]).max()) if live.any() else 0.0


def _check(what, w0, m0, idx, dout, w_got, m_got):
    """touched rows within the bounds, every other row bit-identical"""
    ref = ER.rowwise_adagrad_ref(w0.numpy(), m0.numpy(), idx.numpy(), dout.float().numpy(), LR, EPS)
    rows = ref["rows"]
    wg, mg = w_got.cpu().numpy(), m_got.cpu().numpy()
    err_w = np.abs(wg[rows].astype(np.float64) - ref["weight"][rows])
    err_m = np.abs(mg[rows].astype(np.float64) - ref["momentum1"][rows])
    mw = record_parity(what + " weight", wg[rows], ref["weight"][rows], worst_over_bound=_worst(err_w, ref["tol_weight"]))
    mm = record_parity(what + " momentum1", mg[rows], ref["momentum1"][rows], worst_over_bound=_worst(err_m, ref["tol_momentum1"]))
    print(f"{what}: weight err/bound {_worst(err_w, ref['tol_weight']):.3f} rel_fro {mw['rel_fro']:.2e}; "
          f"momentum1 err/bound {_worst(err_m, ref['tol_momentum1']):.3f} rel_fro {mm['rel_fro']:.2e}")
    assert np.isfinite(wg[rows]).all() and (err_w <= ref["tol_weight"]).all(), what
    assert np.isfinite(mg[rows]).all() and (err_m <= ref["tol_momentum1"]).all(), what
    keep = np.ones(w0.shape[0], dtype=bool)
    keep[rows] = False
    assert np.array_equal(wg[keep].view(np.uint32), w0.numpy()[keep].view(np.uint32)), what + ": an untouched weight row changed"
    assert np.array_equal(mg[keep].view(np.uint32), m0.numpy()[keep].view(np.uint32)), what + ": an untouched momentum1 row changed"


def _run(w0, m0, idx, dout):
    from generative_recommenders_amd.ops.embedding import rowwise_adagrad_update_

    w, m1 = w0.to(DEV), m0.to(DEV)
    rowwise_adagrad_update_(w, m1, idx.to(DEV), dout.to(DEV), LR, EPS)
    torch.cuda.synchronize()
    return w, m1


# (n, dim, table_rows, id distribution): every n, dim, table size and distribution of the issue occurs; n = 257 with all ids
# equal crosses eight 32-row chunk boundaries (one owner, nine partial sums), (257, zipf, 2 rows) cuts two long segments,
# n = 1 / table_rows = 1 are the corners
SHAPES = [
    (1, 8, 1, "equal"), (1, 256, 100_003, "equal"), (63, 64, 8192, "distinct"), (64, 192, 8193, "distinct"),
    (65, 256, 100_003, "zipf"), (257, 8, 2, "zipf"), (257, 64, 8193, "equal"), (257, 192, 8192, "zipf"),
    (257, 256, 100_003, "distinct"), (64, 256, 1, "equal"), (65, 64, 2, "zipf"), (63, 192, 100_003, "zipf"),
]
CASES = [(n, d, r, k, t) for (n, d, r, k) in SHAPES for t in ("bf16", "f16", "f32")] + [
    (257, 1024, 8193, "zipf", "f32"), (65, 1024, 2, "equal", "f32"),         # fp32 dout at the 4 KiB row limit
    (257, 2048, 8193, "equal", "bf16"), (257, 2048, 2, "zipf", "f16"),       # 16-bit dout at it: 8 KiB table rows and partial sums
    (257, 512, 2, "zipf", "f32"), (257, 520, 2, "zipf", "bf16"),             # the widest dim with 32-row chunks, the first with 128
    # the chunk is 32 sorted rows below 262,144 ids (dim <= 512) and 128 from there on: the last n of the one, the first of the other, and
    # two runs of ~131,000 rows (a thousand partial sums each, shared among the combine kernel's waves)
    (262_143, 8, 8193, "zipf", "bf16"), (262_144, 8, 8193, "zipf", "bf16"), (262_144, 16, 2, "zipf", "f32"),
    # 3 ids, n = 2 * 128 + 1 (one id's run crosses both chunk boundaries: the combine kernel finishes it): four pieces of fp32 at
    # their smallest dim, and eight -- fp32 rows above 4 KiB, which go through the coalesced entry
    (257, 516, 3, "zipf", "f32"), (257, 1028, 3, "zipf", "f32")]


@pytest.mark.parametrize("n,dim,rows,kind,tag", CASES)
def test_update_against_the_formula_untouched_rows_and_determinism(n, dim, rows, kind, tag):
    g = torch.Generator().manual_seed(n * 1000 + dim)
    idx = _ids(kind, n, rows, g)
    if kind != "equal":
        assert 0 in idx.tolist() and rows - 1 in idx.tolist()
    dout = torch.randn(n, dim, generator=g).to(DT[tag])
    w0, m0 = _state(rows, dim, g)
    w, m1 = _run(w0, m0, idx, dout)
    _check(f"n{n} d{dim} rows{rows} {kind} {tag}", w0, m0, idx, dout, w, m1)
    w2, m2 = _run(w0, m0, idx, dout)
    assert torch.equal(w, w2) and torch.equal(m1, m2), "two runs of the same batch differ"


@pytest.mark.parametrize("tag", ["bf16", "f32"])
def test_hot_id_with_thousands_of_duplicates(tag):
    g = torch.Generator().manual_seed(7)
    rows, dim, n = 50_000, 256, 6000
    idx = torch.randint(0, rows, (n,), generator=g)
    idx[torch.randperm(n, generator=g)[:5000]] = 31_337
    assert int((idx == 31_337).sum()) >= 5000
    dout = torch.randn(n, dim, generator=g).to(DT[tag])
    w0, m0 = _state(rows, dim, g)
    w, m1 = _run(w0, m0, idx, dout)
    _check(f"hot id {tag}", w0, m0, idx, dout, w, m1)
    w2, m2 = _run(w0, m0, idx, dout)
    assert torch.equal(w, w2) and torch.equal(m1, m2), "two runs of the same batch differ"


def test_two_consecutive_steps_carry_the_state():
    from generative_recommenders_amd.ops.embedding import rowwise_adagrad_update_

    g = torch.Generator().manual_seed(11)
    rows, dim, n = 1000, 64, 300
    w0, m0 = _state(rows, dim, g)
    idx1 = torch.randint(0, 200, (n,), generator=g)
    idx2 = torch.randint(100, 300, (n,), generator=g)                       # overlaps the first batch on [100, 200)
    d1, d2 = torch.randn(n, dim, generator=g).bfloat16(), torch.randn(n, dim, generator=g).bfloat16()
    w, m1 = w0.to(DEV), m0.to(DEV)
    rowwise_adagrad_update_(w, m1, idx1.to(DEV), d1.to(DEV), LR, EPS)
    w_mid, m_mid = w.cpu(), m1.cpu()
    _check("step 1 of 2", w0, m0, idx1, d1, w_mid, m_mid)                   # with the rows step 1 must not touch, bit for bit
    rowwise_adagrad_update_(w, m1, idx2.to(DEV), d2.to(DEV), LR, EPS)
    torch.cuda.synchronize()
    # the second step is checked from the state the first one left (its own bound holds for that step) ...
    _check("step 2 of 2", w_mid, m_mid, idx2, d2, w, m1)
    # ... and the two steps together against the fp64 chain, the two steps' bounds added
    r1 = ER.rowwise_adagrad_ref(w0.numpy(), m0.numpy(), idx1.numpy(), d1.float().numpy(), LR, EPS)
    r2 = ER.rowwise_adagrad_ref(r1["weight"], r1["momentum1"], idx2.numpy(), d2.float().numpy(), LR, EPS)
    tol_w = np.zeros((rows, dim))
    tol_m = np.zeros(rows)
    # first-step errors pass through the second step: dW2/dW1 = 1, |dW2/dm| = c |G| / (2 sqrt(m) (sqrt(m) + eps)) <= c |G| / (2 m)
    tol_w[r1["rows"]] += r1["tol_weight"]
    tol_m[r1["rows"]] += r1["tol_momentum1"]
    G2 = np.zeros((rows, dim))
    np.add.at(G2, idx2.numpy(), d2.double().numpy())
    c2 = LR / (np.sqrt(r2["momentum1"]) + EPS)
    tol_w += (c2 / (2 * r2["momentum1"]) * tol_m)[:, None] * np.abs(G2) * 2
    tol_w[r2["rows"]] += r2["tol_weight"]
    tol_m[r2["rows"]] += r2["tol_momentum1"]
    touched = np.union1d(r1["rows"], r2["rows"])
    err_w = np.abs(w.cpu().numpy().astype(np.float64) - r2["weight"])[touched]
    err_m = np.abs(m1.cpu().numpy().astype(np.float64) - r2["momentum1"])[touched]
    record_parity("two steps weight", w.cpu().numpy()[touched], r2["weight"][touched], worst_over_bound=_worst(err_w, tol_w[touched]))
    assert (err_w <= tol_w[touched]).all() and (err_m <= tol_m[touched]).all()


def test_empty_batch_changes_nothing():
    g = torch.Generator().manual_seed(3)
    w0, m0 = _state(33, 64, g)
    w, m1 = _run(w0, m0, torch.zeros(0, dtype=torch.int64), torch.zeros(0, 64, dtype=torch.bfloat16))
    assert torch.equal(w.cpu(), w0) and torch.equal(m1.cpu(), m0)


def test_reference_scale_addressing_and_memory():
    """a 4.4 GB table (never initialised or read as a whole): rows on both sides of byte offsets 2^31 and 2^32, the last row,
    and no table-sized temporary"""
    from generative_recommenders_amd.ops.embedding import rowwise_adagrad_update_

    rows, dim, n = 4_300_000, 256, 4096
    g = torch.Generator().manual_seed(5)
    special = torch.tensor([0, 2_097_151, 2_097_152, 4_194_303, 4_194_304, 4_299_999])
    idx = torch.randint(0, rows, (n,), generator=g)
    idx[:12] = special.repeat(2)                    # each of them twice
    idx = idx[torch.randperm(n, generator=g)]
    touched = torch.unique(idx)
    near = torch.unique(torch.cat([touched - 1, touched, touched + 1]).clamp_(0, rows - 1))
    k = near.numel()
    w_near = torch.randn(k, dim, generator=g)
    m_near = torch.rand(k, generator=g) * 0.1
    dout = torch.randn(n, dim, generator=g).bfloat16()
    w = torch.empty(rows, dim, device=DEV)
    m1 = torch.empty(rows, device=DEV)
    near_d = near.to(DEV)
    w[near_d] = w_near.to(DEV)
    m1[near_d] = m_near.to(DEV)
    idx_d, dout_d = idx.to(DEV), dout.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rowwise_adagrad_update_(w, m1, idx_d, dout_d, LR, EPS)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print(f"peak memory grew by {grew / 2**20:.3f} MiB across the call")
    assert grew <= 16 * 2**20
    # the compact problem: the near rows renumbered 0 .. k-1
    compact = torch.searchsorted(near, idx)
    _check("4.3M x 256", w_near, m_near, compact, dout, w[near_d], m1[near_d])


def _three_feature_collection(rows_dtype=None):
    from generative_recommenders_amd.modules.dlrm_hstu import EmbeddingCollection, EmbeddingConfig, KeyedJaggedTensor

    ec = EmbeddingCollection([EmbeddingConfig(500, 64, "item", ["a", "b"]), EmbeddingConfig(300, 64, "user", ["c"])]).to(DEV)
    g = torch.Generator().manual_seed(17)
    ids = {"a": torch.randint(0, 40, (70,), generator=g), "b": torch.randint(20, 60, (50,), generator=g),      # overlap on [20, 40)
           "c": torch.randint(0, 300, (30,), generator=g)}
    feats = KeyedJaggedTensor(["a", "b", "c"], torch.cat([ids[k] for k in "abc"]).to(DEV), torch.tensor([70, 50, 30], device=DEV))
    douts = {k: torch.randn(v.numel(), 64, generator=g).to(rows_dtype or torch.float32) for k, v in ids.items()}
    return ec, ids, feats, douts


def test_embedding_collection_one_update_per_table_with_the_summed_gradient():
    ec, ids, feats, douts = _three_feature_collection()
    w0 = {t: e.weight.detach().cpu().clone() for t, e in ec.embeddings.items()}
    ec.apply_rowwise_adagrad_in_backward(lr=LR, eps=EPS)
    out = ec(feats)
    assert list(out) == ["a", "b", "c"]
    for k in "abc":
        assert torch.equal(out[k].values().detach().cpu(), w0["item" if k != "c" else "user"][ids[k]])
    sum((out[k].values() * douts[k].to(DEV)).sum() for k in "abc").backward()
    torch.cuda.synchronize()
    assert all(e.weight.grad is None and e.weight.requires_grad for e in ec.embeddings.values())
    state = ec.fused_optimizer_state_dict()
    z = lambda t: torch.zeros(w0[t].shape[0])
    idx_item, d_item = torch.cat([ids["a"], ids["b"]]), torch.cat([douts["a"], douts["b"]])
    _check("collection item", w0["item"], z("item"), idx_item, d_item, ec.embeddings["item"].weight.detach(), state["item.momentum1"])
    _check("collection user", w0["user"], z("user"), ids["c"], douts["c"], ec.embeddings["user"].weight.detach(), state["user.momentum1"])
    # Adagrad applied per feature is a different result: it must differ from what was computed by more than the bound
    one = ER.rowwise_adagrad_ref(w0["item"].numpy(), z("item").numpy(), idx_item.numpy(), d_item.numpy(), LR, EPS)
    s1 = ER.rowwise_adagrad_ref(w0["item"].numpy(), z("item").numpy(), ids["a"].numpy(), douts["a"].numpy(), LR, EPS)
    s2 = ER.rowwise_adagrad_ref(s1["weight"], s1["momentum1"], ids["b"].numpy(), douts["b"].numpy(), LR, EPS)
    shared = np.intersect1d(ids["a"].numpy(), ids["b"].numpy())
    assert shared.size > 0
    got = ec.embeddings["item"].weight.detach().cpu().numpy().astype(np.float64)
    pos = np.searchsorted(one["rows"], shared)
    gap = np.abs(got[shared] - s2["weight"][shared])
    assert (gap.max(axis=1) > 100 * one["tol_weight"][pos].max(axis=1)).all(), "the result equals two sequential updates"
    # a later step uses the new learning rate
    ec.set_learning_rate(0.0)
    before = ec.embeddings["item"].weight.detach().clone()
    ec(feats)["a"].values().sum().backward()
    assert torch.equal(before, ec.embeddings["item"].weight.detach())


def test_embedding_collection_bf16_rows():
    ec, ids, feats, douts = _three_feature_collection(torch.bfloat16)
    w0 = ec.embeddings["user"].weight.detach().cpu().clone()
    ec.apply_rowwise_adagrad_in_backward(lr=LR, eps=EPS, rows_dtype=torch.bfloat16, tables=["user"])
    out = ec(feats)
    assert out["c"].values().dtype == torch.bfloat16 and out["a"].values().dtype == torch.float32
    assert torch.equal(out["c"].values().detach().cpu(), w0[ids["c"]].bfloat16())
    out["c"].values().backward(douts["c"].to(DEV))
    torch.cuda.synchronize()
    assert ec.embeddings["user"].weight.grad is None and ec.embeddings["user"].weight.dtype == torch.float32
    _check("collection bf16 rows", w0, torch.zeros(300), ids["c"], douts["c"], ec.embeddings["user"].weight.detach(),
           ec.fused_optimizer_state_dict()["user.momentum1"])


def test_dlrm_hstu_fused_tables_match_the_formula_on_the_unfused_gradients(monkeypatch):
    """Copy A (unfused) gives the table gradients; the fp64 formula on them gives the expected tables and state.  Copy B
    (fused) must match them, with every other gradient and every output bit-identical to A's.

    The bound is the helper's, as it stands: its summation term (2m + 16) u A is more than twice the first-order (m - 1) u A of
    one fp32 sum, which leaves room for copy A's own fp32 segment sum next to the kernel's.  It needs the duplicates (m and
    A = sum |dout_i|), which the table gradient no longer shows: hooks on copy A's gathered rows record the gradient rows
    per feature."""
    from generative_recommenders_amd.modules.dlrm_hstu import apply_rowwise_adagrad_in_backward
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
            apply_rowwise_adagrad_in_backward(m, lr=LR, eps=EPS)
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
        assert params_b[name].grad is None
        w0, ga = tables0[table], p.grad.detach().cpu()
        rows = torch.nonzero(ga.abs().sum(dim=1) > 0).flatten()
        want = ER.rowwise_adagrad_ref(w0.numpy(), np.zeros(ga.shape[0]), rows.numpy(), ga[rows].numpy(), LR, EPS)
        keys = [k for k in uih.keys() + cand.keys() if k in R.tables()[table].feature_names]
        ids = torch.cat([(uih if k in uih.keys() else cand)[k].values() for k in keys])
        bound = ER.rowwise_adagrad_ref(w0.numpy(), np.zeros(ga.shape[0]), ids.numpy(), torch.cat([row_grads[k] for k in keys]).numpy(), LR, EPS)
        touched = bound["rows"]
        assert set(rows.tolist()) <= set(touched.tolist())
        w_got, m_got = params_b[name].detach().cpu().numpy(), state[table + ".momentum1"].cpu().numpy()
        err_w = np.abs(w_got[touched].astype(np.float64) - want["weight"][touched])
        err_m = np.abs(m_got[touched].astype(np.float64) - want["momentum1"][touched])
        over_w, over_m = _worst(err_w, bound["tol_weight"]), _worst(err_m, bound["tol_momentum1"])
        record_parity(f"dlrm table {table} weight", w_got[touched], want["weight"][touched], worst_over_bound=over_w)
        record_parity(f"dlrm table {table} momentum1", m_got[touched], want["momentum1"][touched], worst_over_bound=over_m)
        print(f"dlrm table {table}: weight err/bound {over_w:.3f}, momentum1 err/bound {over_m:.3f}")
        assert (err_w <= bound["tol_weight"]).all() and (err_m <= bound["tol_momentum1"]).all()
        keep = np.ones(w0.shape[0], dtype=bool)
        keep[touched] = False
        assert np.array_equal(w_got[keep], w0.numpy()[keep]) and (m_got[keep] == 0).all()
    assert seen_tables == 2
