"""Sampled-softmax loss on the fused HIP kernels vs the reference-minted golden vectors and the
oracle.  fp32: loss rtol 2e-5, gradients 1e-3 relative Frobenius (atomics: the table-gradient sum order is not fixed);
bf16 embeddings: loss 2e-2, gradients 2e-2.  test_lane_classes drives every lane class of loss_launch() -- LPE 1 .. 64 x three
I/O dtypes x forward / backward -- through the C ABI (tests/test_host_logic.py checks that LANE_CASES covers them)."""
import zlib

import numpy as np
import pytest
import torch

from conftest import load_cases
from oracle import hstu_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mods():
    import generative_recommenders_amd.research.modeling.sequential.autoregressive_losses as AL
    import generative_recommenders_amd.research.modeling.sequential.losses.sampled_softmax as SS

    return AL, SS


def _rel(got, ref):
    got = got.detach().double().cpu().numpy().reshape(np.shape(ref))
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def _fixed_draw(sampler, values):
    """Replace the sampler's random draw by the golden one (the reference drew on the CPU generator)."""
    t = torch.as_tensor(values, device=DEV)
    sampler._draw = lambda shape, high, like: t.reshape(shape)
    return sampler


@pytest.mark.parametrize("idx", range(3))
def test_golden_local_sampler(idx):
    AL, SS = _mods()
    c = load_cases("sampled_softmax.npz")[idx]
    emb = torch.nn.Embedding(*c["table"].shape).to(DEV)
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(c["table"]))
    all_ids = c["all_item_ids"].tolist()
    sampler = AL.LocalNegativesSampler(num_items=len(all_ids), item_emb=emb, all_item_ids=all_ids, l2_norm=bool(c["l2"]),
                                       l2_norm_eps=float(c["eps"])).to(DEV)
    # offsets into all_item_ids that reproduce the golden sampled ids
    where = {v: i for i, v in enumerate(all_ids)}
    _fixed_draw(sampler, np.vectorize(where.get)(c["sampled_ids"]))
    loss_mod = SS.SampledSoftmaxLoss(num_to_sample=int(c["R"]), softmax_temperature=float(c["T"]), model=None)
    q = torch.from_numpy(c["q"]).to(DEV).requires_grad_()
    pe = torch.from_numpy(c["pos_emb"]).to(DEV).requires_grad_()
    loss, aux = loss_mod.jagged_forward(output_embeddings=q, supervision_ids=torch.from_numpy(c["pos_ids"]).to(DEV),
                                        supervision_embeddings=pe, supervision_weights=torch.from_numpy(c["weights"]).to(DEV),
                                        negatives_sampler=sampler)
    assert aux == {}
    np.testing.assert_allclose(loss.item(), c["loss"], rtol=2e-5)
    loss.backward()
    assert _rel(q.grad, c["dq"]) < 1e-4
    assert _rel(pe.grad, c["dpos_emb"]) < 1e-4
    assert _rel(emb.weight.grad, c["dtable"]) < 1e-4
    # rows with weight 0 receive exact zeros
    dead = torch.from_numpy(c["weights"] == 0).to(DEV)
    assert idx == 2 or dead.any()
    assert not q.grad[dead].any() and not pe.grad[dead].any()


def test_golden_in_batch_sampler_dedup():
    AL, SS = _mods()
    c = load_cases("sampled_softmax.npz")[3]
    sampler = AL.InBatchNegativesSampler(l2_norm=True, l2_norm_eps=float(c["eps"]), dedup_embeddings=True)
    embs = torch.from_numpy(c["embeddings"]).to(DEV).requires_grad_()
    ids_t, pres_t = torch.from_numpy(c["ids"]).to(DEV), torch.from_numpy(c["presences"]).to(DEV)
    sampler.process_batch(ids=ids_t, presences=pres_t, embeddings=embs)
    # process_batch contract: one cached row per distinct valid id, holding the normalised embedding of ONE of its
    # occurrences.  WHICH occurrence is unspecified in the reference too (an index assignment with duplicate indices,
    # autoregressive_losses.py:172-175), so the golden numbers are reproduced with the reference's own choice:
    valid_ids = c["ids"][c["presences"]]
    valid_emb = c["embeddings"][c["presences"]]
    assert sorted(sampler._cached_ids.cpu().tolist()) == sorted(set(valid_ids.tolist()))
    normed = valid_emb / np.maximum(np.linalg.norm(valid_emb, axis=1, keepdims=True), 1e-6)
    mine = sampler._cached_embeddings.detach().cpu().numpy()
    for cid, row in zip(sampler._cached_ids.cpu().tolist(), mine):
        assert any(np.allclose(row, normed[j], atol=1e-6) for j in np.nonzero(valid_ids == cid)[0])
    choice = []
    for cid, row in zip(c["cached_ids"].tolist(), c["cached_embeddings"]):
        cand = [j for j in np.nonzero(valid_ids == cid)[0] if np.allclose(row, normed[j], atol=1e-6)]
        choice.append(cand[0])
    sampler._cached_ids = torch.from_numpy(c["cached_ids"]).to(DEV)
    sampler._cached_embeddings = sampler._maybe_l2_norm(embs[pres_t][torch.tensor(choice, device=DEV), :])
    _fixed_draw(sampler, c["sampled_offsets"])
    loss_mod = SS.SampledSoftmaxLoss(num_to_sample=int(c["R"]), softmax_temperature=float(c["T"]), model=None)
    q = torch.from_numpy(c["q"]).to(DEV).requires_grad_()
    pe = torch.from_numpy(c["pos_emb"]).to(DEV).requires_grad_()
    loss, _ = loss_mod.jagged_forward(output_embeddings=q, supervision_ids=torch.from_numpy(c["pos_ids"]).to(DEV),
                                      supervision_embeddings=pe, supervision_weights=torch.from_numpy(c["weights"]).to(DEV),
                                      negatives_sampler=sampler)
    np.testing.assert_allclose(loss.item(), c["loss"], rtol=2e-5)
    loss.backward()
    assert _rel(q.grad, c["dq"]) < 1e-4
    assert _rel(pe.grad, c["dpos_emb"]) < 1e-4
    assert _rel(embs.grad, c["dembeddings"]) < 1e-4     # through the cache's gather + normalisation (torch autograd)


def test_golden_padded_entry_point():
    AL, SS = _mods()
    c = load_cases("sampled_softmax.npz")[4]
    emb = torch.nn.Embedding(*c["table"].shape).to(DEV)
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(c["table"]))
    all_ids = c["all_item_ids"].tolist()
    sampler = AL.LocalNegativesSampler(num_items=len(all_ids), item_emb=emb, all_item_ids=all_ids, l2_norm=True, l2_norm_eps=1e-6).to(DEV)
    where = {v: i for i, v in enumerate(all_ids)}
    _fixed_draw(sampler, np.vectorize(where.get)(c["sampled_ids"]))
    loss_mod = SS.SampledSoftmaxLoss(num_to_sample=int(c["R"]), softmax_temperature=float(c["T"]))
    out_emb = torch.from_numpy(c["out_emb"]).to(DEV).requires_grad_()
    sup_emb = torch.from_numpy(c["sup_emb"]).to(DEV).requires_grad_()
    loss, _ = loss_mod(lengths=torch.from_numpy(c["lengths"]).to(DEV), output_embeddings=out_emb,
                       supervision_ids=torch.from_numpy(c["sup_ids"]).to(DEV), supervision_embeddings=sup_emb,
                       supervision_weights=torch.from_numpy(c["sup_weights"]).to(DEV), negatives_sampler=sampler)
    np.testing.assert_allclose(loss.item(), c["loss"], rtol=2e-5)
    loss.backward()
    assert _rel(out_emb.grad, c["dout_emb"]) < 1e-4
    assert _rel(sup_emb.grad, c["dsup_emb"]) < 1e-4
    assert _rel(emb.weight.grad, c["dtable"]) < 1e-4


@pytest.mark.parametrize("dtype,D,R,n,V,l2,T", [
    (torch.float32, 64, 512, 300, 5000, True, 0.05),      # Amazon-Books: D = 64, 512 negatives, l2 norm, T = 0.05
    (torch.bfloat16, 64, 512, 300, 5000, True, 0.05),
    (torch.float32, 50 // 2 * 2 + 2, 128, 77, 400, True, 0.05),   # D = 52: lanes past the row are masked
    (torch.float16, 256, 96, 40, 900, False, 1.0),        # ML-3B-like: 96 negatives, wide embeddings, no norm
    (torch.float32, 4, 3, 5, 7, True, 0.5),               # one 16-byte unit per embedding, fewer negatives than lanes
])
def test_vs_oracle(dtype, D, R, n, V, l2, T):
    _, SS = _mods()
    rng = np.random.default_rng(D * 1000 + R)
    table = torch.from_numpy(rng.standard_normal((V, D)) * 0.5).to(dtype)
    table[3] = 0
    q = torch.from_numpy(rng.standard_normal((n, D)) * 0.7).to(dtype)
    pos_ids = rng.integers(0, V, size=n)
    pos = table[pos_ids].clone()
    rows = rng.integers(0, V, size=(n, R))
    rows[:, 0] = pos_ids                                   # every row has one collision with its positive
    g_row = rng.random(n) * (rng.random(n) > 0.2)
    td, qd, pd = (t.to(DEV).requires_grad_() for t in (table, q, pos))
    rows_t, ids_t = torch.from_numpy(rows).to(DEV), torch.from_numpy(pos_ids).to(DEV)
    row_loss = SS.sampled_softmax_row_loss(qd, pd, td, ids_t, rows_t, rows_t, T, l2, l2, 1e-6)
    f = lambda t: t.double().numpy()
    w = np.ones(n)
    _, ref_rows, _ = O.sampled_softmax_fwd(f(q), f(pos), pos_ids, rows, rows, f(table), w, T, l2)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert _rel(row_loss, ref_rows) < tol
    (row_loss * torch.from_numpy(g_row).to(DEV).float()).sum().backward()
    # oracle gradients of sum_i g_i row_loss_i: weights g_i with the normaliser undone
    dq, dpos, dtable = O.sampled_softmax_bwd(f(q), f(pos), pos_ids, rows, rows, f(table), g_row, T, l2)
    s = g_row.sum()
    gtol = 1e-4 if dtype == torch.float32 else 2e-2
    assert _rel(qd.grad, dq * s) < gtol
    assert _rel(pd.grad, dpos * s) < gtol
    assert _rel(td.grad, dtable * s) < gtol


# ---------------------------------------------------------------------------------------------------------------------
# The lane classes of loss_launch(): LPE lanes per embedding = the smallest power of two >= dim * elt / 16, for three I/O
# dtypes, forward and backward.  Every row goes through the C ABI, so that row strides and gradient buffers are the test's.
#   (dtype group, D, LPE, pos_l2_norm, table_l2_norm, T, strided)
# strided: q, pos, table, dq and dpos rows lie 1, 2, 3, 2 and 1 16-byte units further apart than dim
LANE_CASES = [
    ("32", 4, 1, 1, 1, 0.05, False), ("32", 8, 2, 0, 0, 1.0, False), ("32", 12, 4, 1, 0, 0.05, False), ("32", 16, 4, 0, 1, 1.0, False),
    ("32", 32, 8, 1, 1, 1.0, False), ("32", 36, 16, 0, 0, 0.05, False), ("32", 64, 16, 0, 1, 0.05, False), ("32", 128, 32, 1, 0, 1.0, False),
    ("32", 132, 64, 1, 1, 0.05, False), ("32", 256, 64, 0, 0, 0.05, False),
    ("32", 12, 4, 0, 1, 1.0, True), ("32", 256, 64, 1, 1, 0.05, True),
    ("16", 8, 1, 1, 1, 0.05, False), ("16", 16, 2, 0, 0, 1.0, False), ("16", 24, 4, 1, 0, 0.05, False), ("16", 32, 4, 0, 1, 1.0, False),
    ("16", 64, 8, 1, 1, 1.0, False), ("16", 128, 16, 0, 0, 0.05, False), ("16", 256, 32, 0, 1, 0.05, False), ("16", 264, 64, 1, 0, 1.0, False),
    ("16", 512, 64, 0, 0, 0.05, False),
    ("16", 24, 4, 1, 1, 1.0, True), ("16", 512, 64, 1, 1, 0.05, True),
]
LANE_DTYPES = {"32": (torch.float32,), "16": (torch.bfloat16, torch.float16)}
# per LPE (G = 64 / LPE negatives per wave and step): R below G -- lane groups, and with R <= 3 G / 4 whole waves, never see
# a live negative -- and R = 4 G + 1, a second step with one live group; supervision rows; table rows
LANE_SHAPES = {1: ((1, 257), 6, 7), 2: ((9, 129), 7, 12), 4: ((7, 65), 8, 17), 8: ((5, 33), 9, 23), 16: ((3, 17), 6, 29),
               32: ((1, 9), 7, 34), 64: ((1, 5), 9, 40)}
LANE_EPS = 1e-2        # the clamp of the l2 norm: large enough that g / eps of the all-zero rows stays finite in fp16
LANE_SENT = -77.0
LANE_PAD = 256         # elements around every tensor: a 16-byte multiple in every dtype, and more than the widest lane tile
                       # (64 lanes x 8 features) reaches past a row of dtable
ROW_MASKED, ROW_ZERO_POS, ROW_SAMPLES_ZERO, TABLE_ZERO_ROW = 2, 3, 5, 2
ROWS_NO_GRAD = (1, 4)


def lane_rule(dim, elt):
    """loss_launch restated: the smallest power of two >= dim * elt / 16"""
    lpe = 1
    while lpe * 16 < dim * elt:
        lpe *= 2
    return lpe


class _Rows:
    """(rows, cols), rows `stride` elements apart, LANE_PAD elements into its own `fill`-filled allocation"""

    def __init__(self, rows, cols, dtype, stride=None, data=None, fill=LANE_SENT):
        self.rows, self.cols, self.stride, self.fill = rows, cols, stride or cols, fill
        n = 2 * LANE_PAD + (rows - 1) * self.stride + cols
        self.buf = torch.full((n,), fill, dtype=dtype, device=DEV)
        self.view = self.buf[LANE_PAD:].as_strided((rows, cols), (self.stride, 1))
        assert self.view.data_ptr() % 16 == 0
        if data is not None:
            self.view.copy_(data.reshape(rows, cols).to(dtype))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def bits(self):
        flat = self.buf.cpu()
        return flat.view(torch.int32 if flat.element_size() == 4 else torch.int16).numpy()

    def outside_untouched(self, what):
        bits = self.bits()
        inside = np.zeros(bits.size, dtype=bool)
        for r in range(self.rows):
            inside[LANE_PAD + r * self.stride: LANE_PAD + r * self.stride + self.cols] = True
        want = torch.tensor([self.fill], dtype=self.buf.dtype).view(torch.int32 if bits.itemsize == 4 else torch.int16).item()
        assert (bits[~inside] == want).all(), f"{what}: {(bits[~inside] != want).sum()} elements outside the tensor were written"

    def f64(self):
        return self.view.detach().double().cpu().numpy()


def _lane_params():
    out = []
    for grp, D, lpe, pl2, tl2, T, strided in LANE_CASES:
        for dtype in LANE_DTYPES[grp]:
            for R in LANE_SHAPES[lpe][0]:
                name = str(dtype).replace("torch.", "")
                out.append(pytest.param(dtype, D, lpe, R, pl2, tl2, T, strided,
                                        id=f"{name}-D{D}-lpe{lpe}-R{R}-p{pl2}t{tl2}-T{T}" + ("-strided" if strided else "")))
    return out


# tolerances: relative Frobenius against the float64 oracle, the file's own (test_vs_oracle)
LANE_TOL = {torch.float32: (1e-5, 1e-4), torch.bfloat16: (2e-2, 2e-2), torch.float16: (2e-2, 2e-2)}


def _rel64(got, ref):
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


@pytest.mark.parametrize("dtype,D,lpe,R,pl2,tl2,T,strided", _lane_params())
def test_lane_classes(dtype, D, lpe, R, pl2, tl2, T, strided, request):
    """Every LPE x dtype x direction of loss_launch() against the float64 oracle on inputs already rounded to the I/O dtype.

    Each call has a table row of zeros that is sampled and a positive embedding of zeros (both clamps of the l2 norm), a
    supervision row whose negatives all collide with its positive (loss exactly 0: |loss| <= 1e-6, left out of the
    relative norm), two rows with grad_row_loss == 0 (exact zeros in dq / dpos, nothing added to dtable), table rows
    gathered many times (R up to 257 from at most 40 rows) and a live negative in the LAST table row.  dtable starts as
    -0.0 -- zero to every sum -- inside a band of -0.0: an element the kernel added anything to, even +0.0, no longer
    has those bits, so the rows nobody sampled and the band show stray adds.  With a clamp active the gradient of the
    zero row is g / eps and carries the whole norm: the other rows are held to the same tolerance on their own as well.

    Every row holds the file's tolerances.  Largest errors measured on MI355X over the table (loss and lse | gradients):
    fp32 1.5e-7 | 1.0e-5, bf16 1.7e-7 | 2.4e-3, fp16 2.6e-7 | 2.6e-4; at D = 256 fp32 / D = 512 16-bit with T = 0.05 and no
    norm, which nobody had measured: fp32 1.5e-7 | 2.8e-6, bf16 6.3e-8 | 1.7e-3, fp16 1.2e-7 | 2.1e-4."""
    from generative_recommenders_amd import _lib as L

    lib, code, elt = L.lib(), L.torch_dtype_code(dtype), torch.empty(0, dtype=dtype).element_size()
    assert lane_rule(D, elt) == lpe, f"D = {D} x {elt} bytes is meant for LPE = {lpe}, the rule gives {lane_rule(D, elt)}"
    Rs, n, V = LANE_SHAPES[lpe]
    assert 6 <= n <= 9 and 7 <= V <= 40 and R in Rs
    unit = 16 // elt
    rng = np.random.default_rng(zlib.crc32(request.node.name.encode()))
    table = torch.from_numpy(rng.standard_normal((V, D)) * 0.5).to(dtype)
    table[TABLE_ZERO_ROW] = 0
    q = torch.from_numpy(rng.standard_normal((n, D)) * 0.7).to(dtype)
    pos_ids = rng.choice([r for r in range(V - 1) if r != TABLE_ZERO_ROW], size=n)
    pos = table[pos_ids].clone()
    pos[ROW_ZERO_POS] = 0
    rows = rng.integers(0, V, size=(n, R))
    rows[0, 0] = V - 1                               # a live negative in the last table row (pos_ids never name it)
    if R > 1:
        rows[0, 1] = pos_ids[0]                      # one collision next to live negatives
    rows[ROW_SAMPLES_ZERO, -1] = TABLE_ZERO_ROW
    rows[ROW_MASKED, :] = pos_ids[ROW_MASKED]        # every negative collides with the positive
    g_row = 0.25 + 0.75 * rng.random(n)
    g_row[list(ROWS_NO_GRAD)] = 0.0
    assert 1 <= (g_row == 0).sum() <= n // 2

    s = lambda k: D + k * unit if strided else D
    Q, POS, TABLE = _Rows(n, D, dtype, s(1), q), _Rows(n, D, dtype, s(2), pos), _Rows(V, D, dtype, s(3), table)
    ids_t, rows_t = torch.from_numpy(pos_ids).to(DEV), torch.from_numpy(rows).to(DEV)
    neg_ids_t = rows_t.clone()                       # the local sampler's: the item id of a table row is its index
    LOSS, LSE = _Rows(1, n, torch.float32), _Rows(1, n, torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    common = (Q.ptr, Q.stride, POS.ptr, POS.stride, ids_t.data_ptr(), rows_t.data_ptr(), neg_ids_t.data_ptr(), TABLE.ptr, TABLE.stride,
              V, n, R, D, T, pl2, tl2, LANE_EPS)
    L.check(lib.hstu_sampled_softmax_fwd(*common, LOSS.ptr, LSE.ptr, code, stream))
    torch.cuda.synchronize()
    f = lambda t: t.double().numpy()
    _, ref_loss, ref_lse = O.sampled_softmax_fwd(f(q), f(pos), pos_ids, rows, rows, f(table), np.ones(n), T, bool(pl2), LANE_EPS,
                                                 table_l2_norm=bool(tl2))
    tol, gtol = LANE_TOL[dtype]
    got_loss, got_lse = LOSS.f64()[0], LSE.f64()[0]
    live = np.arange(n) != ROW_MASKED
    e_loss, e_lse = _rel64(got_loss[live], ref_loss[live]), _rel64(got_lse, ref_lse)
    print(f"row loss rel {e_loss:.3e}, lse rel {e_lse:.3e} (tolerance {tol:.0e}); all-masked row: loss {got_loss[ROW_MASKED]:.3e}")
    assert np.isfinite(got_loss).all() and np.isfinite(got_lse).all()
    assert abs(ref_loss[ROW_MASKED]) <= 1e-12 and abs(got_loss[ROW_MASKED]) <= 1e-6
    assert e_loss < tol and e_lse < tol
    LOSS.outside_untouched("row_loss"), LSE.outside_untouched("lse")

    G = _Rows(1, n, torch.float32, data=torch.from_numpy(g_row))
    DQ, DPOS = _Rows(n, D, dtype, s(2)), _Rows(n, D, dtype, s(1))
    DTABLE = _Rows(V, D, torch.float32, fill=-0.0)
    L.check(lib.hstu_sampled_softmax_bwd(*common, LSE.ptr, G.ptr, DQ.ptr, DQ.stride, DPOS.ptr, DPOS.stride, DTABLE.ptr, code, stream))
    torch.cuda.synchronize()
    dq, dpos, dtable = (a * g_row.sum() for a in O.sampled_softmax_bwd(f(q), f(pos), pos_ids, rows, rows, f(table), g_row, T, bool(pl2),
                                                                        LANE_EPS, table_l2_norm=bool(tl2)))
    got_dq, got_dpos, got_dtable = DQ.f64(), DPOS.f64(), DTABLE.f64()
    errs = {"dq": _rel64(got_dq, dq), "dpos": _rel64(got_dpos, dpos), "dtable": _rel64(got_dtable, dtable)}
    if pl2:
        keep = np.arange(n) != ROW_ZERO_POS
        errs["dpos without the clamped row"] = _rel64(got_dpos[keep], dpos[keep])
    if tl2:
        keep = np.arange(V) != TABLE_ZERO_ROW
        errs["dtable without the clamped row"] = _rel64(got_dtable[keep], dtable[keep])
    print(", ".join(f"{k} rel {v:.3e}" for k, v in errs.items()) + f" (tolerance {gtol:.0e})")
    for a in (got_dq, got_dpos, got_dtable):
        assert np.isfinite(a).all()
    for k, v in errs.items():
        assert v < gtol, f"{k}: relative Frobenius error {v:.3e} (tolerance {gtol})"
    # grad_row_loss == 0: exact zeros, written by the kernel (the sentinel is gone)
    for r in ROWS_NO_GRAD:
        assert not got_dq[r].any() and not got_dpos[r].any()
    DQ.outside_untouched("dq"), DPOS.outside_untouched("dpos")
    # dtable: nothing outside it, and nothing in the rows that no live, unmasked negative of a row with gradient names
    DTABLE.outside_untouched("dtable")
    added = np.zeros(V, dtype=bool)
    for i in range(n):
        if g_row[i] != 0:
            added[rows[i][rows[i] != pos_ids[i]]] = True
    assert added[V - 1] and added[TABLE_ZERO_ROW]
    minus_zero = np.int32(-2 ** 31)
    bits = DTABLE.bits()[LANE_PAD:LANE_PAD + V * D].reshape(V, D)
    assert (bits[~added] == minus_zero).all(), "dtable: a row that no negative names was added to"
    for t in (Q, POS, TABLE, G):
        t.outside_untouched("an input's surroundings")


def test_errors_and_refusals():
    AL, SS = _mods()

    class _Mol(torch.nn.Module):
        def debug_str(self):
            return "mol-8x8"

    class _Model:
        _ndp_module = _Mol()

    with pytest.raises(NotImplementedError):
        SS.SampledSoftmaxLoss(num_to_sample=4, softmax_temperature=0.05, model=_Model())
    q = torch.zeros(3, 6, device=DEV)                       # 6 floats = 24 bytes: rows not 16-byte units
    ids = torch.zeros(3, dtype=torch.int64, device=DEV)
    rows = torch.zeros(3, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        SS.sampled_softmax_row_loss(q, q, q, ids, rows, rows, 0.05, True, True, 1e-6)
    q8 = torch.zeros(3, 8, device=DEV)
    with pytest.raises(RuntimeError, match="temperature"):
        SS.sampled_softmax_row_loss(q8, q8, q8, ids, rows, rows, 0.0, True, True, 1e-6)
    with pytest.raises(RuntimeError, match="int64"):
        SS.sampled_softmax_row_loss(q8, q8, q8, ids.int(), rows, rows, 0.05, True, True, 1e-6)
    # empty batch: no launch, empty result
    e = torch.zeros(0, 8, device=DEV)
    out = SS.sampled_softmax_row_loss(e, e, q8, ids[:0], rows[:0], rows[:0], 0.05, True, True, 1e-6)
    assert out.shape == (0,)
