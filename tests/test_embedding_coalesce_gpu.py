"""GPU tests of the row-gradient coalesce (hstu_embedding_grad_coalesce in csrc/embedding_optim.hip,
ops/embedding.py: coalesce_row_gradients) and of the replicated update built on it with the ranks emulated on one GPU.
References and bounds: embedding_coalesce_ref.py (fp64; first-order bounds in any summation order, constants doubled).

Two stages against one (test_two_stages_equal_the_one_shot_update): the update adds the squares of G in one tree for
every row layout and rounds every square on its own, so coalescing and then applying the fp32 rows gives the bits of the
one-shot update on the 16-bit rows; fp32 rows of up to 8 KiB (2048 columns) go through
hstu_embedding_rowwise_adagrad_coalesced."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import embedding_coalesce_ref as CR
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, EPS = 0.05, 1e-8
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _ids(kind, n, rows, g):
    """n ids in [0, rows); zipf and distinct batches hold id 0 and id rows - 1 whenever there is room for both"""
    if kind == "equal":
        return torch.full((n,), rows - 1, dtype=torch.int64)
    if kind == "distinct":
        assert n <= rows
        idx = torch.randperm(rows, generator=g)[:n]
    elif kind == "hot":                             # one id with 5,000 duplicates among the batch
        idx = torch.randint(0, rows, (n,), generator=g)
        idx[torch.randperm(n, generator=g)[:5000]] = rows // 2
    else:                                           # zipf: rank r with probability ~ 1 / (r + 1), the ranks scattered over the table
        p = 1.0 / torch.arange(1, rows + 1, dtype=torch.float64)
        idx = torch.randperm(rows, generator=g)[torch.multinomial(p, n, replacement=True, generator=g)]
    if n >= 2 and kind != "hot":
        idx[0], idx[-1] = 0, rows - 1
    return idx


# (n, dim, dtype, table_rows, ids, scale).  Chunks are 32 sorted rows below 262,144 ids with dim <= 512, else 128.
SHAPES = [
    # one lane per row, and the three register classes (rows of <= 1 KiB, <= 2 KiB, <= 4 KiB)
    (129, 8, "bf16", 8193, "zipf", 1.0), (129, 4, "f32", 50, "zipf", 0.5), (129, 256, "bf16", 50, "zipf", 1.0),
    (129, 264, "bf16", 8193, "zipf", 1 / 3), (129, 1024, "bf16", 50, "zipf", 1.0), (129, 2048, "bf16", 50, "zipf", 0.5),
    (129, 1024, "f32", 50, "zipf", 1 / 3),
    # the small chunk's edges; 7 ids: runs that cross the boundaries
    (1, 64, "bf16", 7, "zipf", 1.0), (31, 64, "f16", 7, "zipf", 1.0), (32, 64, "bf16", 7, "zipf", 0.5), (33, 64, "bf16", 7, "zipf", 1 / 3),
    (129, 64, "f32", 7, "zipf", 1.0),
    # the large chunk
    (300, 1024, "bf16", 7, "zipf", 1.0), (262_144, 8, "bf16", 8193, "zipf", 0.5),
    # a run cut across more than 64 chunks: the combine kernel's look-ahead loop goes round a second time
    (6000, 64, "bf16", 50_000, "hot", 1.0),
    (257, 64, "bf16", 100_003, "distinct", 1.0), (257, 64, "f32", 8193, "equal", 1 / 3), (4097, 8, "f32", 3, "zipf", 1.0),
    # the issue's grid-stride shape (at this n the chunk is 128 and the 8192-block grid still covers it in one trip) and the
    # first n whose 128-row chunks do need the second trip; 4097 above is the scan's third tile
    (32 * 4 * 8192 + 33, 8, "bf16", 8193, "zipf", 1.0), (128 * 4 * 8192 + 33, 8, "bf16", 100_003, "zipf", 0.5),
    # 3 ids, so that a run crosses every chunk boundary, at the smallest dim of: two pieces of fp32 (32-row chunks), four pieces
    # of fp32 and of 16 bits (128-row chunks, n = 2 * 128 + 1); and the narrowest fp32 row in 128-row chunks
    (65, 260, "f32", 3, "zipf", 1 / 3), (257, 516, "f32", 3, "zipf", 1.0), (257, 1032, "bf16", 3, "zipf", 0.5),
    (262_144, 4, "f32", 3, "zipf", 1.0),
]
IDS = [f"n{n}-d{d}-{t}-r{r}-{k}-s{s:.2f}" for n, d, t, r, k, s in SHAPES]


@functools.lru_cache(maxsize=None)
def _batch(n, dim, tag, rows, kind):
    g = torch.Generator().manual_seed(n * 1000 + dim)
    idx = _ids(kind, n, rows, g)
    dout = torch.randn(n, dim, generator=g).to(DT[tag])
    return idx, dout, idx.to(DEV), dout.to(DEV)


def _state(rows, dim, g):
    w = torch.randn(rows, dim, generator=g)
    m1 = torch.rand(rows, generator=g) * 0.1
    w[1::2] = torch.tensor(-12345.671875)           # a NaN-free pattern on every other row
    m1[1::2] = 6789.0625
    return w, m1


def _worst(err, tol):
    live = tol > 0
    return float((err[live] / tol[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("n,dim,tag,rows,kind,scale", SHAPES, ids=IDS)
def test_coalesce_against_the_reference_and_twice(n, dim, tag, rows, kind, scale):
    from generative_recommenders_amd.ops.embedding import coalesce_row_gradients

    idx, dout, idx_d, dout_d = _batch(n, dim, tag, rows, kind)
    ref = CR.coalesce_ref(idx.numpy(), dout.float().numpy(), scale)
    if kind == "zipf" and n >= 2:
        assert ref["rows"][0] == 0 and ref["rows"][-1] == rows - 1
    if kind == "hot":
        assert ref["counts"].max() >= 5000
    out = []
    for _ in range(2):
        r, G, count = coalesce_row_gradients(idx_d, dout_d, rows, scale)
        assert r.shape == (n,) and r.dtype == torch.int32 and G.shape == (n, dim) and G.dtype == torch.float32
        u = int(count)
        out.append((u, r[:u].clone(), G[:u].clone()))
    u, r, G = out[0]
    assert u == len(ref["rows"])
    assert np.array_equal(r.cpu().numpy(), ref["rows"])
    got = G.cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref["G"])
    over = _worst(err, ref["tol"])
    record_parity(f"coalesce n{n} d{dim} {tag} {kind}", got, ref["G"], worst_over_bound=over)
    print(f"coalesce n{n} d{dim} {tag} rows{rows} {kind} scale {scale:.3f}: u = {u}, err/bound {over:.3f}")
    assert np.isfinite(got).all() and (err <= ref["tol"]).all()
    assert out[1][0] == u and torch.equal(out[1][1], r) and torch.equal(out[1][2], G), "two runs of the same batch differ"


def _raw_call(lib, dout, idx, n, dim, table_rows, scale, rows, G, count, ws, ws_bytes, dtype=0):
    return lib.hstu_embedding_grad_coalesce(dout, idx, n, dim, table_rows, scale, rows, G, count, ws, ws_bytes, dtype,
                                            torch.cuda.current_stream().cuda_stream)


def test_empty_batch_writes_count_zero_and_nothing_else():
    from generative_recommenders_amd import _lib as L
    from generative_recommenders_amd.ops.embedding import coalesce_row_gradients

    rows = torch.full((16,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    G = torch.full((16, 8), -12345.671875, device=DEV)
    count = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    rc = _raw_call(L.lib(), None, None, 0, 8, 100, 1.0, rows.data_ptr(), G.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    assert rc == 0 and int(count) == 0
    assert bool((rows == 0x5A5A5A5A).all()) and bool((G == -12345.671875).all())
    r, g, c = coalesce_row_gradients(torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, 8, dtype=torch.bfloat16, device=DEV), 100)
    assert r.shape == (0,) and g.shape == (0, 8) and int(c) == 0


@pytest.mark.parametrize("n,dim,tag,rows,kind,scale", SHAPES, ids=IDS)
def test_two_stages_equal_the_one_shot_update(n, dim, tag, rows, kind, scale):
    """coalesce (scale 1) + the update on (rows[:u], G[:u]) against the one-shot update on (idx, dout): torch.equal on weight and
    momentum1"""
    from generative_recommenders_amd.ops.embedding import coalesce_row_gradients, rowwise_adagrad_update_

    idx, dout, idx_d, dout_d = _batch(n, dim, tag, rows, kind)
    w0, m0 = _state(rows, dim, torch.Generator().manual_seed(dim))
    w1, m1 = w0.to(DEV), m0.to(DEV)
    rowwise_adagrad_update_(w1, m1, idx_d, dout_d, LR, EPS)
    w2, m2 = w0.to(DEV), m0.to(DEV)
    r, G, count = coalesce_row_gradients(idx_d, dout_d, rows, 1.0)
    u = int(count)
    rowwise_adagrad_update_(w2, m2, r[:u], G[:u], LR, EPS)
    torch.cuda.synchronize()
    dw, dm = int((w1 != w2).any(dim=1).sum()), int((m1 != m2).sum())
    print(f"two stages n{n} d{dim} {tag} {kind}: {dw} of {u} weight rows and {dm} momentum1 entries differ")
    assert torch.equal(m1, m2), f"{dm} of {u} momentum1 entries differ"
    assert torch.equal(w1, w2), f"{dw} of {u} weight rows differ"


def test_refusals_return_the_code_and_the_message_and_write_nothing():
    from generative_recommenders_amd import _lib as L

    lib = L.lib()
    n, dim = 64, 8
    need = C.c_int64(0)
    assert lib.hstu_embedding_grad_coalesce_workspace_bytes(n, 100, C.byref(need)) == 0 and need.value > 0
    assert lib.hstu_embedding_grad_coalesce_workspace_bytes(-1, 100, C.byref(need)) == -1
    big = C.c_int64(0)
    assert lib.hstu_embedding_grad_coalesce_workspace_bytes(n, 4_300_000, C.byref(big)) == 0 and big.value < (1 << 20)
    dout = torch.randn(n, 4096, device=DEV).bfloat16()
    idx = torch.randint(0, 100, (n,), dtype=torch.int32, device=DEV)
    rows = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    G = torch.full((n * 4096 + 4,), -12345.671875, device=DEV)
    count = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ws = torch.empty(need.value + 256, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) & ~255
    call = lambda dim=dim, dout_p=dout.data_ptr(), g_p=G.data_ptr(), ws_bytes=need.value, dt=0: _raw_call(
        lib, dout_p, idx.data_ptr(), n, dim, 100, 1.0, rows.data_ptr(), g_p, count.data_ptr(), base, ws_bytes, dt)
    assert call(dim=2056) == -2 and b"columns > 2048" in lib.hstu_last_error()
    assert call(dim=1 << 30) == -2 and b"columns" in lib.hstu_last_error()
    assert call(dim=1032, dt=2) == -2 and b"bytes" in lib.hstu_last_error()             # fp32 dout: 4 KiB is 1024 columns
    assert call(dim=12) == -1 and b"16-byte" in lib.hstu_last_error()                   # 24-byte rows
    assert call(dout_p=dout.data_ptr() + 8) == -1 and b"16-byte" in lib.hstu_last_error()
    assert call(g_p=G.data_ptr() + 4) == -1 and b"16-byte" in lib.hstu_last_error()
    assert call(ws_bytes=need.value - 1) == -1 and b"workspace too small" in lib.hstu_last_error()
    assert call(dt=3) == -1 and b"dtype" in lib.hstu_last_error()
    torch.cuda.synchronize()
    assert int(count) == 77 and bool((rows == 0x5A5A5A5A).all()) and bool((G == -12345.671875).all())
    assert call() == 0                               # the same arguments, nothing wrong: it runs
    torch.cuda.synchronize()
    assert 0 < int(count) <= n


# ---- ranks emulated on one GPU: shard, coalesce each with 1 / W, concatenate in rank order, update
def _emulated_step(w0, m0, shards, dim, rows, scale):
    from generative_recommenders_amd.ops.embedding import coalesce_row_gradients, rowwise_adagrad_update_

    parts = []
    for idx, dout in shards:
        r, G, count = coalesce_row_gradients(idx.to(DEV), dout.to(DEV), rows, scale)
        u = int(count)
        parts.append((r[:u], G[:u]))
    w, m1 = w0.to(DEV), m0.to(DEV)
    rowwise_adagrad_update_(w, m1, torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), LR, EPS)
    torch.cuda.synchronize()
    return w, m1


# dim 2048 in 16 bits: the merged fp32 rows are 8 KiB, and the runs of a row's partial sums that cross a chunk boundary go
# through the combine kernel at that width
@pytest.mark.parametrize("world,tag,dim", [(w, t, 64) for t in ("bf16", "f32") for w in (2, 3, 8)] + [(3, "bf16", 2048), (8, "f16", 1032)])
def test_emulated_ranks_match_the_formula_on_the_whole_batch(world, tag, dim):
    g = torch.Generator().manual_seed(100 + world)
    rows, n = 300, 700
    idx = _ids("zipf", n, rows, g)
    idx[idx == 5] = 6                               # a row no shard touches
    dout = torch.randn(n, dim, generator=g).to(DT[tag])
    # uneven shards, the second one empty
    cuts = [0, n, n] if world == 2 else [0, 37, 37] + sorted(torch.randint(38, n, (world - 3,), generator=g).tolist()) + [n]
    assert len(cuts) == world + 1
    shards = [(idx[a:b], dout[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert any(s[0].numel() == 0 for s in shards) and len({s[0].numel() for s in shards}) > 1
    w0, m0 = _state(rows, dim, g)
    w, m1 = _emulated_step(w0, m0, shards, dim, rows, 1.0 / world)
    ref = CR.replicated_adagrad_ref(w0.numpy(), m0.numpy(), idx.numpy(), dout.float().numpy(), LR, EPS, 1.0 / world)
    touched = ref["rows"]
    wg, mg = w.cpu().numpy(), m1.cpu().numpy()
    err_w = np.abs(wg[touched].astype(np.float64) - ref["weight"][touched])
    err_m = np.abs(mg[touched].astype(np.float64) - ref["momentum1"][touched])
    over_w, over_m = _worst(err_w, ref["tol_weight"]), _worst(err_m, ref["tol_momentum1"])
    record_parity(f"emulated ranks W{world} {tag} d{dim} weight", wg[touched], ref["weight"][touched], worst_over_bound=over_w)
    record_parity(f"emulated ranks W{world} {tag} d{dim} momentum1", mg[touched], ref["momentum1"][touched], worst_over_bound=over_m)
    print(f"emulated ranks W{world} {tag} d{dim}: weight err/bound {over_w:.3f}, momentum1 err/bound {over_m:.3f}")
    assert (err_w <= ref["tol_weight"]).all() and (err_m <= ref["tol_momentum1"]).all()
    keep = np.ones(rows, dtype=bool)
    keep[touched] = False
    assert keep[5]
    assert np.array_equal(wg[keep].view(np.uint32), w0.numpy()[keep].view(np.uint32)), "an untouched weight row changed"
    assert np.array_equal(mg[keep].view(np.uint32), m0.numpy()[keep].view(np.uint32)), "an untouched momentum1 entry changed"
    w2, m2 = _emulated_step(w0, m0, shards, dim, rows, 1.0 / world)
    assert torch.equal(w, w2) and torch.equal(m1, m2), "the same shards in the same order gave different tables"
