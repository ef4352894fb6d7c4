"""CPU tests of the replicated in-backward row-wise Adagrad (ops/embedding.py, modules/dlrm_hstu.py): the settings, the
three-way decision in backward, what the replicated path hands to the kernels (with the launch functions replaced by
recorders), the exchange in a real two-process gloo group and the table checksum.  No kernel is launched."""

import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from generative_recommenders_amd.modules.dlrm_hstu import (EmbeddingCollection, EmbeddingConfig, KeyedJaggedTensor,
                                                          apply_rowwise_adagrad_in_backward)
from generative_recommenders_amd.ops import embedding as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _collection():
    return EmbeddingCollection([EmbeddingConfig(10, 8, "item", ["a", "b"]), EmbeddingConfig(6, 8, "user", ["c"])])


def _features():
    values = torch.tensor([1, 2, 2, 2, 3, 5, 0])
    return KeyedJaggedTensor(["a", "b", "c"], values, torch.tensor([3, 2, 2]))


def test_settings_default_to_off_and_a_second_call_replaces_them():
    cfg = E.RowWiseAdagradConfig(0.1)
    assert (cfg.replicated, cfg.process_group, cfg.average) == (False, None, True)
    ec = _collection()
    ec.apply_rowwise_adagrad_in_backward(lr=0.1)
    assert all((c.replicated, c.process_group, c.average) == (False, None, True) for c in ec._fused.values())
    group = object()
    apply_rowwise_adagrad_in_backward(ec, lr=0.2, tables=["item"], replicated=True, process_group=group, average=False)
    item, user = ec._fused["item"], ec._fused["user"]
    assert (item.lr, item.replicated, item.process_group, item.average) == (0.2, True, group, False)
    assert (user.lr, user.replicated, user.process_group, user.average) == (0.1, False, None, True)     # not named: as it was
    ec.apply_rowwise_adagrad_in_backward(lr=0.3, tables=["item"])                                        # named again: replaced
    assert (item.lr, item.replicated, item.process_group, item.average) == (0.3, False, None, True)
    fresh = _collection()
    fresh.apply_rowwise_adagrad_in_backward(lr=0.1, replicated=True, average=False)                      # the method, first call
    assert all(c.replicated and not c.average for c in fresh._fused.values())


class _FakeRanks:
    """torch.distributed as two ranks would see it from rank ``me``: all_gather hands back this rank's tensor and what the
    other rank 'sent' (its count, then its padded rows, then its padded G)"""

    def __init__(self, monkeypatch, me, other_rows, other_G):
        self.me, self.calls, self.sent = me, 0, []
        self.other = [torch.tensor([other_rows.numel()], dtype=torch.int32), other_rows, other_G]
        monkeypatch.setattr(dist, "is_available", lambda: True)
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
        monkeypatch.setattr(dist, "get_rank", lambda *a, **k: me)
        monkeypatch.setattr(dist, "get_backend", lambda *a, **k: "gloo")
        monkeypatch.setattr(dist, "all_gather", self.all_gather)

    def all_gather(self, out, t, group=None):
        other = self.other[self.calls]
        self.calls += 1
        self.sent.append(t.clone())
        if other.shape != t.shape:                  # the padding both ranks agreed on from the counts
            padded = torch.full_like(t, 99)
            padded[:other.shape[0]] = other
            other = padded
        out[self.me].copy_(t)
        out[1 - self.me].copy_(other)


@pytest.mark.parametrize("average,me", [(True, 0), (False, 0), (True, 1)])
def test_replicated_backward_scales_exchanges_and_concatenates_in_rank_order(monkeypatch, average, me):
    ec = _collection()
    ec.apply_rowwise_adagrad_in_backward(lr=0.1, tables=["user"], replicated=True, average=average)
    out = ec(_features())
    # this rank's coalesced list: 2 valid entries in capacity-4 buffers; the other rank's: 3 entries
    mine_rows, mine_G = torch.tensor([0, 5, -7, -7], dtype=torch.int32), torch.arange(32.0).reshape(4, 8)
    other_rows, other_G = torch.tensor([1, 4, 5], dtype=torch.int32), -torch.arange(24.0).reshape(3, 8)
    fake = _FakeRanks(monkeypatch, me, other_rows, other_G)
    seen = {}

    def coalesce(idx, dout, table_rows, scale=1.0):
        seen["coalesce"] = (idx.clone(), dout.clone(), table_rows, scale)
        return mine_rows, mine_G, torch.tensor([2], dtype=torch.int32)

    def update(weight, momentum1, idx, dout, lr, eps=1e-8):
        seen["update"] = (weight, momentum1, idx.clone(), dout.clone(), lr, eps)

    monkeypatch.setattr(E, "coalesce_row_gradients", coalesce)
    monkeypatch.setattr(E, "rowwise_adagrad_update_", update)
    out["c"].values().sum().backward()              # world size 2 and no refusal
    idx, dout, table_rows, scale = seen["coalesce"]
    assert idx.tolist() == [5, 0] and torch.equal(dout, torch.ones(2, 8)) and table_rows == 6
    assert scale == (0.5 if average else 1.0)
    weight, momentum1, rows_all, G_all, lr, eps = seen["update"]
    assert weight is ec.embeddings["user"].weight and momentum1 is ec._momentum1_user and (lr, eps) == (0.1, 1e-8)
    lists = [(mine_rows[:2], mine_G[:2]), (other_rows, other_G)]
    if me == 1:
        lists.reverse()                             # rank order, whoever runs it
    assert torch.equal(rows_all, torch.cat([l[0] for l in lists])) and rows_all.dtype == torch.int32
    assert torch.equal(G_all, torch.cat([l[1] for l in lists])) and G_all.dtype == torch.float32
    # what travelled: the count, then rows and G padded to the larger count (3), the entries past this rank's count zeroed
    assert [tuple(t.shape) for t in fake.sent] == [(1,), (3,), (3, 8)] and fake.sent[0].tolist() == [2]
    assert fake.sent[1].tolist() == [0, 5, 0] and torch.equal(fake.sent[2][:2], mine_G[:2])
    assert ec.embeddings["user"].weight.grad is None


def test_replicated_off_keeps_the_refusal_and_on_without_a_group_takes_the_one_shot_path(monkeypatch):
    ec = _collection()
    ec.apply_rowwise_adagrad_in_backward(lr=0.1, replicated=True)
    calls = []
    monkeypatch.setattr(E, "rowwise_adagrad_update_", lambda w, m, idx, dout, lr, eps=1e-8: calls.append(idx.tolist()))
    monkeypatch.setattr(E, "coalesce_row_gradients", lambda *a, **k: pytest.fail("no process group: nothing to exchange"))
    ec(_features())["c"].values().sum().backward()                             # no group initialised: today's path
    assert calls == [[5, 0]]
    ec.apply_rowwise_adagrad_in_backward(lr=0.1, tables=["user"])              # replicated off again
    out = ec(_features())
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="replicated tables would diverge"):
        out["c"].values().sum().backward()


def _exchange_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import datetime

    from generative_recommenders_amd.ops import embedding as E

    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}",
                            timeout=datetime.timedelta(seconds=60))
    results = []
    # uneven counts (3 and 1), a zero count on rank 1, zero counts everywhere
    for step, counts in enumerate([(3, 1), (2, 0), (0, 0)]):
        u, cap = counts[rank], 4
        rows = torch.full((cap,), -1, dtype=torch.int32)
        rows[:u] = torch.arange(u, dtype=torch.int32) * 2 + rank + 10 * step
        G = torch.full((cap, 4), float("nan"))
        G[:u] = torch.arange(u * 4, dtype=torch.float32).reshape(u, 4) + 100 * rank + 1000 * step
        rows_all, G_all = E.exchange_row_gradients(rows, G, torch.tensor([u], dtype=torch.int32))
        assert rows_all.shape == (sum(counts),) and G_all.shape == (sum(counts), 4)
        results.append((rows_all.clone(), G_all.clone()))
    # rank order: rank 0's valid entries first
    r0, g0 = results[0]
    assert r0.tolist() == [0, 2, 4, 1] and g0[3].tolist() == [100.0, 101.0, 102.0, 103.0] and g0[0].tolist() == [0.0, 1.0, 2.0, 3.0]
    assert results[1][0].tolist() == [10, 12] and not torch.isnan(results[1][1]).any()
    torch.save(results, os.path.join(out_dir, f"exchange{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_exchange_on_cpu_tensors_in_a_two_process_gloo_group(tmp_path):
    port = 29400 + (os.getpid() % 200)
    mp.spawn(_exchange_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = (torch.load(tmp_path / f"exchange{r}.pt") for r in (0, 1))
    assert len(a) == len(b) == 3
    for (ra, ga), (rb, gb) in zip(a, b):
        assert torch.equal(ra, rb) and torch.equal(ga, gb)          # the result is the same on both ranks


def test_fused_tables_checksum_is_exact_and_sees_every_bit():
    ec = _collection()
    assert E.fused_tables_checksum(ec) == {}                        # nothing fused: nothing to sum
    ec.apply_rowwise_adagrad_in_backward(lr=0.1)
    with torch.no_grad():
        ec.embeddings["item"].weight.copy_(torch.arange(80.0).reshape(10, 8) - 40.5)
        ec.embeddings["user"].weight.fill_(-0.0)
        ec._momentum1_item.copy_(torch.arange(10.0))
        ec._momentum1_user.fill_(1.0)
    want = lambda t: int(t.detach().numpy().view(np.int32).astype(np.int64).sum())
    sums = E.fused_tables_checksum(ec)
    assert sums == {"item": want(ec.embeddings["item"].weight) + want(ec._momentum1_item),
                    "user": 48 * -(1 << 31) + 6 * 0x3F800000}
    assert all(isinstance(v, int) for v in sums.values())
    assert E.fused_tables_checksum(ec) == sums
    # one flipped bit -- the lowest of one weight, the sign of a zero, the lowest of one state entry -- changes that table's sum only
    for table, tensor, bit in (("item", ec.embeddings["item"].weight, 1), ("user", ec.embeddings["user"].weight, -(1 << 31)),
                               ("item", ec._momentum1_item, 1)):
        bits = tensor.detach().view(torch.int32)
        pos = tuple(d // 2 for d in bits.shape)
        old = int(bits[pos])
        with torch.no_grad():
            bits[pos] = old ^ bit
        flipped = E.fused_tables_checksum(ec)
        other = "user" if table == "item" else "item"
        assert flipped[table] != sums[table] and flipped[other] == sums[other]
        with torch.no_grad():
            bits[pos] = old
        assert E.fused_tables_checksum(ec) == sums
    # a model that holds the collection stands for it
    holder = type("M", (), {"_embedding_collection": ec})()
    assert E.fused_tables_checksum(holder) == sums


def test_entry_points_for_coalesced_rows_validate_without_gpu():
    import ctypes as C

    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    buf = (C.c_char * 512)()
    a = (C.addressof(buf) + 255) & ~255
    merged = lambda dim=8, n=0, G=a: lib.hstu_embedding_rowwise_adagrad_coalesced(G, a, n, dim, 4, a, a, 0.1, 1e-8, a, 0, None)
    assert merged() == 0 and merged(dim=1032) == 0 and merged(dim=2048) == 0        # fp32 rows of up to 8 KiB; n == 0: nothing to do
    assert merged(dim=2052) == -2 and b"columns > 2048" in lib.hstu_last_error()
    assert merged(dim=6) == -1 and b"16-byte" in lib.hstu_last_error()
    assert merged(G=a + 4) == -1 and b"16-byte" in lib.hstu_last_error()
    assert merged(n=4) == -1 and b"workspace too small" in lib.hstu_last_error()
    # the one-shot entry point keeps its 4 KiB rows
    assert lib.hstu_embedding_rowwise_adagrad(a, a, 0, 1032, 4, a, a, 0.1, 1e-8, a, 0, 2, None) == -2 and b"bytes" in lib.hstu_last_error()
    need, base = C.c_int64(0), C.c_int64(0)
    assert lib.hstu_embedding_grad_coalesce_workspace_bytes(4096, 4_300_000, C.byref(need)) == 0
    assert lib.hstu_embedding_rowwise_adagrad_workspace_bytes(4096, 4_300_000, C.byref(base)) == 0
    assert base.value < need.value <= base.value + 4 * 4096 + 512                    # 4 more bytes per id, whatever the table
    coalesce = lambda dim=8, dt=0: lib.hstu_embedding_grad_coalesce(a, a, 4, dim, 4, 1.0, a, a, a, a, 0, dt, None)
    assert coalesce(dim=2056) == -2 and coalesce(dim=1032, dt=2) == -2 and coalesce(dim=12) == -1
    assert coalesce() == -1 and b"workspace too small" in lib.hstu_last_error()


def test_in_sync_check_without_a_group_is_a_no_op():
    ec = _collection()
    ec.apply_rowwise_adagrad_in_backward(lr=0.1, replicated=True)
    E.assert_fused_tables_in_sync(ec)
