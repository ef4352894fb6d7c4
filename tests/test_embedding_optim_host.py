"""CPU tests of the in-backward row-wise Adagrad: the fp64 reference helper against a hand-computed example, the refusals
(weight_decay, non-fp32 tables, CPU tensors, more than one rank), the state-dict keys and the optimizer-state round trip.
No kernel is launched."""

import ctypes as C

import numpy as np
import pytest
import torch

import embedding_optim_ref as ER
from generative_recommenders_amd.modules.dlrm_hstu import (EmbeddingCollection, EmbeddingConfig, JaggedTensor, KeyedJaggedTensor,
                                                          apply_rowwise_adagrad_in_backward)
from generative_recommenders_amd.ops import embedding as E


def _collection():
    return EmbeddingCollection([EmbeddingConfig(10, 8, "item", ["a", "b"]), EmbeddingConfig(6, 8, "user", ["c"])])


def _features():
    values = torch.tensor([1, 2, 2, 2, 3, 5, 0])
    return KeyedJaggedTensor(["a", "b", "c"], values, torch.tensor([3, 2, 2]))


def test_reference_helper_against_a_hand_computed_three_row_example():
    w = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    m1 = np.array([0.0, 1.0, 4.0])
    idx = np.array([2, 0, 2])
    dout = np.array([[1.0, 3.0], [2.0, 0.0], [1.0, 1.0]])
    r = ER.rowwise_adagrad_ref(w, m1, idx, dout, lr=0.5, eps=0.0)
    # row 0: G = (2, 0), momentum1 = 0 + 2 = 2, step = 0.5 / sqrt(2);  row 2: G = (2, 4), momentum1 = 4 + 10 = 14; row 1 untouched
    assert r["rows"].tolist() == [0, 2]
    np.testing.assert_allclose(r["momentum1"], [2.0, 1.0, 14.0], rtol=0, atol=1e-15)
    s0, s2 = 0.5 / np.sqrt(2.0), 0.5 / np.sqrt(14.0)
    np.testing.assert_allclose(r["weight"], [[1 - 2 * s0, 2.0], [3.0, 4.0], [5 - 2 * s2, 6 - 4 * s2]], rtol=0, atol=1e-15)
    # the bounds: row 2 has m = 2, A = (2, 4), G = (2, 4)
    u = 2.0 ** -24
    np.testing.assert_allclose(r["tol_weight"][1], s2 * 20 * u * np.array([2.0, 4.0]) + 8 * u * (np.array([5.0, 6.0]) + s2 * np.array([2.0, 4.0])),
                               rtol=1e-12)
    np.testing.assert_allclose(r["tol_momentum1"][1], (4 * u * (4 + 16) / 2 + 4 * u * 10) + 3 * u * 10 + 2 * u * 14, rtol=1e-12)
    assert w[0, 0] == 1.0 and m1[0] == 0.0          # the inputs are not modified


def test_weight_decay_is_refused():
    with pytest.raises(NotImplementedError, match="weight_decay"):
        apply_rowwise_adagrad_in_backward(_collection(), lr=0.1, weight_decay=1e-4)
    with pytest.raises(NotImplementedError, match="weight_decay"):
        _collection().apply_rowwise_adagrad_in_backward(lr=0.1, weight_decay=1e-4)


def test_non_fp32_tables_are_refused():
    with pytest.raises(RuntimeError, match="float32"):
        apply_rowwise_adagrad_in_backward(_collection().to(torch.bfloat16), lr=0.1)
    ec = _collection()
    ec.apply_rowwise_adagrad_in_backward(lr=0.1)
    ec.to(torch.bfloat16)                           # cast away afterwards: the first forward raises
    with pytest.raises(RuntimeError, match="must stay float32"):
        ec(_features())


def test_cpu_tensors_are_refused():
    w, m1 = torch.zeros(4, 8), torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.rowwise_adagrad_update_(w, m1, torch.tensor([1]), torch.zeros(1, 8), 0.1)
    ec = _collection()
    ec.apply_rowwise_adagrad_in_backward(lr=0.1)
    out = ec(_features())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sum(v.values().sum() for v in out.values()).backward()
    assert all(e.weight.grad is None for e in ec.embeddings.values())


def test_more_than_one_rank_is_refused_at_the_first_fused_backward(monkeypatch):
    ec = _collection()
    ec.apply_rowwise_adagrad_in_backward(lr=0.1)
    out = ec(_features())
    monkeypatch.setattr(torch.distributed, "is_available", lambda: True)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="world size 2"):
        out["a"].values().sum().backward()


def test_state_dict_keys_are_unchanged_and_the_state_follows_the_module():
    ec = _collection()
    keys = sorted(ec.state_dict())
    assert keys == ["embeddings.item.weight", "embeddings.user.weight"]
    ec.apply_rowwise_adagrad_in_backward(lr=0.1, tables=["item"])
    assert sorted(ec.state_dict()) == keys
    assert sorted(ec.fused_optimizer_state_dict()) == ["item.momentum1"]
    assert all(p.requires_grad for p in ec.parameters())
    assert [n for n, _ in ec.named_buffers()] == ["_momentum1_item"]
    assert ec.to(torch.float64)._momentum1_item.dtype == torch.float64     # buffers move with the module (.to(device) too)
    with pytest.raises(KeyError):
        _collection().apply_rowwise_adagrad_in_backward(lr=0.1, tables=["nope"])


def test_settings_are_kept_per_table():
    ec = _collection()
    ec.apply_rowwise_adagrad_in_backward(lr=0.1, rows_dtype=torch.bfloat16, tables=["item"])
    ec.apply_rowwise_adagrad_in_backward(lr=0.2, eps=1e-6, tables=["user"])
    out = ec(_features())
    assert out["a"].values().dtype == out["b"].values().dtype == torch.bfloat16 and out["c"].values().dtype == torch.float32
    assert (ec._fused["item"].lr, ec._fused["item"].eps) == (0.1, 1e-8) and (ec._fused["user"].lr, ec._fused["user"].eps) == (0.2, 1e-6)
    ec.apply_rowwise_adagrad_in_backward(lr=0.3, tables=["item"])             # named again: replaced
    assert ec(_features())["a"].values().dtype == torch.float32 and ec._fused["item"].lr == 0.3


def test_fused_optimizer_state_dict_round_trips():
    a, b = _collection(), _collection()
    for ec in (a, b):
        ec.apply_rowwise_adagrad_in_backward(lr=0.1)
    state = a.fused_optimizer_state_dict()
    assert sorted(state) == ["item.momentum1", "user.momentum1"]
    assert state["item.momentum1"].shape == (10,) and state["item.momentum1"].dtype == torch.float32
    with torch.no_grad():
        state["item.momentum1"].copy_(torch.arange(10.0))
        state["user.momentum1"].fill_(0.25)
    b.load_fused_optimizer_state_dict({k: v.clone() for k, v in a.fused_optimizer_state_dict().items()})
    for k, v in b.fused_optimizer_state_dict().items():
        assert torch.equal(v, a.fused_optimizer_state_dict()[k])
    with pytest.raises(KeyError):
        b.load_fused_optimizer_state_dict({"item.momentum1": torch.zeros(10)})
    a.set_learning_rate(0.5)
    assert all(cfg.lr == 0.5 for cfg in a._fused.values())


def test_fused_forward_gathers_each_table_once_and_matches_the_unfused_rows():
    torch.manual_seed(0)
    plain, fused = _collection(), _collection()
    fused.load_state_dict(plain.state_dict())
    fused.apply_rowwise_adagrad_in_backward(lr=0.1)
    calls = []
    orig = E._GatherRowsFusedFunction.apply
    try:
        E._GatherRowsFusedFunction.apply = staticmethod(lambda *a: (calls.append(a[2].numel()), orig(*a))[1])
        got = fused(_features())
    finally:
        E._GatherRowsFusedFunction.apply = orig
    want = plain(_features())
    assert calls == [5, 2]                          # item: the ids of a and b together; user: c
    assert list(got) == list(want) == ["a", "b", "c"]
    for k in want:
        assert torch.equal(got[k].values(), want[k].values()) and torch.equal(got[k].lengths(), want[k].lengths())


def test_entry_point_validation_without_gpu():
    import os

    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    need = C.c_int64(-1)
    assert lib.hstu_embedding_rowwise_adagrad_workspace_bytes(4096, 4_300_000, C.byref(need)) == 0
    assert 0 < need.value < (1 << 20)               # O(n): 136 bytes per id + the sort's temporary, whatever the table size
    assert lib.hstu_embedding_rowwise_adagrad_workspace_bytes(-1, 8, C.byref(need)) == -1
    buf = (C.c_char * 512)()
    a = (C.addressof(buf) + 255) & ~255
    call = lambda dout=a, n=0, dim=8, rows=4, w=a, m=a, dt=0: lib.hstu_embedding_rowwise_adagrad(dout, a, n, dim, rows, w, m, 0.1, 1e-8, a, 0, dt, None)
    assert call() == 0                              # n == 0: nothing to do
    assert call(w=None) == -1 and b"non-NULL" in lib.hstu_last_error()
    assert call(dim=12) == -1 and b"16-byte" in lib.hstu_last_error()
    assert call(dim=4096) == -2 and b"rows of" in lib.hstu_last_error()
    assert call(dim=1 << 30) == -2 and b"rows of" in lib.hstu_last_error()       # dim * 4 would wrap to 0
    assert call(dim=1032, dt=2) == -2 and b"bytes" in lib.hstu_last_error()      # fp32: 4 KiB is 1024 columns
    assert call(dt=3) == -1 and b"dtype" in lib.hstu_last_error()
    assert call(n=1 << 31) == -1 and b"n out of range" in lib.hstu_last_error()
    assert call(n=4) == -1 and b"workspace too small" in lib.hstu_last_error()
