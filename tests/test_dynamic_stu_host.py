"""CPU tests of modules/dynamic_stu.py with a stub inner STU (records its keyword arguments, returns x + 1): SDSTU's skip
decisions, what it hands the wrapped STU on a skip, the untouched RNG state and the call counter; DynamicSTU is abstract."""

import pytest
import torch

from generative_recommenders_amd.modules.dynamic_stu import DynamicSTU, L2STU, SDSTU
from generative_recommenders_amd.modules.stu import STU

D = 6


class StubSTU(STU):
    def __init__(self):
        super().__init__(is_inference=False)
        self.calls = []
        self._marker = 0

    def forward(self, x, x_lengths, x_offsets, max_seq_len, num_targets, max_kv_caching_len=0, kv_caching_lengths=None):
        self.calls.append(dict(x=x, x_lengths=x_lengths, x_offsets=x_offsets, max_seq_len=max_seq_len, num_targets=num_targets,
                               max_kv_caching_len=max_kv_caching_len, kv_caching_lengths=kv_caching_lengths))
        return x + 1


def _batch():
    lengths = torch.tensor([3, 0, 5], dtype=torch.int64)
    offsets = torch.tensor([0, 3, 3, 8], dtype=torch.int64)
    x = torch.randn(8, D, dtype=torch.float64)
    nt = torch.tensor([1, 0, 2], dtype=torch.int64)
    return dict(x=x, x_lengths=lengths, x_offsets=offsets, max_seq_len=7, num_targets=nt)


def _run(sd, stub, n=20):
    """n calls; per call (skipped, rng untouched)"""
    out = []
    for _ in range(n):
        b = _batch()
        before = torch.get_rng_state()
        y = sd(**b)
        assert torch.equal(torch.get_rng_state(), before), "the caller's RNG state moved"
        seen = stub.calls[-1]
        skipped = y is b["x"]
        if skipped:
            assert seen["x"].shape == (0, D) and seen["x"].dtype == b["x"].dtype
            assert seen["x_lengths"].shape == b["x_lengths"].shape and seen["x_lengths"].dtype == b["x_lengths"].dtype
            assert seen["x_offsets"].shape == b["x_offsets"].shape and seen["x_offsets"].dtype == b["x_offsets"].dtype
            assert not seen["x_lengths"].any() and not seen["x_offsets"].any()
            assert seen["max_seq_len"] == 1
        else:
            assert torch.equal(y, b["x"] + 1)
            assert seen["x"] is b["x"] and seen["x_lengths"] is b["x_lengths"] and seen["x_offsets"] is b["x_offsets"]
            assert seen["max_seq_len"] == 7
        assert seen["num_targets"] is b["num_targets"] and seen["max_kv_caching_len"] == 0 and seen["kv_caching_lengths"] is None
        assert sd._skip_x is None
        out.append(skipped)
    assert len(stub.calls) == n                       # the wrapped STU is called on a skip too
    return out


def test_sdstu_skip_decisions_match_an_independent_replay():
    stub = StubSTU()
    sd = SDSTU(stub, is_inference=False, dropout_ratio=0.3, seed=3).train()
    assert (sd._stu is stub, sd._dropout_ratio, sd._iter, sd._seed, sd._skip_x) == (True, 0.3, 0, 3, None)
    got = _run(sd, stub)
    state = torch.get_rng_state()
    want = []
    for i in range(20):
        torch.manual_seed(i + 3)
        want.append(torch.rand(1).item() <= 0.3)
    torch.set_rng_state(state)
    assert got == want
    assert any(want) and not all(want), "seed 3 / ratio 0.3 must show both outcomes in 20 draws"
    assert sd._iter == 20


def test_sdstu_ratio_one_always_skips_ratio_zero_never_and_eval_never():
    stub = StubSTU()
    sd = SDSTU(stub, is_inference=False, dropout_ratio=1.0, seed=3).train()
    assert all(_run(sd, stub)) and sd._iter == 20
    stub = StubSTU()
    sd = SDSTU(stub, is_inference=False, dropout_ratio=0.0, seed=3).train()
    assert not any(_run(sd, stub)) and sd._iter == 20
    stub = StubSTU()
    sd = SDSTU(stub, is_inference=False, dropout_ratio=1.0, seed=3).eval()
    assert not any(_run(sd, stub)) and sd._iter == 0            # eval never skips and does not count


def test_kv_arguments_pass_through():
    stub = StubSTU()
    sd = SDSTU(stub, is_inference=False, dropout_ratio=1.0).train()
    b = _batch()
    kv = torch.tensor([1, 0, 2])
    assert sd(**b, max_kv_caching_len=9, kv_caching_lengths=kv) is b["x"]
    assert stub.calls[-1]["max_kv_caching_len"] == 9 and stub.calls[-1]["kv_caching_lengths"] is kv


def test_dynamic_stu_is_abstract_and_constructors_are_the_references():
    with pytest.raises(TypeError, match="abstract"):
        DynamicSTU(StubSTU(), is_inference=False)
    l2 = L2STU(StubSTU(), max_l2_len=8, is_inference=True, contextual_seq_len=3)
    assert (l2._max_l2_len, l2._contextual_seq_len, l2._saved_tensors, l2._runtime_max_l2_len, l2._runtime_prefix_len) == (8, 3, None, 0, 0)
    assert l2.is_inference and L2STU(StubSTU(), 4, False)._contextual_seq_len == 0
    sd = SDSTU(StubSTU(), False)
    assert (sd._dropout_ratio, sd._seed) == (0.5, 0)
    assert issubclass(SDSTU, DynamicSTU) and issubclass(L2STU, DynamicSTU) and issubclass(DynamicSTU, STU)


def test_recursive_setattr_reaches_the_wrapped_stu():
    stub = StubSTU()
    outer = L2STU(SDSTU(stub, is_inference=False), max_l2_len=4, is_inference=False)
    outer.recursive_setattr("_marker", 5)
    assert stub._marker == 5
    outer.set_is_inference(True)
    assert stub.is_inference and outer._stu.is_inference and outer.is_inference
    assert [n for n, _ in outer.named_modules()] == ["", "_stu", "_stu._stu"]


def test_fx_infer_max_len():
    from generative_recommenders_amd.common import fx_infer_max_len

    v = fx_infer_max_len(torch.tensor([3, 9, 0]))
    assert v == 9 and type(v) is int
