"""CPU-side checks of the fused MIPS top-k and the research eval metrics: the C ABI exports and validates the new entry
points without a device, the workspace does not depend on the table, the Python layers import with the reference's
signatures, the fixtures under tests/golden/mips_topk/ regenerate bit for bit, and the metric formulas hold on a
hand-built ranking."""

import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from mips_topk_ref import FIXTURES, fixture_files, load_case

REFERENCE = "/root/reference/generative_recommenders"
NEW = ("hstu_mips_topk_workspace_bytes", "hstu_mips_topk")


@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_entry_points_declared_exported_and_bound(lib):
    from generative_recommenders_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hstu_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/hstu_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"libhstu_hip.so does not export {name}"
    assert lib.hstu_abi_version() == 13 and _lib.ABI_VERSION == 13        # purely additive


def test_workspace_depends_on_batch_and_k_only(lib):
    from generative_recommenders_amd import _lib

    assert len(_lib.SIGNATURES["hstu_mips_topk_workspace_bytes"][1]) == 2          # (batch, k): the table size is not an argument
    f = lib.hstu_mips_topk_workspace_bytes
    assert f(0, 10) == 0
    sizes_b = [f(b, 2711) for b in (1, 2, 63, 64, 65, 1024, 4096)]
    sizes_k = [f(1024, k) for k in (1, 2, 100, 2048, 2049, 4096)]
    assert sizes_b == sorted(sizes_b) and len(set(sizes_b)) == len(sizes_b)
    assert sizes_k == sorted(sizes_k) and len(set(sizes_k)) == len(sizes_k)
    assert f(1024, 2711) >= 1024 * (256 * 4 + 2711 * 8)                            # bins + candidates per row ...
    assert f(1024, 2711) <= 1024 * (256 * 4 + 2711 * 8 + 64)                       # ... and little else


def _args(**kw):
    a = dict(q=64, qrs=16, items=128, irs=16, scores=256, idx=512, ws=1024, batch=2, x=100, dim=16, k=5, dtype=0)
    a.update(kw)
    return [a["q"], a["qrs"], a["items"], a["irs"], a["scores"], a["idx"], a["ws"], a["batch"], a["x"], a["dim"], a["k"],
            a["dtype"], None]


@pytest.mark.parametrize("bad, text", [
    (dict(q=None), "non-NULL"), (dict(items=None), "non-NULL"), (dict(scores=None), "non-NULL"), (dict(idx=None), "non-NULL"),
    (dict(ws=None), "non-NULL"), (dict(x=0), "positive"), (dict(dim=0), "positive"), (dict(dim=-8), "positive"),
    (dict(batch=-1), "negative batch"), (dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"),
    (dict(dim=12, qrs=24, irs=24), "multiple of 8"), (dict(dtype=2, dim=6), "multiple of 4"),
    (dict(dim=520, qrs=520, irs=520), "exceeds the limit of 512"),
    (dict(k=0), "k must be in [1, min"), (dict(k=101), "k must be in [1, min"), (dict(x=5000, k=4097), "k must be in [1, min"),
    (dict(q=66), "16-byte aligned"), (dict(items=136), "16-byte aligned"), (dict(qrs=20), "16-byte aligned"),
    (dict(irs=17), "16-byte aligned"), (dict(ws=1028), "16-byte aligned"), (dict(qrs=8), "smaller than a row"),
])
def test_refuses_bad_arguments_before_any_launch(lib, bad, text):
    assert lib.hstu_mips_topk(*_args(**bad)) == -1      # HSTU_EINVAL; no device exists here, so nothing was launched
    assert text in lib.hstu_last_error().decode()


def test_k_equal_to_table_and_empty_batch_pass_validation(lib):
    # no device exists in this test: a launch would fail, HSTU_OK means none was attempted
    assert lib.hstu_mips_topk(*_args(batch=0)) == 0
    assert lib.hstu_mips_topk(*_args(batch=0, k=100, q=None, items=None, scores=None, idx=None, ws=None)) == 0


def test_python_layers_import_with_the_reference_signatures():
    from generative_recommenders_amd.research.data import eval as E
    from generative_recommenders_amd.research.indexing.candidate_index import CandidateIndex
    from generative_recommenders_amd.research.indexing.utils import get_top_k_module
    from generative_recommenders_amd.research.rails.indexing.candidate_index import TopKModule
    from generative_recommenders_amd.research.rails.indexing.mips_top_k import MIPSBruteForceTopK, MIPSTopKModule

    names = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert names(MIPSBruteForceTopK.__init__) == ["self", "item_embeddings", "item_ids"]
    assert names(MIPSBruteForceTopK.forward) == ["self", "query_embeddings", "k", "sorted", "kwargs"]
    assert names(CandidateIndex.__init__) == ["self", "ids", "embeddings", "invalid_ids", "debug_path"]
    assert names(CandidateIndex.get_top_k_outputs) == ["self", "query_embeddings", "k", "top_k_module", "invalid_ids", "r",
                                                       "return_embeddings"]
    assert names(CandidateIndex.filter_invalid_ids) == ["self", "invalid_ids"]
    assert names(get_top_k_module) == ["top_k_method", "model", "item_embeddings", "item_ids"]
    assert names(E.get_eval_state) == ["model", "all_item_ids", "negatives_sampler", "top_k_module_fn", "device", "float_dtype"]
    assert names(E.eval_metrics_v2_from_tensors) == ["eval_state", "model", "seq_features", "target_ids", "min_positive_rating",
                                                     "target_ratings", "epoch", "filter_invalid_ids", "user_max_batch_size", "dtype"]
    assert names(E.eval_recall_metrics_from_tensors) == ["eval_state", "model", "seq_features", "user_max_batch_size", "dtype"]
    assert names(E._avg) == ["x", "world_size"] and E.MAX_K == 2500
    assert issubclass(MIPSBruteForceTopK, MIPSTopKModule) and issubclass(MIPSTopKModule, TopKModule)
    with pytest.raises(TypeError):
        TopKModule()                                     # abstract

    emb, ids = torch.zeros(1, 7, 50, dtype=torch.bfloat16), torch.arange(1, 8).unsqueeze(0)
    module = get_top_k_module("MIPSBruteForceTopK", torch.nn.Identity(), emb, ids)
    assert isinstance(module, MIPSBruteForceTopK) and module._items.shape == (7, 56)         # padded once, in the constructor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        module(query_embeddings=torch.zeros(2, 50, dtype=torch.bfloat16), k=3)
    with pytest.raises(ValueError, match="MoLBruteForceTopK is not built"):
        get_top_k_module("MoLBruteForceTopK", torch.nn.Identity(), emb, ids)
    with pytest.raises(ValueError, match="Invalid top-k method"):
        get_top_k_module("nope", torch.nn.Identity(), emb, ids)
    c = CandidateIndex(ids=ids, embeddings=emb)
    assert c.num_objects == 7 and c.ids is ids and c.embeddings is emb
    assert float(E._avg(torch.tensor([1.0, 0.0, 0.0, 1.0]), 1)) == 0.5


def test_eval_module_does_not_import_tensorboard():
    code = ("import sys; import generative_recommenders_amd.research.data.eval; "
            "sys.exit(1 if any('tensorboard' in m for m in sys.modules) else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT, timeout=300).returncode == 0


def test_eval_code_reads_no_version_counter():
    pkg = os.path.join(ROOT, "generative_recommenders_amd", "research")
    for sub in ("rails/indexing/candidate_index.py", "rails/indexing/mips_top_k.py", "indexing/candidate_index.py", "indexing/utils.py",
                "data/eval.py"):
        assert "._version" not in open(os.path.join(pkg, sub)).read(), sub


# ---- the metric formulas on a hand-built ranking ---------------------------------------------------------------------------
class _StubTopK(torch.nn.Module):
    """returns the first k columns of a fixed (B, X) ranking"""

    def __init__(self, ranking):
        super().__init__()
        self.ranking = ranking

    def forward(self, query_embeddings, k, sorted=True, **kwargs):
        ids = self.ranking[:, :k]
        return -torch.arange(k, dtype=torch.float32).expand(ids.shape[0], -1), ids


class _StubModel(torch.nn.Module):
    def get_item_embeddings(self, ids):
        return torch.zeros(ids.shape + (4,))

    def encode(self, past_lengths, past_ids, past_embeddings, past_payloads):
        return torch.zeros(past_ids.shape[0], 4)


def test_metric_formulas_against_hand_computed_ranks(monkeypatch):
    from generative_recommenders_amd.research.data import eval as E
    from generative_recommenders_amd.research.indexing.candidate_index import CandidateIndex
    from generative_recommenders_amd.research.modeling.sequential.features import SequentialFeatures

    X = 3000
    corpus = torch.arange(1, X + 1)
    # rows: target first; target 10th; target 11th; target 2500th; target 2501st (absent: MAX_K + 1); target 3rd after filtering
    ranking = torch.stack([corpus.clone() for _ in range(6)])
    targets = torch.tensor([1, 10, 11, 2500, 2501, 5]).unsqueeze(1)
    past_ids = torch.zeros(6, 3, dtype=torch.int64)
    past_ids[5] = torch.tensor([2, 4, 0])               # row 5: ids 2 and 4 are filtered in front of the target 5 -> rank 3
    ranks = [1, 10, 11, 2500, E.MAX_K + 1, 3]
    state = E.EvalState(all_item_ids=set(corpus.tolist()), candidate_index=CandidateIndex(ids=corpus.unsqueeze(0), embeddings=torch.zeros(1, X, 4)),
                        top_k_module=_StubTopK(ranking))
    feats = SequentialFeatures(past_lengths=torch.tensor([1] * 5 + [2]), past_ids=past_ids, past_embeddings=None, past_payloads={})
    ratings = torch.tensor([5, 4, 3, 5, 1, 2]).unsqueeze(1)
    out = E.eval_metrics_v2_from_tensors(state, _StubModel(), feats, target_ids=targets, target_ratings=ratings, min_positive_rating=3)
    assert set(out) == ({f"ndcg@{n}" for n in (1, 10, 50, 100, 200)} | {f"hr@{n}" for n in (1, 10, 50, 100, 200, 500, 1000)} |
                        {"mrr", "ndcg@10_>=4", "hr@10_>=3", "hr@50_>=3", "mrr_>=3"})
    for n in (1, 10, 50, 100, 200, 500, 1000):
        assert out[f"hr@{n}"].tolist() == [r <= n for r in ranks], n
    for n in (1, 10, 50, 100, 200):
        want = [1.0 / math.log2(r + 1) if r <= n else 0.0 for r in ranks]
        assert out[f"ndcg@{n}"].shape == (6,) and np.allclose(out[f"ndcg@{n}"].numpy(), want, rtol=1e-6, atol=0), n
    assert np.allclose(out["mrr"].numpy(), [1.0 / r for r in ranks], rtol=1e-6, atol=0)
    assert np.allclose(out["ndcg@10_>=4"].numpy(), [1.0, 1.0 / math.log2(11), 0.0], rtol=1e-6, atol=0)      # rows 0, 1, 3
    assert out["hr@10_>=3"].tolist() == [True, True, False, False] and out["hr@50_>=3"].tolist() == [True, True, True, False]
    assert np.allclose(out["mrr_>=3"].numpy(), [1.0, 0.1, 1.0 / 11, 1.0 / 2500], rtol=1e-6, atol=0)
    assert all(v.is_inference() for v in out.values())                                                       # ran under inference mode

    # leave-one-out wrapper: the last column is the target and is not filtered as history
    loo = SequentialFeatures(past_lengths=torch.tensor([3, 3]), past_ids=torch.tensor([[1, 2, 3], [7, 1, 9]]), past_embeddings=None,
                             past_payloads={})
    state2 = E.EvalState(all_item_ids=set(corpus.tolist()), candidate_index=state.candidate_index, top_k_module=_StubTopK(ranking[:2]))
    out = E.eval_recall_metrics_from_tensors(state2, _StubModel(), loo)
    assert out["mrr"].tolist() == [1.0, pytest.approx(1.0 / 7)]      # row 0: 1, 2 filtered -> 3 is first; row 1: 1, 7 filtered -> 9 is 7th


# ---- fixtures --------------------------------------------------------------------------------------------------------------
def test_fixture_set_covers_the_required_cases():
    cases = [load_case(p) for p in fixture_files()]
    shapes = {(c["queries"].shape[0], c["items"].shape[0], c["items"].shape[1], int(c["k"]), c["invalid_ids"].shape[1]) for c in cases}
    assert shapes == {(5, 700, 50, 33, 7), (3, 4500, 64, 2500, 61), (17, 1000, 32, 1000, 0), (1, 1, 8, 1, 0), (2, 257, 16, 1, 0),
                      (64, 8195, 256, 300, 0)}
    for c in cases:
        assert c["queries"].dtype == np.int8 and c["items"].dtype == np.int8 and c["item_ids"].dtype == np.int64
        assert (c["item_ids"] > 0).all() and len(set(c["item_ids"].tolist())) == c["item_ids"].size
        assert not np.array_equal(c["item_ids"], np.arange(1, c["item_ids"].size + 1))
        assert int(c["k_prime"]) == min(int(c["k"]) + c["invalid_ids"].shape[1], c["items"].shape[0])
        s64 = c["queries"].astype(np.float64) @ c["items"].astype(np.float64).T
        assert np.abs(s64).max() <= 128
        for dt in ("float32", "bfloat16", "float16"):
            assert c[f"ref_scores_{dt}"].shape == (c["queries"].shape[0], int(c["k_prime"]))
            assert np.array_equal(c[f"ref_scores_{dt}"], -np.sort(-s64, axis=1)[:, : int(c["k_prime"])])
        if c["invalid_ids"].size:
            assert (c["invalid_ids"] == 0).any() and (c["invalid_ids"] > 0).any()
    for f in os.listdir(FIXTURES):
        assert os.path.getsize(os.path.join(FIXTURES, f)) < 1 << 20


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree (build container only)")
def test_mips_topk_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    res = subprocess.run([sys.executable, os.path.join(FIXTURES, "make_mips_topk_golden.py"), "--out", str(tmp_path)], cwd=ROOT,
                         env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    committed = sorted(f for f in os.listdir(FIXTURES) if f.endswith(".npz"))
    fresh = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert committed == fresh, f"fixture sets differ: committed {committed}, regenerated {fresh}"
    for f in committed:
        a, b = np.load(os.path.join(FIXTURES, f)), np.load(os.path.join(tmp_path, f))
        assert sorted(a.files) == sorted(b.files), f"{f}: array names differ"
        for key in a.files:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, f"{f}:{key} dtype / shape"
            assert np.array_equal(a[key], b[key]), f"{f}:{key} is not reproduced bit for bit"
