"""CPU-side checks of the Mixture-of-Logits similarity: the C ABI declares, exports and binds ``hstu_mol_scores`` and
refuses shapes outside its limits without a device, the Python layers carry the reference's parameter names and debug
strings (so its ``state_dict`` loads), the composite path reproduces the reference's fp64 forward on the CPU, the fused
path refuses CPU tensors, ``get_top_k_module`` still refuses a model without MoL, and the fixtures regenerate bit for
bit."""

import copy
import os
import re
import subprocess
import sys

import pytest
import torch

import mol_golden as G
from conftest import ROOT

REFERENCE = "/root/reference/generative_recommenders"
HSTU_EUNSUPPORTED = -2


@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _module(case):
    from generative_recommenders_amd.research.modeling.similarity_utils import create_mol_interaction_module

    module, debug_str = create_mol_interaction_module(**G.factory_kwargs(*case[:5]))
    return module, debug_str


def test_entry_point_declared_exported_and_bound(lib):
    from generative_recommenders_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hstu_hip.h")).read(), flags=re.S)
    assert re.search(r"\bhstu_mol_scores\s*\(", header), "hstu_mol_scores is not declared in include/hstu_hip.h"
    assert "hstu_mol_scores" in _lib.SIGNATURES and hasattr(lib, "hstu_mol_scores")
    for macro, value in (("HSTU_MOL_MAX_LOGITS", 64), ("HSTU_MOL_MAX_DIM", 128), ("HSTU_MOL_MAX_HIDDEN", 256)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", header), macro


def test_abi_version_is_unchanged(lib):
    from generative_recommenders_amd import _lib

    assert _lib.ABI_VERSION == 13 and lib.hstu_abi_version() == 13


@pytest.mark.parametrize("pq,px,dim,hidden,word", [(5, 13, 32, 128, "logits"), (8, 8, 129, 128, "dimension"), (8, 8, 136, 128, "dimension"),
                                                   (8, 8, 32, 257, "hidden"), (0, 8, 32, 128, "logits"), (8, 8, 12, 0, "dimension")])
def test_library_refuses_shapes_outside_its_limits_before_any_launch(lib, pq, px, dim, hidden, word):
    """the limits are judged before the pointers are looked at: no device is needed (or touched)"""
    rc = lib.hstu_mol_scores(None, None, None, None, None, None, None, None, None, 4, 100, pq, px, dim, hidden, 20.0, 0, 2, None)
    assert rc == HSTU_EUNSUPPORTED
    assert word in lib.hstu_last_error().decode()


def test_python_layer_names_the_limit():
    from generative_recommenders_amd.ops import mol

    mol.mol_check_limits(8, 8, 128, 256)
    mol.mol_check_limits(1, 1, 1, 0)
    with pytest.raises(ValueError, match=r"P_Q \* P_X <= 64"):
        mol.mol_check_limits(5, 13, 32, 128)
    with pytest.raises(ValueError, match=r"D_P <= 128"):
        mol.mol_check_limits(8, 8, 129, 128)
    with pytest.raises(ValueError, match=r"H <= 256"):
        mol.mol_check_limits(8, 8, 32, 257)
    assert mol.mol_pad_components(torch.ones(3, 5, 10)).shape == (3, 5, 16)
    assert torch.equal(mol.mol_pad_components(torch.ones(3, 5, 10))[..., 10:], torch.zeros(3, 5, 6))


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_state_dict_names_and_debug_string_are_the_references(case):
    fixture, state_dict = G.load_module_fixture(case)
    module, debug_str = _module(case)
    assert list(module.state_dict().keys()) == list(state_dict.keys())
    assert {k: tuple(v.shape) for k, v in module.state_dict().items()} == {k: tuple(v.shape) for k, v in state_dict.items()}
    assert debug_str == str(fixture["debug_str"][()])
    module.load_state_dict(state_dict)


@pytest.mark.parametrize("case", G.CASES[:3], ids=G.case_id)
def test_composite_path_reproduces_the_reference_in_fp64_on_the_cpu(case):
    """the composite path is plain torch: in fp64 on the CPU it must agree with the reference's own fp64 forward, its
    ``mi_loss`` and its gradient to rounding"""
    fixture, state_dict = G.load_module_fixture(case)
    module, _ = _module(case)
    module.load_state_dict(state_dict)
    m64 = copy.deepcopy(module).double().train()
    queries = torch.from_numpy(fixture["queries"]).double().requires_grad_(True)
    scores, aux = m64(queries, torch.from_numpy(fixture["items"]).double())
    (grad,) = torch.autograd.grad(scores.sum(), queries)
    s64 = torch.from_numpy(fixture["s64"])
    assert (scores.detach() - s64).abs().max().item() <= 1e-12 * max(1.0, s64.abs().max().item())
    assert abs(aux["mi_loss"].item() - float(fixture["mi_loss"][()])) <= 1e-12
    ref_grad = torch.from_numpy(fixture["grad_queries"])
    assert (grad - ref_grad).norm().item() <= 1e-10 * ref_grad.norm().item()


def test_path_rule():
    case = G.CASES[1]
    module, _ = _module(case)
    items, per_query_items = torch.zeros(1, 7, G.ITEM_DIM), torch.zeros(3, 7, G.ITEM_DIM)
    module.eval()
    with torch.no_grad():
        assert module.fused_path_applies(items)
        assert not module.fused_path_applies(per_query_items)              # B' = B
    assert not module.fused_path_applies(items)                            # autograd is recording
    module.train()
    with torch.no_grad():
        assert not module.fused_path_applies(items)                        # dropout / mi_loss
        module.eval()
        module._gating_fn._combination_type = "none"
        assert not module.fused_path_applies(items)
        module._gating_fn._combination_type = "glu_silu"
        module._gating_fn._qi_partial_module = torch.nn.Linear(8, 8)       # not the factory's Sequential
        assert not module.fused_path_applies(items)


def test_fused_path_refuses_cpu_tensors():
    module, _ = _module(G.CASES[1])
    module.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        module(torch.zeros(2, G.QUERY_DIM), torch.zeros(1, 7, G.ITEM_DIM))


def test_get_similarity_function_dispatch():
    from generative_recommenders_amd.research.modeling.similarity_utils import get_similarity_function
    from generative_recommenders_amd.research.rails.similarities.dot_product_similarity_fn import DotProductSimilarity
    from generative_recommenders_amd.research.rails.similarities.mol.similarity_fn import MoLSimilarity

    module, debug_str = get_similarity_function("DotProduct", query_embedding_dim=8, item_embedding_dim=8)
    assert isinstance(module, DotProductSimilarity) and debug_str == "DotProduct"
    kw = G.factory_kwargs(4, 2, 16, 16, "glu_silu")
    for name in ("query_embedding_dim", "item_embedding_dim", "bf16_training"):
        kw.pop(name)
    module, debug_str = get_similarity_function("MoL", query_embedding_dim=G.QUERY_DIM, item_embedding_dim=G.ITEM_DIM, bf16_training=True, **kw)
    assert isinstance(module, MoLSimilarity) and module._autocast_bf16 and debug_str.startswith("MoL-4x2x16-t0.05")
    with pytest.raises(ValueError, match="Unknown interaction_module_type Cosine"):
        get_similarity_function("Cosine", query_embedding_dim=8, item_embedding_dim=8)


def test_top_k_helper_still_refuses_a_model_without_mol():
    from generative_recommenders_amd.research.indexing.utils import get_top_k_module

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._ndp_module = torch.nn.Identity()

    for model in (torch.nn.Identity(), Model()):
        with pytest.raises(ValueError, match="MoLBruteForceTopK is not built"):
            get_top_k_module("MoLBruteForceTopK", model, torch.zeros(1, 4, 8), torch.arange(4).unsqueeze(0))


def test_sampled_softmax_still_refuses_mol():
    from generative_recommenders_amd.research.modeling.sequential.losses.sampled_softmax import SampledSoftmaxLoss

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._ndp_module = _module(G.CASES[1])[0]

    with pytest.raises(NotImplementedError, match="dot-product similarity only"):     # training with the fused loss on MoL: out of scope
        SampledSoftmaxLoss(num_to_sample=4, softmax_temperature=0.05, model=Model())(
            torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 8), torch.ones(2), negatives_sampler=None)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree (build container only)")
def test_mol_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    res = subprocess.run([sys.executable, os.path.join(G.GOLDEN, "make_mol_golden.py"), "--out", str(tmp_path)], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    committed = sorted(f for f in os.listdir(G.GOLDEN) if f.endswith(".npz"))
    assert committed == sorted(os.listdir(tmp_path)) and committed
    for f in committed:
        assert open(os.path.join(G.GOLDEN, f), "rb").read() == open(os.path.join(tmp_path, f), "rb").read(), f
