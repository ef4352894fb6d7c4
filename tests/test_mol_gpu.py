"""GPU checks of the Mixture-of-Logits similarity against the fixtures of tests/golden/mol (minted from the reference).

The gates are margins over the REFERENCE's own error on the same operands, ``e_ref = max |reference at T - fp64|``:

* op level, fp32: ``16 e_ref(fp32)`` -- both errors are the same first-order quantity; an order of magnitude covers another
  accumulation order and the hardware exp2 / rcp; a wrong term shows at 1e-2 max|s|, four orders above;
* op level, 16-bit: ``e_ref(T)`` plus half an ulp of the op's output dtype (fp32) at |s| -- the kernel keeps fp32 where the
  reference rounds every intermediate;
* module level, fp32: ``64 e_ref(fp32)`` -- the upstream projections run as GPU GEMMs in another order, and their
  differences are multiplied by 1 / temperature = 20 before the gate.

Every measured error goes through ``record_parity`` with its error / gate ratio."""

import numpy as np
import pytest
import torch

import mol_golden as G
from conftest import record_parity

pytestmark = pytest.mark.gpu
DTYPE_NAMES = ("float32", "bfloat16", "float16")


@pytest.fixture(scope="module")
def dev():
    from generative_recommenders_amd import _lib

    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.lib()
    return torch.device("cuda")


def _op(ops, dev, rows=None):
    from generative_recommenders_amd.ops import mol

    t = {k: (v.to(dev) if v is not None else None) for k, v in ops.items()}
    if rows is not None:
        t["qc"], t["gq"] = t["qc"][rows].contiguous(), t["gq"][rows].contiguous()
    return t, lambda comb: mol.mol_scores(t["qc"], t["xc"], t["gq"], t["gi"], t["w1"], t["b1"], t["w2"], t["b2"], G.TEMPERATURE, comb)


def _half_ulp_fp32(s64):
    return 0.5 * torch.exp2(torch.floor(torch.log2(s64.abs().clamp_min(1e-30))) - 23)


def _check(what, got, s64, gate, dtype_name):
    """per element |got - s64| <= gate (a number or a tensor); the measured error and its ratio to the gate are recorded"""
    got = got.detach().double().cpu()
    assert got.shape == s64.shape and torch.isfinite(got).all()
    err = (got - s64).abs()
    ratio = float((err / gate).max()) if err.numel() else 0.0
    record_parity(what, got.numpy(), s64.numpy(), dtype_name, max_abs_err=float(err.max()), gate=float(torch.as_tensor(gate).max()),
                  err_over_gate=ratio)
    print(f"{what} [{dtype_name}]: max |err| {float(err.max()):.3e}  gate {float(torch.as_tensor(gate).max()):.3e}  err/gate {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: error / gate = {ratio:.3f}"
    return ratio


# --------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("dtype_name", DTYPE_NAMES)
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_op_matches_fp64_within_the_references_own_error(dev, case, dtype_name):
    ops, _, s64, e_ref = G.load_operands(case, dtype_name)
    _, run = _op(ops, dev)
    out = run(case[4])
    assert out.dtype == torch.float32 and out.shape == s64.shape
    gate = 16 * e_ref if dtype_name == "float32" else e_ref + _half_ulp_fp32(s64)
    _check(f"mol_scores {G.case_id(case)}", out, s64, gate, dtype_name)
    assert torch.equal(run(case[4]), out), "two calls differ"


@pytest.mark.parametrize("dtype_name", DTYPE_NAMES)
def test_op_single_query(dev, dtype_name):
    case = G.CASES[3]
    ops, _, s64, e_ref = G.load_operands(case, dtype_name)
    _, run = _op(ops, dev, rows=slice(2, 3))
    gate = 16 * e_ref if dtype_name == "float32" else e_ref + _half_ulp_fp32(s64[2:3])
    _check(f"mol_scores B=1 {G.case_id(case)}", run(case[4]), s64[2:3], gate, dtype_name)


def _torch_eval(t, comb, dtype):
    """the formula of the op in plain torch at ``dtype``, on the device the operands are on"""
    c = {k: (v.to(dtype) if v is not None else None) for k, v in t.items()}
    L = c["gq"].shape[1]
    logits = torch.einsum("bnd,xmd->bxnm", c["qc"], c["xc"]).reshape(c["qc"].shape[0], c["xc"].shape[0], L) / G.TEMPERATURE
    if c["w2"] is not None:
        mlp = torch.nn.functional.silu(logits @ c["w1"].t() + c["b1"]) @ c["w2"].t() + c["b2"]
    else:
        mlp = logits @ c["w1"].t() + c["b2"]
    g = c["gq"].unsqueeze(1) * c["gi"].unsqueeze(0) + mlp
    arg = g if comb == "glu_silu" else torch.nn.functional.layer_norm(g, [L])
    return (torch.softmax(g * torch.sigmoid(arg), dim=-1) * logits).sum(-1)


# shapes at which the kernel takes another path than in the fixtures: fp32 weights staged in two chunks of hidden units
# (L = 64, H = 256), 16 column tiles per wave (P_X = 64), 8 row tiles (P_Q = 64), the largest dot product dimension
@pytest.mark.parametrize("pq,px,dp,h,comb,dtype_name", [(8, 8, 24, 256, "glu_silu_ln", "float32"), (1, 64, 8, 40, "glu_silu", "float32"),
                                                        (64, 1, 128, 0, "glu_silu", "float32"), (2, 32, 128, 256, "glu_silu", "bfloat16")])
def test_op_other_kernel_paths(dev, pq, px, dp, h, comb, dtype_name):
    """operands drawn here; the same gates, with e_ref = the error of the plain torch evaluation at the operands' dtype
    (fp32 operands: fp32 on the CPU) against its fp64 evaluation"""
    B, X, L = 6, 70, pq * px
    dt = G.DTYPES[dtype_name]
    t = _draw_operands(B, X, pq, px, dp, h, dt, 7 + L + h)
    s64 = _torch_eval(t, comb, torch.float64)
    e_ref = float((_torch_eval(t, comb, torch.float32 if dt == torch.float32 else dt).double() - s64).abs().max())
    _, run = _op(t, dev)
    gate = 16 * e_ref if dtype_name == "float32" else e_ref + _half_ulp_fp32(s64)
    _check(f"mol_scores {pq}x{px}x{dp} h{h} {comb}", run(comb), s64, gate, dtype_name)


def _draw_operands(B, X, pq, px, dp, h, dt, seed):
    L = pq * px
    g = torch.Generator().manual_seed(seed)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, generator=g), dim=-1)      # noqa: E731
    t = {"qc": unit(B, pq, dp), "xc": unit(X, px, dp), "gq": torch.randn(B, L, generator=g), "gi": torch.randn(X, L, generator=g),
         "w1": torch.randn(h if h else L, L, generator=g) * (2.0 / (L + max(h, L))) ** 0.5, "b1": torch.randn(h, generator=g) * 0.2 if h else None,
         "w2": torch.randn(L, h, generator=g) * (2.0 / (L + h)) ** 0.5 if h else None, "b2": torch.randn(L, generator=g) * 0.2}
    return {k: (v.to(dt) if v is not None else None) for k, v in t.items()}


def _tiles_per_workgroup(B, X):
    """launch_mol_t's rule (csrc/mol_ops.hip): 32-item tiles a workgroup walks"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    q_groups, n_tiles = -(-B // 4), -(-X // 32)
    splits = max(1, min(n_tiles, 8 * cus // q_groups))
    return -(-n_tiles // splits)


# the regime the kernel exists for: a workgroup walks SEVERAL item tiles, so the waves' logit tiles in LDS are rewritten, the
# rows of gi refilled and -- fp32, 8 x 8, H = 256 -- the two weight chunks restaged tile after tile.  References: the
# torch evaluation above in fp64 and at the operands' dtype, both on the GPU (563,200 pairs)
@pytest.mark.parametrize("pq,px,dp,h,comb,dtype_name", [(3, 5, 16, 40, "glu_silu_ln", "float32"), (8, 8, 32, 256, "glu_silu", "float32"),
                                                        (8, 8, 32, 128, "glu_silu", "bfloat16"), (4, 2, 16, 0, "glu_silu", "float16")])
def test_op_several_tiles_per_workgroup(dev, pq, px, dp, h, comb, dtype_name):
    B, X = 512, 1100
    assert _tiles_per_workgroup(B, X) > 1, "this shape no longer makes a workgroup walk more than one tile"
    t = {k: (v.to(dev) if v is not None else None) for k, v in _draw_operands(B, X, pq, px, dp, h, G.DTYPES[dtype_name], 11 + h).items()}
    s64 = _torch_eval(t, comb, torch.float64).cpu()
    e_ref = float((_torch_eval(t, comb, G.DTYPES[dtype_name]).double().cpu() - s64).abs().max())
    _, run = _op(t, dev)
    gate = 16 * e_ref if dtype_name == "float32" else e_ref + _half_ulp_fp32(s64)
    out = run(comb)
    _check(f"mol_scores several tiles {pq}x{px}x{dp} h{h} {comb}", out, s64, gate, dtype_name)
    assert torch.equal(run(comb), out), "two calls differ"


def test_op_batch_beyond_one_launch(dev):
    """more than 4 x 2^20 queries run as several launches over rows of qc, gq and out (a grid of 2^32 threads is the
    runtime's limit): the queries around the seam and the last ones against fp64"""
    B, X, pq, px, dp = (4 << 20) + 5, 3, 2, 2, 8
    t = {k: (v.to(dev) if v is not None else None) for k, v in _draw_operands(B, X, pq, px, dp, 0, torch.float32, 5).items()}
    s64 = _torch_eval(t, "glu_silu", torch.float64).cpu()
    e_ref = float((_torch_eval(t, "glu_silu", torch.float32).double().cpu() - s64).abs().max())
    _, run = _op(t, dev)
    _check("mol_scores B = 4 x 2^20 + 5", run("glu_silu"), s64, 16 * e_ref, "float32")


@pytest.mark.parametrize("pq,px,dp,h", [(5, 13, 32, 128), (8, 8, 129, 128), (8, 8, 32, 257)])
def test_op_refuses_shapes_outside_its_limits(dev, pq, px, dp, h):
    from generative_recommenders_amd.ops import _launch, mol

    L = pq * px
    z = lambda *s: torch.zeros(*s, device=dev)      # noqa: E731
    args = (z(2, pq, dp), z(3, px, dp), z(2, L), z(3, L), z(h, L), z(h), z(L, h), z(L))
    with pytest.raises(RuntimeError, match="libhstu_hip error -2"):
        _launch.mol_scores(*args, 20.0, "glu_silu")
    with pytest.raises(ValueError, match="limit"):
        mol.mol_scores(*args, G.TEMPERATURE, "glu_silu")


# --------------------------------------------------------------------------------------------------------------- module level
def _module(case, dev, dtype=torch.float32):
    from generative_recommenders_amd.research.modeling.similarity_utils import create_mol_interaction_module

    fixture, state_dict = G.load_module_fixture(case)
    module, _ = create_mol_interaction_module(**G.factory_kwargs(*case[:5]))
    module.load_state_dict(state_dict)
    module = module.to(device=dev, dtype=dtype).eval()
    tensor = lambda name: torch.from_numpy(fixture[name]).to(dev)      # noqa: E731
    return module, fixture, tensor("queries").to(dtype), tensor("items").to(dtype), tensor("item_ids")


def _module_gate(case):
    return 64 * G.load_operands(case, "float32")[3]


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_module_fused_and_composite_paths(dev, case):
    module, fixture, queries, items, _ = _module(case, dev)
    s64, gate = torch.from_numpy(fixture["s64"]), _module_gate(case)
    with torch.no_grad():
        assert module.fused_path_applies(items)
        fused, aux = module(queries, items)
    assert fused.dtype == torch.float32 and aux == {}
    _check(f"MoLSimilarity fused {G.case_id(case)}", fused, s64, gate, "float32")
    assert not module.fused_path_applies(items)                # autograd is recording: the composite path
    composite, aux = module(queries, items)
    assert aux == {}
    _check(f"MoLSimilarity composite {G.case_id(case)}", composite, s64, gate, "float32")


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_module_training_path_loss_and_gradient(dev, case):
    module, fixture, queries, items, _ = _module(case, dev)
    module.train()                                             # every dropout rate of the fixtures' modules is 0
    queries.requires_grad_(True)
    scores, aux = module(queries, items)
    _check(f"MoLSimilarity train {G.case_id(case)}", scores, torch.from_numpy(fixture["s64"]), _module_gate(case), "float32")
    mi64 = float(fixture["mi_loss"][()])
    mi = float(aux["mi_loss"].detach())
    mi_err = abs(mi - mi64)
    print(f"mi_loss {mi:.9g} vs {mi64:.9g}: relative error {mi_err / max(abs(mi64), 1e-300):.3e}, gate {_module_gate(case):.3e}")
    assert mi_err <= _module_gate(case) * abs(mi64)
    (grad,) = torch.autograd.grad(scores.sum(), queries)
    ref = torch.from_numpy(fixture["grad_queries"])
    m = record_parity(f"MoLSimilarity d scores.sum() / d queries {G.case_id(case)}", grad.double().cpu().numpy(), ref.numpy(), "float32")
    assert m["rel_fro"] <= 1e-4, m


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_module_bf16_fused_returns_bf16(dev, case):
    """recorded, not gated beyond the op-level test: the operands differ from the fixture's (GPU GEMMs in bf16)"""
    module, _, queries, items, _ = _module(case, dev, torch.bfloat16)
    with torch.no_grad():
        scores, _ = module(queries, items)
    assert scores.dtype == torch.bfloat16 and torch.isfinite(scores).all()
    s64 = G.load_operands(case, "bfloat16")[2]
    record_parity(f"MoLSimilarity fused bf16 {G.case_id(case)}", scores.double().cpu().numpy(), s64.numpy(), "bfloat16")


def test_module_autocast_bf16_returns_bf16(dev):
    case = G.CASES[1]
    module, fixture, queries, items, _ = _module(case, dev)
    module._autocast_bf16 = True
    with torch.no_grad():
        scores, _ = module(queries, items)
    assert scores.dtype == torch.bfloat16
    s64 = torch.from_numpy(fixture["s64"])
    assert float((scores.double().cpu() - s64).abs().max()) < 0.1 * float(s64.abs().max())      # the fixtures' bound on a 16-bit error


def test_module_names_the_limit(dev):
    from generative_recommenders_amd.research.modeling.similarity_utils import create_mol_interaction_module

    module, _ = create_mol_interaction_module(**G.factory_kwargs(5, 13, 16, 16, "glu_silu"))
    module = module.to(dev).eval()
    with torch.no_grad(), pytest.raises(ValueError, match=r"P_Q \* P_X <= 64"):
        module(torch.zeros(2, G.QUERY_DIM, device=dev), torch.zeros(1, 9, G.ITEM_DIM, device=dev))


# --------------------------------------------------------------------------------------------------------------- top-k
@pytest.mark.parametrize("case", G.CASES[1:], ids=G.case_id)
def test_brute_force_top_k(dev, case):
    from generative_recommenders_amd.research.indexing.utils import get_top_k_module
    from generative_recommenders_amd.research.rails.indexing.mol_top_k import MoLBruteForceTopK

    module, fixture, queries, items, item_ids = _module(case, dev)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._ndp_module = module

    top_k = get_top_k_module("MoLBruteForceTopK", Model(), items, item_ids)
    assert isinstance(top_k, MoLBruteForceTopK) and top_k.mol_module is module
    s64, gate, X = fixture["s64"], _module_gate(case), case[6]
    ids_np = fixture["item_ids"][0]
    pos_of = {int(i): p for p, i in enumerate(ids_np)}
    for k in (1, 10, min(X, 300)):
        scores, ids = top_k(queries, k=k)
        assert scores.shape == (case[5], k) and ids.shape == (case[5], k) and ids.dtype == item_ids.dtype
        scores, ids = scores.double().cpu().numpy(), ids.cpu().numpy()
        assert (np.diff(scores, axis=1) <= 0).all(), "scores are not descending"
        for b in range(case[5]):
            assert len(set(ids[b].tolist())) == k and all(int(i) in pos_of for i in ids[b]), "ids are not distinct members of item_ids"
            pos = np.array([pos_of[int(i)] for i in ids[b]])
            assert np.abs(scores[b] - s64[b, pos]).max() <= gate
            omitted = np.ones(X, dtype=bool)
            omitted[pos] = False
            if omitted.any():
                assert s64[b, omitted].max() <= s64[b, pos].min() + 2 * gate, "an omitted item scores above the returned ones"


def test_brute_force_top_k_chunks_queries(dev):
    """the chunk rule itself: with a 1-row score buffer every query is its own chunk, and the result does not change"""
    from generative_recommenders_amd.research.rails.indexing.mol_top_k import MoLBruteForceTopK

    module, _, queries, items, item_ids = _module(G.CASES[1], dev)
    top_k = MoLBruteForceTopK(module, items, item_ids)
    whole = top_k(queries, k=7)
    top_k.SCORE_BUFFER_BYTES = 4 * items.shape[1]
    by_row = top_k(queries, k=7)
    assert torch.equal(whole[0], by_row[0]) and torch.equal(whole[1], by_row[1])


# --------------------------------------------------------------------------------------------------------------- memory
def test_fused_forward_never_holds_a_b_x_l_tensor(dev):
    """the capability claim: B = 64 queries against X = 20,000 items at L = 64, H = 128 in bf16 grow the allocator's peak by
    less than 4 (B, X) fp32 tensors + 8 MiB (about 28 MB), where ONE (B, X, L) fp32 tensor is 328 MB"""
    from generative_recommenders_amd.research.modeling.similarity_utils import create_mol_interaction_module

    B, X = 64, 20000
    module, _ = create_mol_interaction_module(**G.factory_kwargs(8, 8, 32, 128, "glu_silu"))
    module = module.to(device=dev, dtype=torch.bfloat16).eval()
    queries = torch.randn(B, G.QUERY_DIM, device=dev, dtype=torch.bfloat16)
    items = torch.randn(1, X, G.ITEM_DIM, device=dev, dtype=torch.bfloat16)
    with torch.no_grad():
        module(queries[:2], items[:, :64])                      # library load, first-use allocations
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        scores, _ = module(queries, items)
        torch.cuda.synchronize()
        growth = torch.cuda.max_memory_allocated() - before
    assert scores.shape == (B, X) and torch.isfinite(scores).all()
    print(f"peak growth {growth / 2**20:.1f} MiB, bound {(4 * B * X * 4 + (8 << 20)) / 2**20:.1f} MiB")
    assert growth < 4 * B * X * 4 + (8 << 20)
