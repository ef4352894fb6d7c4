"""The research-path model parts on the GPU.

* The fused input preprocessor (``research_input_preprocess``, three layouts) against the fixtures minted from the
  reference's modules: fp32 with dropout off is bit-identical in ``out``, ``valid_mask`` and ``d_past_embeddings``; the table
  gradients and everything in bf16 pass the project's gate ``e_hip <= m * e_ref`` (both relative Frobenius errors against the
  fp64 truth, ``multitask_ref.gate_multiplier``; the ratios are printed and recorded).  Untouched table rows are exactly zero
  and two backward calls agree bit for bit.
* Dropout against ``oracle.hstu_oracle.dropout_keep_mask``: the forward equals ``where(keep, fl(out_p0 * scale), 0)`` and the
  backward uses the same mask, bit for bit.
* A batch of 300 users (several slabs of users, the second reduction step) against the composition in torch ops on the
  device: forward bit-exact, gradients within the bound of an fp32 sum in any order against the fp64 composition.
* The modules: the reference's state_dict loads with ``strict=True``; preprocessors and postprocessors pass the same checks.
* ``HSTU`` and ``SASRec`` built from this package's modules only, against the reference models built from the reference's."""

import numpy as np
import pytest
import torch

import research_modules_ref as R
from conftest import record_parity
from oracle.hstu_oracle import dropout_keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYOUT = {"plain": 0, "concat": 1, "interleave": 2}


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def same_bits(t, ref):
    """t (tensor) equals ref (numpy array of the same float type) bit for bit"""
    ref = np.ascontiguousarray(ref)
    return tuple(t.shape) == ref.shape and np.array_equal(bits(t), ref.view(np.int16 if ref.itemsize == 2 else np.int32))


def _inputs(z, dtype):
    t = dict(ids=torch.from_numpy(z["past_ids"]).to(DEV), ratings=torch.from_numpy(z["ratings"]).to(DEV),
             emb=torch.from_numpy(z["past_embeddings"]).to(DEV).to(dtype).requires_grad_(True),
             pos=torch.from_numpy(z["sd:_pos_emb.weight"]).to(DEV).to(dtype).requires_grad_(True),
             r=torch.from_numpy(z["r"]).to(DEV).to(dtype))
    t["rat"] = (torch.from_numpy(z["sd:_rating_emb.weight"]).to(DEV).to(dtype).requires_grad_(True)
                if "sd:_rating_emb.weight" in z else None)
    return t


def _run_op(z, t, p=0.0, seed=0):
    from generative_recommenders_amd.ops.research_preprocess import research_input_preprocess

    kind = str(z["kind"])
    return research_input_preprocess(t["ids"], t["emb"], t["pos"], layout=LAYOUT[kind], ratings=t["ratings"] if kind != "plain" else None,
                                     rating_table=t["rat"], dropout_ratio=p, seed=seed)


def _grads(t):
    got = {"g:past_embeddings": t["emb"].grad, "gp:_pos_emb.weight": t["pos"].grad}
    if t["rat"] is not None:
        got["gp:_rating_emb.weight"] = t["rat"].grad
    return got


def _untouched_rows_are_zero(z, got):
    n_out = z["f32:out"].shape[1]
    d_pos = got["gp:_pos_emb.weight"]
    assert d_pos.shape[0] == int(z["sd:_pos_emb.weight"].shape[0])
    assert d_pos.shape[0] == n_out or float(d_pos[n_out:].abs().max()) == 0.0, "position rows beyond N' are zero"
    if "gp:_rating_emb.weight" in got:
        used = set(np.unique(z["ratings"][z["past_ids"] != 0]).tolist())
        unused = [r for r in range(int(z["num_ratings"])) if r not in used]
        assert unused and {0, 5} <= used
        assert float(got["gp:_rating_emb.weight"][unused].abs().max()) == 0.0, "rows of ratings never seen are zero"


# ------------------------------------------------------------------------------------------------- 1, 4: fp32, dropout off
@pytest.mark.parametrize("case", R.PRE_CASES)
def test_op_fp32_is_bit_identical_and_table_gradients_pass_the_gate(case):
    z = R.load("pre_" + case)
    t = _inputs(z, torch.float32)
    out, valid = _run_op(z, t)
    (out * t["r"]).sum().backward()
    assert out.dtype == torch.float32 and valid.dtype == torch.float32 and valid.shape == out.shape[:2] + (1,)
    assert same_bits(out, z["f32:out"]), "out"
    assert same_bits(valid, z["f32:valid_mask"]), "valid_mask"
    got = _grads(t)
    assert same_bits(got["g:past_embeddings"], z["f32:g:past_embeddings"]), "d_past_embeddings"
    tables = [k for k in got if k.startswith("gp:")]
    R.gate("op " + case, "f32", got, z, tables, record=record_parity)
    _untouched_rows_are_zero(z, got)
    # determinism: a second backward on the same inputs
    first = {k: got[k].clone() for k in tables}
    for k in ("emb", "pos", "rat"):
        if t[k] is not None:
            t[k].grad = None
    out2, _ = _run_op(z, t)
    (out2 * t["r"]).sum().backward()
    again = _grads(t)
    assert all(torch.equal(first[k], again[k]) for k in tables), "two backward calls differ"


# ------------------------------------------------------------------------------------------------- 2: bf16
@pytest.mark.parametrize("case", R.PRE_CASES)
def test_op_bf16_passes_the_gate(case):
    z = R.load("pre_" + case)
    t = _inputs(z, torch.bfloat16)
    out, valid = _run_op(z, t)
    (out * t["r"]).sum().backward()
    assert out.dtype == torch.bfloat16 and valid.dtype == torch.float32
    assert same_bits(valid, z["f32:valid_mask"])
    got = dict(_grads(t), out=out)
    assert all(v.dtype == torch.bfloat16 for v in got.values())
    R.gate("op " + case, "bf16", got, z, list(got), record=record_parity)
    _untouched_rows_are_zero(z, got)


def test_op_promotes_16_bit_embeddings_into_an_fp32_module():
    z = R.load("pre_concat_d56_r8")
    t = _inputs(z, torch.float32)
    t["emb"] = t["emb"].detach().to(torch.bfloat16).requires_grad_(True)      # the fixture's values are bf16-representable
    out, _ = _run_op(z, t)
    (out * t["r"]).sum().backward()
    assert out.dtype == torch.float32 and same_bits(out, z["f32:out"])
    assert t["emb"].grad.dtype == torch.bfloat16 and t["pos"].grad.dtype == torch.float32
    assert torch.equal(t["emb"].grad, torch.from_numpy(z["f32:g:past_embeddings"]).to(DEV).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------- 3: dropout
def _item_part(kind, x, di):
    """the elements of a (B, N', Do) tensor that came from past_embeddings, as (B, N, Di)"""
    if kind == "concat":
        return x[:, :, :di]
    return x[:, 0::2] if kind == "interleave" else x


@pytest.mark.parametrize("seed", [3, 0x1234567890ABCDEF])
@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("case", ["plain_b3_n7_d50", "plain_b2_n3_d5", "plain_b2_n5_d256", "concat_d50_r14", "interleave_d64"])
def test_dropout_is_the_package_generator_forward_and_backward(case, p, seed):
    z = R.load("pre_" + case)
    kind, di = str(z["kind"]), int(z["item_dim"])
    t = _inputs(z, torch.float32)
    with torch.no_grad():
        out_p0, valid = _run_op(z, t)
    out, _ = _run_op(z, t, p=p, seed=seed)
    B, n_out, Do = out.shape
    keep, scale = dropout_keep_mask(seed, B * n_out, Do, p)
    keep = torch.from_numpy(keep.reshape(B, n_out, Do)).to(DEV)
    assert 0.5 * (1 - p) < float(keep.float().mean()) < min(1.0, 1.5 * (1 - p))
    scale32 = torch.tensor(scale, dtype=torch.float64).to(torch.float32).to(DEV)
    zero = torch.zeros((), device=DEV)
    want = torch.where(keep, out_p0 * scale32, zero)
    assert np.array_equal(bits(out), bits(want)), "forward: where(keep, fl(out_p0 * scale), 0)"
    g = t["r"]
    out.backward(g)
    s32 = torch.tensor(float(Do) ** 0.5, dtype=torch.float64).to(torch.float32).to(DEV)
    d_want = torch.where(keep, ((g * valid) * scale32) * s32, zero)
    d_emb = t["emb"].grad
    assert torch.equal(d_emb, _item_part(kind, d_want, di)), "backward: g * m * scale * s where kept"
    assert float(d_emb[~_item_part(kind, keep, di)].abs().max()) == 0.0, "backward: zero exactly where dropped"
    # the table gradients see the same mask: against the fp64 sums of h = g m keep scale (fp32 terms, any order)
    h = torch.where(keep, (g * valid) * scale32, zero).double()
    err = (t["pos"].grad.double()[:n_out] - h.sum(0)).abs()
    assert bool((err <= (B + 1) * 2.0**-24 * h.abs().sum(0)).all()), "d_pos under dropout"


def test_modules_ignore_dropout_in_eval_mode_and_training_is_reproducible():
    z = R.load("pre_concat_d50_r14")
    m = R.build_preprocessor(z, dropout_rate=0.5).to(DEV)
    args = (torch.from_numpy(z["past_lengths"]).to(DEV), torch.from_numpy(z["past_ids"]).to(DEV),
            torch.from_numpy(z["past_embeddings"]).to(DEV), {"ratings": torch.from_numpy(z["ratings"]).to(DEV)})
    assert m._emb_dropout.p == 0.5
    m.eval()
    assert same_bits(m(*args)[1], z["f32:out"]), "eval mode is the plain op"
    m.train()
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        runs.append(m(*args)[1])
    assert torch.equal(runs[0], runs[1]), "torch.manual_seed reproduces a training call"
    assert not torch.equal(runs[0], m(*args)[1]), "the next call draws another seed"
    live = torch.from_numpy(z["past_ids"]).to(DEV) != 0
    dropped = float((runs[0][live] == 0).float().mean())
    assert 0.4 < dropped < 0.6, f"p = 0.5 drops about half of the live elements, got {dropped:.3f}"


# ------------------------------------------------------------------------------------------------- the reference-free case
def _composition(kind, ids, emb, pos, ratings, rat):
    """the reference's chain in torch ops (dropout off), in the dtype of its arguments"""
    B, N = ids.shape
    if kind == "plain":
        x, n_out = emb, N
    else:
        x, n_out = torch.cat([emb, rat[ratings]], dim=2), N
    do = x.shape[-1]
    x = x * (do ** 0.5) + pos[:n_out].unsqueeze(0)
    return x * (ids != 0).unsqueeze(-1).to(x.dtype)


@pytest.mark.parametrize("kind", ["plain", "concat"])
def test_many_users_against_the_composition_on_the_device(kind):
    from generative_recommenders_amd.ops.research_preprocess import research_input_preprocess

    B, N, D, R_ = 300, 9, 64, 6
    di, dr = (D, 0) if kind == "plain" else (56, 8)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, 4, (B, N), generator=g).to(DEV)                  # a quarter of the ids are zero
    ratings = torch.randint(0, R_, (B, N), generator=g).to(DEV)
    emb = (0.05 * torch.randn(B, N, di, generator=g)).to(DEV)
    pos = (0.1 * torch.randn(N + 2, D, generator=g)).to(DEV)
    rat = (0.1 * torch.randn(R_, dr, generator=g)).to(DEV) if dr else None
    r = torch.randn(B, N, D, generator=g).to(DEV)
    leaves = [x.clone().requires_grad_(True) for x in (emb, pos) + ((rat,) if dr else ())]
    out, valid = research_input_preprocess(ids, leaves[0], leaves[1], layout=LAYOUT[kind], ratings=ratings if dr else None,
                                           rating_table=leaves[2] if dr else None)
    (out * r).sum().backward()
    want = _composition(kind, ids, emb, pos, ratings, rat)
    assert np.array_equal(bits(out), bits(want)), "fp32 forward is bit-exact against the composition"
    assert torch.equal(valid, (ids != 0).unsqueeze(-1).float())
    truth = [x.double().clone().requires_grad_(True) for x in (emb, pos) + ((rat,) if dr else ())]
    (_composition(kind, ids, truth[0], truth[1], ratings, truth[2] if dr else None) * r.double()).sum().backward()
    s, m = D ** 0.5, (ids != 0).unsqueeze(-1).double()
    h = (r.double() * m).abs()
    # an fp32 sum of n terms in any order: |err| <= n 2^-24 sum |terms| (+ one rounding for the factor s)
    bounds = [2.0**-24 * h[:, :, :di] * s,
              torch.cat([(B + 1) * 2.0**-24 * h.sum(0), torch.zeros(2, D, dtype=torch.float64, device=DEV)])]
    if dr:
        n_r = torch.stack([((ratings == k) & (ids != 0)).sum() for k in range(R_)]).double().view(-1, 1)
        abs_r = torch.stack([(h[:, :, di:] * (ratings == k).unsqueeze(-1)).sum((0, 1)) for k in range(R_)])
        bounds.append((n_r + 2) * 2.0**-24 * abs_r * s)
    for name, leaf, t64, bound in zip(("d_past_embeddings", "d_pos", "d_rating"), leaves, truth, bounds):
        err = (leaf.grad.double() - t64.grad).abs()
        print(f"many users {kind} {name}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
        record_parity(f"many_users_{kind}:{name}", leaf.grad.double().cpu().numpy(), t64.grad.cpu().numpy(), "float32")
        assert bool((err <= bound).all()), f"{name}: {float((err - bound).max()):.3e} over the bound"
    assert float(leaves[1].grad[N:].abs().max()) == 0.0
    first = [x.grad.clone() for x in leaves]
    for x in leaves:
        x.grad = None
    out2, _ = research_input_preprocess(ids, leaves[0], leaves[1], layout=LAYOUT[kind], ratings=ratings if dr else None,
                                        rating_table=leaves[2] if dr else None)
    (out2 * r).sum().backward()
    assert all(torch.equal(a, x.grad) for a, x in zip(first, leaves)), "two backward calls differ"


def test_empty_batch_and_gradients_only_where_asked():
    from generative_recommenders_amd.ops.research_preprocess import research_input_preprocess

    pos = torch.randn(4, 8, device=DEV, requires_grad=True)
    out, valid = research_input_preprocess(torch.zeros(0, 3, dtype=torch.int64, device=DEV), torch.zeros(0, 3, 8, device=DEV), pos)
    assert out.shape == (0, 3, 8) and valid.shape == (0, 3, 1)
    emb = torch.randn(2, 3, 8, device=DEV)                                   # no gradient asked for the embeddings
    out, _ = research_input_preprocess(torch.ones(2, 3, dtype=torch.int64, device=DEV), emb, pos)
    out.sum().backward()
    assert emb.grad is None and torch.equal(pos.grad[:3], torch.full((3, 8), 2.0, device=DEV)) and float(pos.grad[3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- 5: the modules
@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.PRE_CASES)
def test_preprocessor_modules_against_the_fixtures(case, tag):
    z = R.load("pre_" + case)
    dtype = R.TAGS[tag]
    m = R.build_preprocessor(z).to(DEV).to(dtype).eval()             # load_state_dict(strict=True) inside
    emb = torch.from_numpy(z["past_embeddings"]).to(DEV).to(dtype).requires_grad_(True)
    payloads = {"ratings": torch.from_numpy(z["ratings"]).to(DEV)} if str(z["kind"]) != "plain" else {}
    lengths, out, valid = m(torch.from_numpy(z["past_lengths"]).to(DEV), torch.from_numpy(z["past_ids"]).to(DEV), emb, payloads)
    (out * torch.from_numpy(z["r"]).to(DEV).to(dtype)).sum().backward()
    assert np.array_equal(lengths.cpu().numpy(), z["out_lengths"])
    assert out.dtype == dtype and same_bits(valid, z["f32:valid_mask"])
    got = {"out": out, "g:past_embeddings": emb.grad}
    got.update({"gp:" + k: p.grad for k, p in m.named_parameters()})
    if tag == "f32":
        assert same_bits(out, z["f32:out"]) and same_bits(emb.grad, z["f32:g:past_embeddings"])
        R.gate("module " + case, tag, got, z, [k for k in got if k.startswith("gp:")], record=record_parity)
    else:
        R.gate("module " + case, tag, got, z, list(got), record=record_parity)
    _untouched_rows_are_zero(z, got)


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.POST_CASES)
def test_postprocessor_modules_against_the_fixtures(case, tag):
    z = R.load("post_" + case)
    cls = R.CLASSES["L2NormEmbeddingPostprocessor" if str(z["kind"]) == "l2" else "LayerNormEmbeddingPostprocessor"]()
    m = cls(embedding_dim=int(z["embedding_dim"]), eps=float(z["eps"]))
    m.load_state_dict(R.state_dict_of(z), strict=True)
    dtype = R.TAGS[tag]
    m = m.to(DEV).to(dtype)
    x = torch.from_numpy(z["x"]).to(DEV).to(dtype).requires_grad_(True)
    out = m(x)
    (out * torch.from_numpy(z["r"]).to(DEV).to(dtype)).sum().backward()
    assert out.dtype == dtype and out.shape[-1] == int(z["embedding_dim"]) and x.grad.shape == x.shape
    if x.shape[-1] > out.shape[-1]:
        assert float(x.grad[..., out.shape[-1]:].abs().max()) == 0.0, "the columns cut off get no gradient"
    R.gate("post " + case, tag, {"out": out, "g:x": x.grad}, z, ["out", "g:x"], record=record_parity)


# ------------------------------------------------------------------------------------------------- 6: end to end
def _build_model(z):
    """HSTU / SASRec from THIS package's modules only, the reference model's state_dict loaded"""
    from generative_recommenders_amd.research.modeling.sequential.hstu import HSTU
    from generative_recommenders_amd.research.modeling.sequential.sasrec import SASRec

    D, H, blocks, n, linear_dim, attention_dim, hidden = (int(x) for x in z["config"])
    c = {k: f() for k, f in R.CLASSES.items()}
    parts = dict(embedding_module=c["LocalEmbeddingModule"](int(z["num_items"]), D), similarity_module=c["DotProductSimilarity"](),
                 input_features_preproc_module=c["LearnablePositionalEmbeddingInputFeaturesPreprocessor"](n, D, 0.0),
                 output_postproc_module=c["L2NormEmbeddingPostprocessor"](D, 1e-6))
    if str(z["kind"]) == "hstu":
        model = HSTU(max_sequence_len=n - 2, max_output_len=2, embedding_dim=D, num_blocks=blocks, num_heads=H,
                     linear_dim=linear_dim, attention_dim=attention_dim, normalization="rel_bias", linear_config="uvqk",
                     linear_activation="silu", linear_dropout_rate=0.0, attn_dropout_rate=0.0, verbose=False, **parts)
    else:
        model = SASRec(max_sequence_len=n - 2, max_output_len=2, embedding_dim=D, num_blocks=blocks, num_heads=H,
                       ffn_hidden_dim=hidden, ffn_activation_fn=str(z["activation"]), ffn_dropout_rate=0.0, **parts)
    own = model.state_dict()
    assert list(own) == [str(k) for k in z["sd_keys"]], "state_dict keys = the reference model's"
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(z["sd:" + k])).to(own[k].dtype) for k in own}, strict=True)
    return model


BLOCK_WEIGHT = {"hstu": "_hstu._attention_layers.0._uvqk", "sasrec": "attention_layers.0.in_proj_weight"}


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["hstu", "sasrec"])
def test_models_built_from_the_package_modules_only(kind, tag):
    from generative_recommenders_amd.research.modeling.sequential.losses.sampled_softmax import SampledSoftmaxLoss

    z = R.load("model_" + kind)
    dtype = R.TAGS[tag]
    model = _build_model(z).to(DEV).to(dtype).eval()
    SampledSoftmaxLoss(num_to_sample=8, softmax_temperature=0.05, model=model)          # accepts the similarity module
    lengths, ids = torch.from_numpy(z["past_lengths"]).to(DEV), torch.from_numpy(z["past_ids"]).to(DEV)
    payloads = {"timestamps": torch.from_numpy(z["timestamps"]).to(DEV)}
    emb = model.get_item_embeddings(ids)
    y = model(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads=payloads)
    cur = model.encode(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads=payloads)
    sim, _ = model.similarity_fn(cur, torch.from_numpy(z["item_ids"]).to(DEV))
    r = {k: torch.from_numpy(z["r:" + k]).to(DEV).to(dtype) for k in ("forward", "encode", "similarity")}
    ((y * r["forward"]).sum() + (cur * r["encode"]).sum() + (sim * r["similarity"]).sum()).backward()
    params = dict(model.named_parameters())
    got = {"forward": y, "encode": cur, "similarity": sim}
    for name in ("_embedding_module._item_emb.weight", "_input_features_preproc._pos_emb.weight", BLOCK_WEIGHT[kind]):
        got["gp:" + name] = params[name].grad
    assert all(v is not None and v.dtype == dtype for v in got.values())
    R.gate("model " + kind, tag, got, z, list(got), record=record_parity)
