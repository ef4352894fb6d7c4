#!/usr/bin/env python3
"""Mint the fixtures of the research-path model parts from the REFERENCE's modules (CPU).

Run in the build container only (needs /root/reference):

    python tests/golden/research_modules/make_research_modules_golden.py [--out DIR]

``generative_recommenders.research.modeling.sequential.{embedding_modules,input_features_preprocessors,
output_postprocessors,hstu,sasrec}`` and ``research.rails.similarities.dot_product_similarity_fn`` are imported unmodified
(``_fbgemm_shim`` stands in for the absent fbgemm ops of the two models).  Every float case runs on the SAME values in fp32, in
bf16 (``module.to(torch.bfloat16)``) and in fp64, the truth: inputs and parameters are rounded to bf16-representable numbers
first, so only the arithmetic differs.  The loss is ``(out * r).sum()``.

* ``pre_<case>.npz``: the three input-feature preprocessors (eval mode: the reference's dropout stream cannot be restated;
  the fused op's dropout is tested against this package's generator) -- out, valid_mask, and the gradients of the
  embeddings and of both tables; for the combined preprocessor also ``get_preprocessed_ids`` / ``get_preprocessed_masks``.
* ``post_<case>.npz``: the L2-norm and LayerNorm postprocessors, with and without a cutting ``[..., :embedding_dim]``.
* ``embeddings.npz``: ``LocalEmbeddingModule`` / ``CategoricalEmbeddingModule`` lookups (id 0, the category remap).
* ``similarity.npz``: the three shape branches of ``DotProductSimilarity``.
* ``model_<name>.npz``: ``HSTU`` and ``SASRec`` built from the reference's own LocalEmbeddingModule, plain preprocessor,
  L2NormEmbeddingPostprocessor and DotProductSimilarity: forward, encode, similarity_fn over 20 item ids, every gradient.
* ``reference_names.npz``: constructor parameter names, state_dict keys and debug_str() of every class.

Only arrays, integers and lists of names are stored.  16-bit values are stored as bf16 bit patterns."""

import argparse
import inspect
import io
import os
import sys
from contextlib import redirect_stdout

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import _fbgemm_shim  # noqa: F401  (registers torch.ops.fbgemm.*)

from generative_recommenders.research.modeling.sequential.embedding_modules import (  # noqa: E402
    CategoricalEmbeddingModule,
    LocalEmbeddingModule,
)
from generative_recommenders.research.modeling.sequential.hstu import HSTU  # noqa: E402
from generative_recommenders.research.modeling.sequential.input_features_preprocessors import (  # noqa: E402
    CombinedItemAndRatingInputFeaturesPreprocessor,
    LearnablePositionalEmbeddingInputFeaturesPreprocessor,
    LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor,
)
from generative_recommenders.research.modeling.sequential.output_postprocessors import (  # noqa: E402
    L2NormEmbeddingPostprocessor,
    LayerNormEmbeddingPostprocessor,
)
from generative_recommenders.research.modeling.sequential.sasrec import SASRec  # noqa: E402
from generative_recommenders.research.rails.similarities.dot_product_similarity_fn import DotProductSimilarity  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
NUM_RATINGS = 6

# name -> (kind, B, N, Di, Dr, spare position rows)
PRE_CASES = {
    "plain_b3_n7_d50": ("plain", 3, 7, 50, 0, 3),
    "plain_b2_n3_d5": ("plain", 2, 3, 5, 0, 0),
    "plain_b2_n5_d256": ("plain", 2, 5, 256, 0, 2),
    "concat_d50_r14": ("concat", 3, 7, 50, 14, 1),
    "concat_d56_r8": ("concat", 3, 7, 56, 8, 0),
    "interleave_d64": ("interleave", 3, 4, 64, 64, 1),
    "interleave_d50": ("interleave", 3, 4, 50, 50, 0),
}
# name -> (kind, B, N, last dimension of the input, embedding_dim)
POST_CASES = {
    "l2_cut_40_32": ("l2", 3, 5, 40, 32),
    "l2_full_50": ("l2", 3, 5, 50, 50),
    "ln_cut_40_32": ("ln", 3, 5, 40, 32),
    "ln_full_64": ("ln", 3, 5, 64, 64),
}


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def store(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def quiet(fn, *args, **kwargs):
    """the reference's embedding modules print while they initialise"""
    with redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def rounded_state_dict(module, g, jitter=0.0):
    sd = {}
    for k, v in module.state_dict().items():
        if v.is_floating_point():
            sd[k] = bf16_round(v + jitter * torch.randn(v.shape, generator=g))
        else:
            sd[k] = v.clone()
    return sd


def put_state_dict(z, sd):
    z["sd_keys"] = np.array(list(sd))
    for k, v in sd.items():
        z["sd:" + k] = v.numpy().astype(np.uint8) if v.dtype == torch.bool else v.numpy()


def check_differs(name, res, keys):
    for tag in ("f32", "bf16"):
        for k in keys:
            truth = res["f64"][k].detach().double()
            err = float((res[tag][k].detach().double() - truth).norm() / truth.norm())
            assert err > 0.0, f"{name}: {tag}:{k} equals the fp64 truth exactly: a relative gate on it would be vacuous"


def ids_with_zeros(B, N, g, high):
    """user 0 full, user 1 all zero, user 2 with a zero id in the middle; further users as user 0 (B == 2: full, middle zero)"""
    ids = torch.randint(1, high, (B, N), generator=g)
    if B >= 3:
        ids[1] = 0
        ids[2, N // 2] = 0
        ids[2, N - 1] = 0
    else:
        ids[1, N // 2] = 0
    return ids


# ------------------------------------------------------------------------------------------------------ preprocessors
def build_pre(kind, N, Di, Dr, spare):
    if kind == "plain":
        return LearnablePositionalEmbeddingInputFeaturesPreprocessor(N + spare, Di, 0.2)
    if kind == "concat":
        return LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor(N + spare, Di, 0.2, Dr, NUM_RATINGS)
    return CombinedItemAndRatingInputFeaturesPreprocessor(N + spare, Di, 0.2, NUM_RATINGS)


def pre_case(name, seed):
    kind, B, N, Di, Dr, spare = PRE_CASES[name]
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    ids = ids_with_zeros(B, N, g, 100)
    lengths = (ids != 0).sum(1)
    emb = bf16_round(0.05 * torch.randn(B, N, Di, generator=g))
    ratings = torch.randint(0, NUM_RATINGS - 1, (B, N), generator=g)      # 0 .. 4, then:
    ratings[ratings == 3] = 5                                                 # 0 and 5 used, 3 never
    ratings[0, 0], ratings[0, 1] = 0, 5
    proto = build_pre(kind, N, Di, Dr, spare)
    sd = rounded_state_dict(proto, g)
    n_out = 2 * N if kind == "interleave" else N
    r = torch.randn(B, n_out, Di + Dr if kind == "concat" else Di, generator=g)
    z = dict(kind=np.array(kind), past_ids=ids.numpy(), past_lengths=lengths.numpy(), past_embeddings=emb.numpy(),
             ratings=ratings.numpy(), r=r.numpy(), num_ratings=np.int64(NUM_RATINGS), max_sequence_len=np.int64(N + spare),
             item_dim=np.int64(Di), rating_dim=np.int64(Dr), dropout_rate=np.float64(0.2))
    put_state_dict(z, sd)
    res = {}
    for tag, dt in DTYPES.items():
        m = build_pre(kind, N, Di, Dr, spare)
        m.load_state_dict(sd, strict=True)
        m = m.to(dt).eval()
        e = emb.clone().to(dt).requires_grad_(True)
        payloads = {"ratings": ratings} if kind != "plain" else {}
        out_lengths, out, valid = m(lengths, ids, e, payloads)
        (out * r.to(dt)).sum().backward()
        d = {"out": out, "valid_mask": valid, "g:past_embeddings": e.grad}
        for k, p in m.named_parameters():
            d["gp:" + k] = p.grad
        res[tag] = d
        if tag == "f32":
            z["out_lengths"] = out_lengths.numpy()
            if kind == "interleave":
                z["preprocessed_ids"] = m.get_preprocessed_ids(lengths, ids, e, payloads).numpy()
                z["preprocessed_masks"] = m.get_preprocessed_masks(lengths, ids, e, payloads).numpy()
    check_differs(name, res, [k for k in res["f64"] if k.startswith("gp:")])
    for tag, d in res.items():
        for k, v in d.items():
            z[f"{tag}:{k}"] = store(v)
    return z


# ------------------------------------------------------------------------------------------------------ postprocessors
def post_case(name, seed):
    kind, B, N, D_in, D = POST_CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = bf16_round(torch.randn(B, N, D_in, generator=g))
    x[1, 2] = 0.0                                  # a zero row: the eps clamp of the L2 norm
    r = torch.randn(B, N, D, generator=g)
    cls = L2NormEmbeddingPostprocessor if kind == "l2" else LayerNormEmbeddingPostprocessor
    z = dict(kind=np.array(kind), x=x.numpy(), r=r.numpy(), embedding_dim=np.int64(D), eps=np.float64(1e-6))
    put_state_dict(z, cls(embedding_dim=D, eps=1e-6).state_dict())
    res = {}
    for tag, dt in DTYPES.items():
        m = cls(embedding_dim=D, eps=1e-6).to(dt)
        xi = x.clone().to(dt).requires_grad_(True)
        out = m(xi)
        (out * r.to(dt)).sum().backward()
        res[tag] = {"out": out, "g:x": xi.grad}
    check_differs(name, res, ["out", "g:x"])
    for tag, d in res.items():
        for k, v in d.items():
            z[f"{tag}:{k}"] = store(v)
    return z


# ------------------------------------------------------------------------------------------------------ plain-torch parts
def embeddings_case(seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    num_items, D = 12, 8
    ids = torch.tensor([[0, 1, 12, 5], [7, 0, 0, 3]])
    local = quiet(LocalEmbeddingModule, num_items, D)
    to_cat = torch.randint(0, 4, (num_items,), generator=g)
    cat = quiet(CategoricalEmbeddingModule, num_items, D, to_cat)
    z = dict(num_items=np.int64(num_items), item_embedding_dim=np.int64(D), item_ids=ids.numpy(),
             item_id_to_category_id=to_cat.numpy())
    for name, m in (("local", local), ("categorical", cat)):
        z[name + ":sd_keys"] = np.array(list(m.state_dict()))
        for k, v in m.state_dict().items():
            z[f"{name}:sd:{k}"] = v.numpy()
        z[name + ":out"] = m.get_item_embeddings(ids).detach().numpy()
    return z


def similarity_case(seed):
    g = torch.Generator().manual_seed(seed)
    B, X, D, rep = 4, 7, 16, 3
    m = DotProductSimilarity()
    q = torch.randn(B, D, generator=g)
    q_rep = torch.randn(B * rep, D, generator=g)
    shared = torch.randn(1, X, D, generator=g)
    per_user = torch.randn(B, X, D, generator=g)
    z = dict(q=q.numpy(), q_rep=q_rep.numpy(), items_shared=shared.numpy(), items_per_user=per_user.numpy())
    z["out:shared"] = m(q, shared)[0].numpy()               # (B, D) x (1, X, D)
    z["out:repeated"] = m(q_rep, per_user)[0].numpy()       # (B r, D) x (B, X, D)
    z["out:per_user"] = m(q, per_user)[0].numpy()           # (B, D) x (B, X, D)
    return z


# ------------------------------------------------------------------------------------------------------ the two models
NUM_ITEMS = 60


def build_model(kind, cfg):
    D, n = cfg["D"], cfg["N"]
    parts = dict(embedding_module=quiet(LocalEmbeddingModule, NUM_ITEMS, D), similarity_module=DotProductSimilarity(),
                 input_features_preproc_module=LearnablePositionalEmbeddingInputFeaturesPreprocessor(n, D, 0.0),
                 output_postproc_module=L2NormEmbeddingPostprocessor(D, 1e-6))
    if kind == "hstu":
        return HSTU(max_sequence_len=n - 2, max_output_len=2, embedding_dim=D, num_blocks=cfg["blocks"], num_heads=cfg["H"],
                    linear_dim=cfg["linear_dim"], attention_dim=cfg["attention_dim"], normalization="rel_bias",
                    linear_config="uvqk", linear_activation="silu", linear_dropout_rate=0.0, attn_dropout_rate=0.0,
                    verbose=False, **parts)
    return SASRec(max_sequence_len=n - 2, max_output_len=2, embedding_dim=D, num_blocks=cfg["blocks"], num_heads=cfg["H"],
                  ffn_hidden_dim=cfg["hidden"], ffn_activation_fn=cfg["act"], ffn_dropout_rate=0.0, **parts)


MODEL_CASES = {
    "hstu": dict(D=32, H=2, blocks=2, N=14, linear_dim=16, attention_dim=16, lengths=[14, 5, 9, 1]),
    "sasrec": dict(D=48, H=3, blocks=2, N=40, hidden=40, act="gelu", lengths=[40, 1, 0, 17, 33]),      # model_a of golden/sasrec
}


def model_case(kind, seed):
    cfg = MODEL_CASES[kind]
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    D, n, lengths = cfg["D"], cfg["N"], torch.tensor(cfg["lengths"])
    B = len(lengths)
    proto = build_model(kind, cfg)
    sd = rounded_state_dict(proto, g, jitter=0.02)
    ids = torch.randint(1, NUM_ITEMS + 1, (B, n), generator=g) * (torch.arange(n).unsqueeze(0) < lengths.unsqueeze(1))
    ts = torch.sort(torch.randint(0, 10**7, (B, n), generator=g), dim=1).values
    item_ids = torch.randint(1, NUM_ITEMS + 1, (1, 20), generator=g)
    r = {"forward": torch.randn(B, n, D, generator=g), "encode": torch.randn(B, D, generator=g),
         "similarity": torch.randn(B, 20, generator=g)}
    z = dict(kind=np.array(kind), past_lengths=lengths.numpy(), past_ids=ids.numpy(), timestamps=ts.numpy(),
             item_ids=item_ids.numpy(), num_items=np.int64(NUM_ITEMS), activation=np.array(cfg.get("act", "")),
             config=np.array([D, cfg["H"], cfg["blocks"], n, cfg.get("linear_dim", 0), cfg.get("attention_dim", 0),
                              cfg.get("hidden", 0)], dtype=np.int64))
    for k, v in r.items():
        z["r:" + k] = v.numpy()
    put_state_dict(z, sd)
    res = {}
    for tag, dt in DTYPES.items():
        m = build_model(kind, cfg)
        m.load_state_dict(sd, strict=True)
        m = m.to(dt).eval()
        payloads = {"timestamps": ts}
        emb = m.get_item_embeddings(ids)
        y = m(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads=payloads)
        cur = m.encode(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads=payloads)
        sim, _ = m.similarity_fn(cur, item_ids)
        ((y * r["forward"].to(dt)).sum() + (cur * r["encode"].to(dt)).sum() + (sim * r["similarity"].to(dt)).sum()).backward()
        d = {"forward": y, "encode": cur, "similarity": sim}
        for k, p in m.named_parameters():
            if p.grad is not None:
                d["gp:" + k] = p.grad
        res[tag] = d
    for tag, d in res.items():
        for k, v in d.items():
            z[f"{tag}:{k}"] = store(v)
    return z


# ------------------------------------------------------------------------------------------------------ names
def reference_names():
    to_cat = torch.zeros(4, dtype=torch.int64)
    instances = {
        "LocalEmbeddingModule": quiet(LocalEmbeddingModule, 4, 8),
        "CategoricalEmbeddingModule": quiet(CategoricalEmbeddingModule, 4, 8, to_cat),
        "LearnablePositionalEmbeddingInputFeaturesPreprocessor": LearnablePositionalEmbeddingInputFeaturesPreprocessor(5, 8, 0.2),
        "LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor":
            LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor(5, 8, 0.5, 4, 6),
        "CombinedItemAndRatingInputFeaturesPreprocessor": CombinedItemAndRatingInputFeaturesPreprocessor(5, 8, 0.25, 6),
        "L2NormEmbeddingPostprocessor": L2NormEmbeddingPostprocessor(8, 1e-6),
        "LayerNormEmbeddingPostprocessor": LayerNormEmbeddingPostprocessor(8, 1e-6),
        "DotProductSimilarity": DotProductSimilarity(),
    }
    z = {"classes": np.array(list(instances))}
    for name, m in instances.items():
        z[name + ":init"] = np.array([p for p in inspect.signature(type(m).__init__).parameters if p != "self"] or [""])
        z[name + ":state_dict"] = np.array(list(m.state_dict()) or [""])
        z[name + ":debug_str"] = np.array(m.debug_str())
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(1)   # one summation order whatever the host

    def save(name, z):
        np.savez_compressed(os.path.join(args.out, name + ".npz"), **z)

    for n, name in enumerate(PRE_CASES):
        save("pre_" + name, pre_case(name, 1100 + n))
    for n, name in enumerate(POST_CASES):
        save("post_" + name, post_case(name, 1200 + n))
    save("embeddings", embeddings_case(1300))
    save("similarity", similarity_case(1301))
    for n, kind in enumerate(MODEL_CASES):
        save("model_" + kind, model_case(kind, 1400 + n))
    save("reference_names", reference_names())


if __name__ == "__main__":
    main()
