"""Loader of the fixtures under tests/golden/research_modules/ (minted from the reference's modules by
make_research_modules_golden.py), builders of this package's modules from them, and the parity gate shared by the CPU and
GPU tests of the research-path model parts."""

import os

import numpy as np
import torch

from conftest import GOLDEN
from multitask_ref import gate_multiplier, rel_fro

FIXTURES = os.path.join(GOLDEN, "research_modules")
TAGS = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_NAME = {"f32": "float32", "bf16": "bfloat16"}
PRE_CASES = ("plain_b3_n7_d50", "plain_b2_n3_d5", "plain_b2_n5_d256", "concat_d50_r14", "concat_d56_r8", "interleave_d64",
             "interleave_d50")
POST_CASES = ("l2_cut_40_32", "l2_full_50", "ln_cut_40_32", "ln_full_64")


def _classes():
    from generative_recommenders_amd.research.modeling.sequential import embedding_modules as E
    from generative_recommenders_amd.research.modeling.sequential import input_features_preprocessors as P
    from generative_recommenders_amd.research.modeling.sequential import output_postprocessors as O
    from generative_recommenders_amd.research.rails.similarities.dot_product_similarity_fn import DotProductSimilarity

    return {
        "LocalEmbeddingModule": E.LocalEmbeddingModule,
        "CategoricalEmbeddingModule": E.CategoricalEmbeddingModule,
        "LearnablePositionalEmbeddingInputFeaturesPreprocessor": P.LearnablePositionalEmbeddingInputFeaturesPreprocessor,
        "LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor": P.LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor,
        "CombinedItemAndRatingInputFeaturesPreprocessor": P.CombinedItemAndRatingInputFeaturesPreprocessor,
        "L2NormEmbeddingPostprocessor": O.L2NormEmbeddingPostprocessor,
        "LayerNormEmbeddingPostprocessor": O.LayerNormEmbeddingPostprocessor,
        "DotProductSimilarity": DotProductSimilarity,
    }


class _Lazy(dict):
    """name -> a function returning the class: the package is imported when a test asks, not at collection"""

    def __init__(self):
        super().__init__((name, (lambda name=name: _classes()[name])) for name in (
            "LocalEmbeddingModule", "CategoricalEmbeddingModule", "LearnablePositionalEmbeddingInputFeaturesPreprocessor",
            "LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor", "CombinedItemAndRatingInputFeaturesPreprocessor",
            "L2NormEmbeddingPostprocessor", "LayerNormEmbeddingPostprocessor", "DotProductSimilarity"))


CLASSES = _Lazy()


def instance_for_names(cls_name):
    """the instances whose names the fixture maker recorded (same constructor arguments)"""
    args = {
        "LocalEmbeddingModule": (4, 8),
        "CategoricalEmbeddingModule": (4, 8, torch.zeros(4, dtype=torch.int64)),
        "LearnablePositionalEmbeddingInputFeaturesPreprocessor": (5, 8, 0.2),
        "LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor": (5, 8, 0.5, 4, 6),
        "CombinedItemAndRatingInputFeaturesPreprocessor": (5, 8, 0.25, 6),
        "L2NormEmbeddingPostprocessor": (8, 1e-6),
        "LayerNormEmbeddingPostprocessor": (8, 1e-6),
        "DotProductSimilarity": (),
    }[cls_name]
    return CLASSES[cls_name]()(*args)


def widen(a):
    """bf16 bit patterns (uint16) -> the float32 values they stand for"""
    return (a.astype(np.uint32) << 16).view(np.float32) if a.dtype == np.uint16 else a


def load(name):
    z = np.load(os.path.join(FIXTURES, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def load_names():
    z = np.load(os.path.join(FIXTURES, "reference_names.npz"), allow_pickle=False)
    return {k: [str(s) for s in np.atleast_1d(z[k]) if str(s) != "" or k.endswith(":debug_str")] for k in z.files}


def state_dict_of(z, prefix="sd"):
    keys = z["sd_keys"] if prefix == "sd" else z[prefix + "_keys"]
    return {str(k): torch.from_numpy(np.asarray(z[f"{prefix}:{k}"])) for k in keys}


def build_preprocessor(z, dropout_rate=None):
    """this package's preprocessor of a ``pre_*`` fixture with the reference's state_dict loaded (strict)"""
    c = _classes()
    kind = str(z["kind"])
    n, di, dr = int(z["max_sequence_len"]), int(z["item_dim"]), int(z["rating_dim"])
    p = float(z["dropout_rate"]) if dropout_rate is None else dropout_rate
    if kind == "plain":
        m = c["LearnablePositionalEmbeddingInputFeaturesPreprocessor"](n, di, p)
    elif kind == "concat":
        m = c["LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor"](n, di, p, dr, int(z["num_ratings"]))
    else:
        m = c["CombinedItemAndRatingInputFeaturesPreprocessor"](n, di, p, int(z["num_ratings"]))
    m.load_state_dict(state_dict_of(z), strict=True)
    return m


def gate(name, tag, got, z, keys, record=None):
    """e_hip <= m * e_ref per tensor, both relative Frobenius errors against the fp64 truth (multitask_ref.gate_multiplier)"""
    bad = []
    for k in keys:
        truth = z["f64:" + k]
        hip = got[k].detach().double().cpu().numpy().reshape(truth.shape)
        e_hip = rel_fro(hip, truth)
        e_ref = rel_fro(widen(z[f"{tag}:{k}"]), truth)
        mult = gate_multiplier(DTYPE_NAME[tag], truth.size)
        ratio = e_hip / e_ref if e_ref > 0 else (0.0 if e_hip == 0 else float("inf"))
        print(f"{name} {tag} {k}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {ratio:.3f} (m = {mult})")
        if record is not None:
            record(f"{name}:{k}", hip, truth, DTYPE_NAME[tag], e_ref=e_ref, ratio=ratio)
        if not e_hip <= mult * e_ref:
            bad.append((k, e_hip, e_ref, mult))
    assert not bad, f"{name} {tag}: (tensor, e_hip, e_ref, m) with e_hip > m * e_ref: {bad}"
