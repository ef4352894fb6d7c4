#!/usr/bin/env python3
"""Mint the fixtures of the input preprocessors from the REFERENCE's modules (PyTorch path, CPU).

Run in the build container only (needs /root/reference):

    python tests/golden/preprocessor/make_preprocessor_golden.py [--out DIR]

``generative_recommenders.modules.{action_encoder,content_encoder,preprocessors,contextual_interleave_preprocessor}`` are
imported unmodified: ``_fbgemm_shim`` stands in for the absent fbgemm ops and a ``libfb.py.pyre.none_throws`` stand-in is
planted as in ``tests/golden/jagged_bmm/make_jagged_bmm_golden.py``.  Every case runs on the SAME values in fp32, in bf16
(``module.to(torch.bfloat16)``: the CPU ignores ``autocast("cuda")``) and in fp64, the truth -- inputs and parameters are
rounded to bf16-representable numbers first, so only the arithmetic differs.  In the fp64 run the reference's LayerNorm /
SwishLayerNorm, whose PyTorch path casts to fp32 whatever comes in, compute the same formula in the dtype of their input
(``make_multitask_golden.py`` does the same); everything else is the reference's code.

* ``op_<case>.npz``: ``ActionEncoder`` -- the output and the gradients of ``(out * r).sum()`` for both tables.
* ``module_<case>.npz``: ``ContextualInterleavePreprocessor`` in its three combine modes (the inference one forward only, in
  fp32 next to the truth) and ``ContextualPreprocessor`` -- every returned value, the MLP outputs handed to ``combine_embeddings`` and the gradients of ``(out * r).sum()`` (not
  ``out.sum()``: the MLPs end in a LayerNorm, whose plain sum has next to no gradient) for the inputs and every parameter.

Every stored float tensor of the fp32 and bf16 runs that a relative gate is applied to must differ from the truth (asserted
here).  16-bit values are stored as bf16 bit patterns."""

import argparse
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import _fbgemm_shim  # noqa: F401  (registers torch.ops.fbgemm.*)

_pyre = types.ModuleType("libfb.py.pyre")


def _none_throws(x):
    assert x is not None
    return x


_pyre.none_throws = _none_throws
for _name in ("libfb", "libfb.py"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["libfb.py.pyre"] = _pyre

from generative_recommenders.common import HammerKernel, set_dev_mode  # noqa: E402
from generative_recommenders.modules.action_encoder import ActionEncoder  # noqa: E402
from generative_recommenders.modules.content_encoder import ContentEncoder  # noqa: E402
from generative_recommenders.modules.contextual_interleave_preprocessor import ContextualInterleavePreprocessor  # noqa: E402
from generative_recommenders.modules.contextualize_mlps import (  # noqa: E402
    ParameterizedContextualizedMLP,
    SimpleContextualizedMLP,
)
from generative_recommenders.modules.preprocessors import ContextualPreprocessor  # noqa: E402
from generative_recommenders.ops.layer_norm import LayerNorm, SwishLayerNorm  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
LENGTHS, TARGETS = [7, 1, 4, 3, 9], [2, 1, 0, 3, 1]     # a user without targets, one without UIH rows, one of targets only

# name -> (action weights, [(threshold, weight)], Da, lengths, targets)
OP_CASES = {
    "reftest": ([1, 2, 4, 8, 16], [(30, 32), (60, 64), (100, 128)], 32, [6, 3], [2, 1]),
    "odd_3x5": ([2], [(10, 1), (50, 4)], 5, LENGTHS, TARGETS),
    "wide_8x32": ([1, 2, 4, 8, 16, 32, 64, 128], [], 32, [12, 5, 8], [3, 0, 2]),
}
D_IN, D_OUT, HIDDEN = 16, 24, 8
CONTEXTUAL, MIN_UIH = {"c0": 1, "c1": 2}, {"c1": 4}
ADDITIONAL, ENRICH = {"a0": 8}, {"t0": 8}
ACTION_WEIGHTS, ACTION_THRESHOLDS, ACTION_DIM = [1, 2, 4], [(30, 8)], 8
# name -> (class, interleaving, parameterized MLPs, is_inference, dtypes)
MODULE_CASES = {
    "train_sum_simple": ("interleave", False, False, False, ("f32", "bf16", "f64")),
    "train_interleave_pmlp": ("interleave", True, True, False, ("f32", "bf16", "f64")),
    "infer_interleave": ("interleave", True, False, True, ("f32", "f64")),
    "contextual": ("contextual", False, False, False, ("f32", "f64")),
}


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def store(t, as_bf16=False):
    t = t.detach().contiguous()
    if as_bf16 or t.dtype == torch.bfloat16:
        return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def offsets_of(lengths):
    o = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    o[1:] = torch.tensor(lengths).cumsum(0)
    return o


def truth_norms(module):
    """fp64 run: LayerNorm / SwishLayerNorm in the dtype of their input (the reference's PyTorch path drops to fp32)"""
    for m in module.modules():
        if isinstance(m, SwishLayerNorm):
            m.forward = lambda x, m=m: x * torch.sigmoid(
                torch.nn.functional.layer_norm(x, m._normalized_shape, m.weight, m.bias, m._eps))
        elif isinstance(m, LayerNorm):
            m.forward = lambda x, m=m: torch.nn.functional.layer_norm(x, m._normalized_shape, m.weight, m.bias, m._eps)


def rounded_state_dict(module, g):
    """every float parameter moved off its default (zero biases, (1, 0) norms) and rounded to bf16-representable values"""
    sd = {}
    for k, v in module.state_dict().items():
        sd[k] = bf16_round(v + 0.1 * torch.randn(v.shape, generator=g)) if v.is_floating_point() else v.clone()
    return sd


def check_differs(name, res, keys):
    for tag in ("f32", "bf16"):
        if tag not in res:
            continue
        for k in keys:
            truth = res["f64"][k].detach().double()
            err = float((res[tag][k].detach().double() - truth).norm() / truth.norm())
            assert err > 0.0, f"{name}: {tag}:{k} equals the fp64 truth exactly: a relative gate on it would be vacuous"


# ------------------------------------------------------------------------------------------------------ ActionEncoder
def op_case(name, seed):
    weights, thresholds, da, lengths, targets = OP_CASES[name]
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    uih = [l - t for l, t in zip(lengths, targets)]
    n_uih, total = sum(uih), sum(lengths)
    combined = weights + [w for _, w in thresholds]
    if name == "reftest":       # modules/tests/action_encoder_test.py:43-58
        enabled = [[0], [0, 1], [1, 3, 4], [1, 2, 3, 4], [1, 2], [2]]
        watch = [40, 20, 110, 31, 26, 55]
        for i, wt in enumerate(watch):
            for j, w in enumerate(thresholds):
                if wt > w[0]:
                    enabled[i].append(j + len(weights))
        actions = torch.tensor([sum(combined[t] for t in x) for x in enabled])
        watchtimes = torch.tensor(watch)
    else:
        actions = torch.randint(0, 2 * max(combined), (n_uih,), generator=g)
        watchtimes = torch.randint(0, 100, (n_uih,), generator=g)
        if thresholds:
            watchtimes[0], watchtimes[1] = thresholds[0][0], thresholds[1][0] - 1     # ">=": at and just below a threshold
    proto = ActionEncoder(action_embedding_dim=da, action_feature_name="actions", action_weights=weights,
                          watchtime_feature_name="watchtimes", watchtime_to_action_thresholds_and_weights=thresholds)
    sd = rounded_state_dict(proto, g)
    r = torch.randn(total, len(combined) * da, generator=g)
    uo, to = offsets_of(uih), offsets_of(targets)
    z = dict(action_weights=np.array(weights, dtype=np.int64), thresholds=np.array(thresholds, dtype=np.int64).reshape(-1, 2),
             embedding_dim=np.int64(da), uih_offsets=uo.numpy(), target_offsets=to.numpy(), actions=actions.numpy(),
             watchtimes=watchtimes.numpy(), r=store(r), max_uih_len=np.int64(max(uih)), max_targets=np.int64(max(targets)),
             sd_keys=np.array(list(sd)))
    for k, v in sd.items():
        z["sd:" + k] = store(v, v.is_floating_point())
    res = {}
    for tag, dt in DTYPES.items():
        m = ActionEncoder(action_embedding_dim=da, action_feature_name="actions", action_weights=weights,
                          watchtime_feature_name="watchtimes", watchtime_to_action_thresholds_and_weights=thresholds)
        m.load_state_dict(sd, strict=True)
        m.set_hammer_kernel(HammerKernel.PYTORCH)
        m = m.to(dt)
        out = m(max_uih_len=max(uih), max_targets=max(targets), uih_offsets=uo, target_offsets=to,
                seq_embeddings=torch.zeros(total, 4, dtype=dt), seq_payloads={"actions": actions, "watchtimes": watchtimes})
        (out * r.to(dt)).sum().backward()
        res[tag] = dict(out=out, g_table=m._action_embedding_table.grad, g_target=m._target_action_embedding_table.grad)
    check_differs(name, res, ("g_table", "g_target"))
    for tag, d in res.items():
        assert torch.equal(d["out"].double(), res["f64"]["out"]), f"{name}: the {tag} output is not a copy of the parameters"
        for k, v in d.items():
            z[f"{tag}:{k}"] = store(v)
    return z


# ------------------------------------------------------------------------------------------------------ the preprocessors
def build_module(kind, interleaving, pmlp, is_inference):
    if kind == "contextual":
        return ContextualPreprocessor(
            input_embedding_dim=D_IN, output_embedding_dim=D_OUT, contextual_feature_to_max_length=dict(CONTEXTUAL),
            contextual_feature_to_min_uih_length=dict(MIN_UIH), action_embedding_dim=ACTION_DIM, action_feature_name="actions",
            action_weights=list(ACTION_WEIGHTS), is_inference=is_inference)

    def mlp(in_dim, out_dim, contextual_dim, is_inf):
        if pmlp:
            return ParameterizedContextualizedMLP(contextual_embedding_dim=contextual_dim, sequential_input_dim=in_dim,
                                                  sequential_output_dim=out_dim, hidden_dim=HIDDEN, is_inference=is_inf)
        return SimpleContextualizedMLP(sequential_input_dim=in_dim, sequential_output_dim=out_dim, hidden_dim=HIDDEN,
                                       is_inference=is_inf)

    return ContextualInterleavePreprocessor(
        input_embedding_dim=D_IN, output_embedding_dim=D_OUT, contextual_feature_to_max_length=dict(CONTEXTUAL),
        contextual_feature_to_min_uih_length=dict(MIN_UIH),
        content_encoder=ContentEncoder(input_embedding_dim=D_IN, additional_content_features=dict(ADDITIONAL),
                                       target_enrich_features=dict(ENRICH), is_inference=is_inference),
        content_contextualize_mlp_fn=mlp,
        action_encoder=ActionEncoder(action_embedding_dim=ACTION_DIM, action_feature_name="actions",
                                     action_weights=list(ACTION_WEIGHTS), watchtime_feature_name="watchtimes",
                                     watchtime_to_action_thresholds_and_weights=list(ACTION_THRESHOLDS),
                                     is_inference=is_inference),
        action_contextualize_mlp_fn=mlp, pmlp_contextual_dropout_ratio=0.0, enable_interleaving=interleaving,
        is_inference=is_inference)


FLOAT_INPUTS = ("seq_embeddings", "c0", "c1", "a0", "t0")
OUT_NAMES = ("max_seq_len", "total_uih_len", "total_targets", "seq_lengths", "seq_offsets", "seq_timestamps", "seq_embeddings",
             "num_targets")


def module_case(name, seed):
    kind, interleaving, pmlp, is_inference, tags = MODULE_CASES[name]
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    B, total, n_tgt = len(LENGTHS), sum(LENGTHS), sum(TARGETS)
    uih = [l - t for l, t in zip(LENGTHS, TARGETS)]
    c_len = {"c0": [1, 0, 1, 1, 1], "c1": [2, 1, 0, 2, 2]}        # per-user rows of the contextual features (<= max length)
    inputs = dict(seq_embeddings=bf16_round(torch.randn(total, D_IN, generator=g)),
                  a0=bf16_round(torch.randn(total, ADDITIONAL["a0"], generator=g)),
                  t0=bf16_round(torch.randn(n_tgt, ENRICH["t0"], generator=g)))
    for k, lens in c_len.items():
        inputs[k] = bf16_round(torch.randn(sum(lens), D_IN, generator=g))
    ints = dict(c0_offsets=offsets_of(c_len["c0"]), c1_offsets=offsets_of(c_len["c1"]),
                actions=torch.randint(0, 16, (sum(uih),), generator=g), watchtimes=torch.randint(0, 60, (sum(uih),), generator=g),
                seq_lengths=torch.tensor(LENGTHS), num_targets=torch.tensor(TARGETS),
                seq_timestamps=torch.randint(1, 10**6, (total,), generator=g).sort().values)
    proto = build_module(kind, interleaving, pmlp, is_inference)
    sd = rounded_state_dict(proto, g)
    z = dict(kind=np.array(kind), enable_interleaving=np.int64(interleaving), parameterized=np.int64(pmlp),
             is_inference=np.int64(is_inference), max_uih_len=np.int64(max(uih)), max_targets=np.int64(max(TARGETS)),
             total_uih_len=np.int64(sum(uih)), total_targets=np.int64(n_tgt), sd_keys=np.array(list(sd)),
             param_keys=np.array([k for k, _ in proto.named_parameters()]))
    for k, v in inputs.items():
        z["in:" + k] = store(v, True)
    for k, v in ints.items():
        z["in:" + k] = v.numpy()
    for k, v in sd.items():
        z["sd:" + k] = store(v, v.is_floating_point())
    res, r = {}, None
    for tag in tags:
        dt = DTYPES[tag]
        m = build_module(kind, interleaving, pmlp, is_inference)
        m.load_state_dict(sd, strict=True)
        m.set_hammer_kernel(HammerKernel.PYTORCH)
        m = m.to(dt)
        m.set_training_dtype(dt)
        if tag == "f64":
            truth_norms(m)
        m.train(not is_inference)
        fl = {k: v.clone().to(dt).requires_grad_(not is_inference) for k, v in inputs.items()}
        seen = {}
        if kind == "interleave":
            inner = m.combine_embeddings

            def spy(**kw):
                seen.update(content=kw["content_embeddings"], action=kw["action_embeddings"],
                            contextual=kw["contextual_embeddings"])
                return inner(**kw)

            m.combine_embeddings = spy
        payloads = {k: v for k, v in fl.items() if k != "seq_embeddings"}
        payloads.update({k: ints[k] for k in ("c0_offsets", "c1_offsets", "actions", "watchtimes")})
        out = m(max_uih_len=max(uih), max_targets=max(TARGETS), total_uih_len=sum(uih), total_targets=n_tgt,
                seq_lengths=ints["seq_lengths"], seq_timestamps=ints["seq_timestamps"], seq_embeddings=fl["seq_embeddings"],
                num_targets=ints["num_targets"], seq_payloads=payloads)
        d = {"out:" + k: (torch.tensor(v) if isinstance(v, int) else v) for k, v in zip(OUT_NAMES, out[:8])}
        for k, v in seen.items():
            d["mlp:" + k] = v.reshape(B, -1, D_OUT) if k == "contextual" else v
        emb = out[6]
        if not is_inference:
            if r is None:
                r = torch.randn(emb.shape, generator=g)
                z["r"] = store(r)
            (emb * r.to(dt)).sum().backward()
            for k, v in fl.items():
                d["g:" + k] = v.grad if v.grad is not None else torch.zeros_like(v)
            for k, p in m.named_parameters():
                d["gp:" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
        res[tag] = d
    if "f64" in res:
        gated = [k for k in res["f64"] if k.startswith(("g:", "gp:")) or k == "out:seq_embeddings"]
        gated = [k for k in gated if float(res["f64"][k].detach().double().norm()) > 0.0]
        z["gated"] = np.array(gated)
        check_differs(name, res, gated)
    for tag, d in res.items():
        for k, v in d.items():
            z[f"{tag}:{k}"] = store(v)
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    set_dev_mode(True)
    torch.set_num_threads(1)   # one summation order whatever the host
    for n, name in enumerate(OP_CASES):
        np.savez_compressed(os.path.join(args.out, f"op_{name}.npz"), **op_case(name, 700 + n))
    for n, name in enumerate(MODULE_CASES):
        np.savez_compressed(os.path.join(args.out, f"module_{name}.npz"), **module_case(name, 800 + n))


if __name__ == "__main__":
    main()
