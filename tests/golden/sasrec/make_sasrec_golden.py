#!/usr/bin/env python3
"""Mint the fixtures of the SASRec baseline (tests/golden/sasrec/) on the CPU.

Run in the build container only (the model cases need /root/reference):

    python tests/golden/sasrec/make_sasrec_golden.py [--out DIR]

Op cases (``op_<n>_...``): torch's math path as ``torch.nn.MultiheadAttention`` takes it with ``need_weights=True`` (scaled q,
``baddbmm`` onto a -inf causal mask, ``softmax``, ``bmm``; tests/softmax_attn_ref.py ``math_path``) on the padded batch,
without dropout, in fp64 (the truth), fp32 and bf16.  Stored: q, k, v, dO, the lengths and out, dq, dk, dv at the valid
rows.  The maker asserts on its first case that ``math_path`` equals ``torch.nn.functional.multi_head_attention_forward``
with identity projections bit for bit.

Model cases (``model_<x>_...``): ``generative_recommenders.research.modeling.sequential.sasrec.SASRec``, imported
unmodified (``_fbgemm_shim`` stands in for the absent fbgemm ops), in fp64, fp32 and bf16 with ``ffn_dropout_rate = 0``.  All
1-D parameters are re-drawn from a seeded normal (``reset_state`` leaves the attention biases at zero).  The preprocessor
stand-in returns a stored (B, N, D) tensor zeroed past each length, the postprocessor stand-in is the identity.  Stored: the
inputs, the state dict, a random r, and for loss = sum(out r) the output and the gradient of every parameter and of the
stored embeddings, per tag.  ``reference_names.npz``: state-dict keys and shapes.  ``bf16:relu_flips``: per block, the number
of ReLU units (all rows) that are open in the reference's bf16 run and closed in its fp64 run or the
other way round, read off the first convolution's output by a forward hook; 0 for gelu.

Every input value is representable in bf16, so only the arithmetic differs between the tags.  16-bit values are stored as
bf16 bit patterns; a case is spread over several files (``<case>__<group>.npz``) so that each stays small.
"""

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))                      # tests/golden: _fbgemm_shim
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # tests: softmax_attn_ref

import numpy as np
import torch

import _fbgemm_shim  # noqa: F401  (registers torch.ops.fbgemm.*)
import softmax_attn_ref as R

OP_CASES = [
    # (name, H, d, N, lengths)
    ("op_1_h2_d16_n70", 2, 16, 70, [0, 1, 2, 31, 32, 33, 64, 65, 70]),
    ("op_2_h1_d50_n210", 1, 50, 210, [210, 129, 128, 7]),
    ("op_3_h4_d64_n130", 4, 64, 130, [130, 96, 1]),
    ("op_4_h1_d64_n510", 1, 64, 510, [510, 257, 3]),
]
MODEL_CASES = [
    # (name, D, H, blocks, activation, hidden, N, lengths)
    ("model_a_d48_h3_gelu", 48, 3, 2, "gelu", 40, 40, [40, 1, 0, 17, 33]),
    ("model_b_d50_h1_relu", 50, 1, 2, "relu", 50, 70, [70, 64, 65, 2]),
]


def bf16_exact(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def store(tag, t):
    t = t.detach()
    return R.to_bits(t) if tag == "bf16" else t.numpy().copy()


# ---------------------------------------------------------------------------------------------------------------- op cases
def check_math_path_is_mha(q, k, v, lengths, n):
    """math_path == F.multi_head_attention_forward (identity projections, need_weights=True), fp32, bit for bit"""
    L, H, d = q.shape
    E = H * d
    pad = lambda x: torch.stack([torch.cat([x[o:o + ln], x.new_zeros((n - ln, H, d))]) for o, ln in
                                 zip(R.offsets_of(lengths)[:-1].tolist(), lengths)]).reshape(len(lengths), n, E)
    tq, tk, tv = (torch.from_numpy(x).float() for x in (q, k, v))
    eye = torch.eye(E)
    out, _ = torch.nn.functional.multi_head_attention_forward(
        pad(tq).transpose(0, 1), pad(tk).transpose(0, 1), pad(tv).transpose(0, 1), E, H, in_proj_weight=None,
        in_proj_bias=None, bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0.0, out_proj_weight=eye,
        out_proj_bias=None, training=False, need_weights=True,
        attn_mask=torch.triu(torch.ones((n, n), dtype=torch.bool), diagonal=1), use_separate_proj_weight=True,
        q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)
    out = out.transpose(0, 1).reshape(len(lengths), n, H, d)
    mine = R.math_path(q, k, v, np.zeros_like(q), lengths, n, torch.float32)["out"]
    got = torch.cat([out[b, :ln] for b, ln in enumerate(lengths)]).double().numpy()
    assert np.array_equal(got, mine), "math_path is not what nn.MultiheadAttention computes"


def make_op_case(idx, name, H, d, n, lengths, out_dir):
    g = torch.Generator().manual_seed(1000 + idx)
    L = sum(lengths)
    q, k, v, dout = (bf16_exact(torch.randn((L, H, d), generator=g, dtype=torch.float64)).numpy() for _ in range(4))
    if idx == 0:
        check_math_path_is_mha(q, k, v, lengths, n)
    groups = {"in": {"lengths": np.asarray(lengths, dtype=np.int64), "max_seq_len": np.asarray(n, dtype=np.int64)}}
    for key, x in (("q", q), ("k", k), ("v", v), ("dout", dout)):
        groups["in"][key] = R.to_bits(torch.from_numpy(x))
    for tag in R.TAGS:
        res = R.math_path(q, k, v, dout, lengths, n, R.TORCH_DTYPE[tag])
        for gname in R.GRADS:
            arr = res[gname]
            val = R.to_bits(torch.from_numpy(arr)) if tag == "bf16" else arr.astype(np.float32 if tag == "f32" else np.float64)
            grp = tag if tag != "f64" else ("f64a" if gname in ("out", "dq") else "f64b")     # the fp64 truth in two files
            groups.setdefault(grp, {})[f"{tag}:{gname}"] = val
    for grp, arrays in groups.items():
        np.savez_compressed(os.path.join(out_dir, f"{name}__{grp}.npz"), **arrays)


# ------------------------------------------------------------------------------------------------------------- model cases
class _Embedding(torch.nn.Module):
    def __init__(self, dim):
        super().__init__()
        self._dim = dim

    @property
    def item_embedding_dim(self):
        return self._dim

    def get_item_embeddings(self, item_ids):
        raise NotImplementedError

    def debug_str(self):
        return "stub_emb"


class _Preproc(torch.nn.Module):
    """returns the stored (B, N, D) tensor zeroed past each length"""

    def __init__(self):
        super().__init__()
        self.emb = None

    def debug_str(self):
        return "stub_pre"

    def forward(self, past_lengths, past_ids, past_embeddings, past_payloads):
        n = self.emb.shape[1]
        valid = (torch.arange(n).view(1, -1) < past_lengths.view(-1, 1)).unsqueeze(-1).to(self.emb.dtype)
        return past_lengths, self.emb * valid, valid


class _Postproc(torch.nn.Module):
    def debug_str(self):
        return "stub_post"

    def forward(self, x):
        return x


def make_model_case(idx, name, D, H, blocks, act, hidden, n, lengths, out_dir, names):
    from generative_recommenders.research.modeling.sequential.sasrec import SASRec

    torch.manual_seed(2000 + idx)
    pre = _Preproc()
    model = SASRec(max_sequence_len=n - 2, max_output_len=2, embedding_dim=D, num_blocks=blocks, num_heads=H, ffn_hidden_dim=hidden,
                   ffn_activation_fn=act, ffn_dropout_rate=0.0, embedding_module=_Embedding(D), similarity_module=torch.nn.Identity(),
                   input_features_preproc_module=pre, output_postproc_module=_Postproc())
    g = torch.Generator().manual_seed(3000 + idx)
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            p.copy_(bf16_exact(p))
    B = len(lengths)
    emb = bf16_exact(torch.randn((B, n, D), generator=g, dtype=torch.float64))
    r = bf16_exact(torch.randn((B, n, D), generator=g, dtype=torch.float64))
    lens = torch.tensor(lengths, dtype=torch.int64)
    sd = {k_: v_.detach().clone() for k_, v_ in model.state_dict().items()}
    if not names:
        names["keys"] = np.array(list(sd))
        names["blocks"] = np.asarray(blocks)
    names[f"{name}:shapes"] = np.array([",".join(map(str, v_.shape)) for v_ in sd.values()])
    arrays = {"lengths": lens.numpy(), "emb": R.to_bits(emb), "r": R.to_bits(r), "sd_keys": np.array(list(sd)),
              "config": np.array([D, H, blocks, hidden, n], dtype=np.int64), "activation": np.array(act)}
    for k_, v_ in sd.items():
        arrays["sd:" + k_] = v_.numpy().astype(np.uint8) if v_.dtype == torch.bool else R.to_bits(v_)
    hidden = {}
    for i in range(blocks):       # pre-activations of every feed-forward, per tag (recorded by a hook; nothing is modified)
        model.forward_layers[i]._conv1d[0].register_forward_hook(
            lambda _m, _i, o, i=i: hidden.setdefault(tag_now[0], {}).__setitem__(i, o.detach().double()))
    tag_now = [None]
    for tag in R.TAGS:
        tag_now[0] = tag
        dt = R.TORCH_DTYPE[tag]
        model.to(dt)
        model.zero_grad(set_to_none=True)
        pre.emb = emb.detach().to(dt).clone().requires_grad_(True)
        out = model(lens, None, None, {})
        (out * r.to(dt)).sum().backward()
        arrays[f"{tag}:out"] = store(tag, out.to(dt) if tag == "bf16" else out)
        arrays[f"{tag}:g:emb"] = store(tag, pre.emb.grad)
        for k_, p in model.named_parameters():
            arrays[f"{tag}:g:{k_}"] = store(tag, p.grad)
    # ReLU units whose gate in the reference's own bf16 run differs from the truth (softmax_attn_ref.model_multiplier)
    flips = [int(((hidden["bf16"][i] > 0) != (hidden["f64"][i] > 0)).sum()) if act == "relu" else 0 for i in range(blocks)]
    arrays["bf16:relu_flips"] = np.asarray(flips, dtype=np.int64)
    np.savez_compressed(os.path.join(out_dir, f"{name}__all.npz"), **arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(1)                       # one summation order, whatever the machine
    for i, c in enumerate(OP_CASES):
        make_op_case(i, *c, args.out)
    names = {}
    for i, c in enumerate(MODEL_CASES):
        make_model_case(i, *c, args.out, names)
    np.savez_compressed(os.path.join(args.out, "reference_names.npz"), **names)


if __name__ == "__main__":
    main()
