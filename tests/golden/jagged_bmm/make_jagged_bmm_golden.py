#!/usr/bin/env python3
"""Mint the fixtures of jagged_dense_bmm_broadcast_add and the contextualized MLPs from the REFERENCE's PyTorch path.

Run in the build container only (needs /root/reference):

    python tests/golden/jagged_bmm/make_jagged_bmm_golden.py [--out DIR]

Like ``tests/golden/make_golden.py`` it imports ``generative_recommenders`` unmodified with ``_fbgemm_shim`` standing in
for the absent fbgemm ops; ``modules/contextualize_mlps.py`` also imports ``libfb.py.pyre.none_throws``, which is not in
the open tree, so a stand-in is planted in ``sys.modules`` first.  Inputs follow the reference test
(ops/tests/jagged_tensors_test.py:603-700): uniform(-1, 1) operands, 0.01 * randn for d_out, an empty user planted on
purpose.  One ``.npz`` per case; 16-bit tensors are stored in 16 bits (bf16 as its uint16 bit pattern)."""

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

from generative_recommenders.common import HammerKernel  # noqa: E402
from generative_recommenders.modules.contextualize_mlps import (  # noqa: E402
    ParameterizedContextualizedMLP,
    SimpleContextualizedMLP,
)
from generative_recommenders.ops.jagged_tensors import jagged_dense_bmm_broadcast_add  # noqa: E402

PT = HammerKernel.PYTORCH
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}

# name -> (K, N, max_seq_len, lengths, offsets dtype, dense stored as (B, N, K) and passed transposed)
OP_CASES = {
    "odd_37x23": (37, 23, 57, [31, 0, 1, 57, 12, 44], torch.int64, False),      # empty, one-row and max_seq_len users
    "odd_37x23_i32_t": (37, 23, 57, [9, 57, 0, 26], torch.int32, True),
    "sq_200": (200, 200, 40, [40, 13], torch.int32, False),
    "aligned_64x512": (64, 512, 24, [20, 0, 9], torch.int64, True),
    "small_24x40": (24, 40, 33, [33, 5, 0, 17, 1], torch.int32, False),
}


def store(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def op_case(name, dtype_name, seed):
    K, N, max_seq_len, lengths, odt, transposed = OP_CASES[name]
    dtype = DTYPES[dtype_name]
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    off = torch.zeros(B + 1, dtype=odt)
    off[1:] = torch.cumsum(torch.tensor(lengths), 0)
    L = int(off[-1])
    jagged = torch.empty(L, K).uniform_(-1, 1, generator=g).to(dtype).requires_grad_()
    if transposed:
        storage = torch.empty(B, N, K).uniform_(-1, 1, generator=g).to(dtype).requires_grad_()
        dense = storage.transpose(1, 2)
    else:
        storage = torch.empty(B, K, N).uniform_(-1, 1, generator=g).to(dtype).requires_grad_()
        dense = storage
    bias = torch.empty(B, N).uniform_(-1, 1, generator=g).to(dtype).requires_grad_()
    d_out = (torch.randn(L, N, generator=g) * 0.01).to(dtype)
    out = jagged_dense_bmm_broadcast_add(max_seq_len, off, jagged, dense, bias, kernel=PT)
    out.backward(d_out)
    d_dense = storage.grad.transpose(1, 2) if transposed else storage.grad
    return dict(dtype=np.array(dtype_name), max_seq_len=np.int64(max_seq_len), seq_offsets=off.numpy(),
                dense_transposed=np.int64(transposed), jagged=store(jagged), dense=store(dense), bias=store(bias),
                d_out=store(d_out), out=store(out), d_jagged=store(jagged.grad), d_dense=store(d_dense),
                d_bias=store(bias.grad))


def module_case(kind, seed):
    torch.manual_seed(seed)
    if kind == "parameterized":
        m = ParameterizedContextualizedMLP(contextual_embedding_dim=48, sequential_input_dim=24, sequential_output_dim=40,
                                           hidden_dim=32)
    else:
        m = SimpleContextualizedMLP(sequential_input_dim=24, sequential_output_dim=40, hidden_dim=32)
    m.set_hammer_kernel(PT)
    g = torch.Generator().manual_seed(seed + 1)
    # the reference initialises biases to zero and norms to (1, 0): move every parameter off its default so that a
    # swapped or dropped one shows
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    lengths = torch.tensor([5, 0, 17, 9])
    off = torch.zeros(5, dtype=torch.int64)
    off[1:] = lengths.cumsum(0)
    x = torch.randn(int(off[-1]), 24, generator=g).requires_grad_()
    c = torch.randn(4, 48, generator=g).requires_grad_()
    y = m(seq_embeddings=x, seq_offsets=off, max_seq_len=17, contextual_embeddings=c)
    dy = torch.randn(y.shape, generator=g) * 0.1
    y.backward(dy)
    z = dict(max_seq_len=np.int64(17), seq_offsets=off.numpy(), x=store(x), c=store(c), y=store(y), dy=store(dy),
             gx=store(x.grad))
    if c.grad is not None:
        z["gc"] = store(c.grad)
    for k, v in m.state_dict().items():
        z["sd:" + k] = store(v)
    for k, p in m.named_parameters():
        z["gp:" + k] = store(p.grad)
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    seed = 100
    for dtype_name in DTYPES:
        for name in OP_CASES:
            seed += 1
            np.savez_compressed(os.path.join(args.out, f"op_{dtype_name}_{name}.npz"), **op_case(name, dtype_name, seed))
    np.savez_compressed(os.path.join(args.out, "module_parameterized.npz"), **module_case("parameterized", 7))
    np.savez_compressed(os.path.join(args.out, "module_simple.npz"), **module_case("simple", 11))


if __name__ == "__main__":
    main()
