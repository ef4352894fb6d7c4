#!/usr/bin/env python3
"""Mint tests/golden/rms_norm/rms_norm.npz from the REFERENCE's own ``RMSNorm`` (ops/layer_norm.py:139-158, its PyTorch
branch, fp32, on the CPU).  Imports the unmodified reference the way make_golden.py does (build container only):

    python tests/golden/make_rms_norm_golden.py [--out DIR]

The fixture lives in a directory of its own: the .npz files directly under tests/golden/ are the set make_golden.py writes, and
tests/test_golden_regen.py holds the two sets equal.  tests/test_rms_norm_host.py regenerates this one the same way.

Per case: x (rows, dim), a non-trivial weight, g (the cotangent), eps, and y = RMSNorm(x), dx, dw of sum(y * g).
In fp32 the PyTorch branch and the Triton kernels this package follows compute the same function (the rounding to x's dtype
in front of the weight multiply is the identity), so the fixture binds ``rms_norm`` and the ``RMSNorm`` module in fp32."""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)

import numpy as np
import torch

import _fbgemm_shim  # noqa: F401  (registers torch.ops.fbgemm.*)

from generative_recommenders.common import HammerKernel  # noqa: E402
from generative_recommenders.ops.layer_norm import RMSNorm  # noqa: E402

EPS = 1e-5
SHAPES = [(7, 37), (33, 520)]


def rms_norm_cases():
    gen = torch.Generator().manual_seed(20251020)
    cases = []
    for rows, dim in SHAPES:
        x = (torch.randn(rows, dim, generator=gen) + 0.3).requires_grad_()
        w = 1.0 + 0.1 * torch.randn(dim, generator=gen)
        g = torch.randn(rows, dim, generator=gen)
        m = RMSNorm(dim, eps=EPS)
        m.set_hammer_kernel(HammerKernel.PYTORCH)
        assert m.hammer_kernel() == HammerKernel.PYTORCH
        with torch.no_grad():
            m.weight.copy_(w)
        y = m(x)
        (y * g).sum().backward()
        c = {name: t.detach().numpy().astype(np.float32) for name, t in (("x", x), ("w", w), ("g", g), ("y", y), ("dx", x.grad), ("dw", m.weight.grad))}
        c["eps"] = np.float32(EPS)
        cases.append(c)
    return cases


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "rms_norm"), help="directory rms_norm.npz is written to")
    args = ap.parse_args()
    torch.set_num_threads(1)
    cases = rms_norm_cases()
    flat = {f"c{i}:{key}": np.asarray(val) for i, c in enumerate(cases) for key, val in c.items()}
    flat["n_cases"] = np.asarray(len(cases))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "rms_norm.npz")
    np.savez_compressed(path, **flat)     # the layout of make_golden.py's _save_cases
    print(f"wrote {path}: {len(cases)} cases")


if __name__ == "__main__":
    main()
