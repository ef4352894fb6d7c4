#!/usr/bin/env python3
"""Mint the fixtures of the multitask prediction head from the REFERENCE's DefaultMultitaskModule (PyTorch path, CPU).

Run in the build container only (needs /root/reference):

    python tests/golden/multitask/make_multitask_golden.py [--out DIR]

``generative_recommenders.modules.multitask_module`` is imported unmodified (``_fbgemm_shim`` stands in for the absent fbgemm
ops, as in ``tests/golden/make_golden.py``).  Per case the module of modules/dlrm_hstu.py:139-149 (Linear(64, 512) ->
SwishLayerNorm(512) -> Linear(512, T)) runs three times on the SAME values -- inputs and parameters are rounded to
bf16-representable numbers first, so only the arithmetic differs:

* fp32 as it is,
* bf16 after ``module.to(torch.bfloat16)`` (the CPU ignores ``autocast("cuda")``; without the cast the first Linear raises a
  dtype mismatch),
* fp64, the truth, after ``module.to(torch.float64)`` with float64 labels and weights (otherwise
  ``mt_logits.to(mt_labels.dtype)`` drops the loss to fp32).  The reference's own SwishLayerNorm cannot take part in this
  run: its PyTorch path casts x to float32 whatever comes in (ops/pytorch/pt_layer_norm.py:48-61), which would leave the
  "truth" at fp32 accuracy (2e-8).  The truth's ``prediction_fn`` therefore puts ``SwishLayerNormTruth`` -- the same formula
  and parameter names in the dtype of its input, defined below -- between the two Linears; everything else (the module,
  its predictions, labels, weights and losses) is the reference's code, unmodified.

Stored per run: preds, losses and the gradients of ``losses.sum() + (preds * r).sum()`` (r stored) with respect to u, i and
every parameter.  Every stored tensor of the fp32 and bf16 runs must differ from the truth (asserted here): a zero
reference error would make a relative gate vacuous.  The task lists are the seven of
modules/tests/multitask_module_test.py:37-134 (D = 64, causal_multitask_weights = 0.3 as there), L in {1, 37, 200}, labels
randint(0, 11) for binary and randn for regression tasks, weights for a subset of the tasks -- among them one task whose
weights sum to less than 1 (the clamp) and one with all-zero weights.  16-bit values are stored as bf16 bit patterns."""

import argparse
import inspect
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import _fbgemm_shim  # noqa: F401  (registers torch.ops.fbgemm.*)

from generative_recommenders.common import HammerKernel, set_dev_mode  # noqa: E402
from generative_recommenders.modules import multitask_module as M  # noqa: E402
from generative_recommenders.ops.layer_norm import SwishLayerNorm  # noqa: E402

B, R = M.MultitaskTaskType.BINARY_CLASSIFICATION, M.MultitaskTaskType.REGRESSION
TASK_LISTS = [
    [("is_click", 1, B)],
    [("vvp", 2, R)],
    [("is_click", 1, B), ("is_like", 2, B), ("is_follow", 4, B)],
    [("rating", 1, R), ("vvp", 2, R)],
    [("type_1", 2, R)],
    [("is_click", 1, B), ("is_like", 2, B), ("is_follow", 4, B), ("rating", 1, R), ("vvp", 2, R)],
    [("is_click", 1, B), ("is_like", 2, B), ("is_follow", 4, B), ("rating", 1, R), ("vvp", 2, R)],
]
# case -> (task list, L, {task: kind of weights}); "rand": uniform(0, 2), "small": sums to < 1, "zero": all zero
CASES = {
    "0_click_L200": (0, 200, {}),
    "1_vvp_L37": (1, 37, {"vvp": "rand"}),
    "2_bin3_L1": (2, 1, {"is_like": "rand"}),
    "3_reg2_L200": (3, 200, {"rating": "small"}),
    "4_type1_L37": (4, 37, {"type_1": "small"}),
    "5_mixed_L200": (5, 200, {"is_click": "rand", "is_like": "zero", "vvp": "rand"}),
    "6_mixed_L37": (6, 37, {"is_follow": "small", "rating": "rand"}),
}
D, HIDDEN, CMW = 64, 512, 0.3
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}


class SwishLayerNormTruth(torch.nn.Module):
    """x * sigmoid(layer_norm(x)) in x's dtype, parameters named as the reference's SwishLayerNorm names them"""

    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(dim))
        self.bias = torch.nn.Parameter(torch.zeros(dim))
        self._dim, self._eps = dim, eps

    def forward(self, x):
        return x * torch.sigmoid(torch.nn.functional.layer_norm(x, [self._dim], self.weight, self.bias, self._eps))


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def store(t, as_bf16=False):
    t = t.detach().contiguous()
    if as_bf16 or t.dtype == torch.bfloat16:
        return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def run(configs, sd, u, i, labels, weights, r, dtype):
    m = M.DefaultMultitaskModule(
        task_configs=configs, embedding_dim=D,
        prediction_fn=lambda in_dim, num_tasks: torch.nn.Sequential(
            torch.nn.Linear(in_features=in_dim, out_features=HIDDEN),
            SwishLayerNormTruth(HIDDEN) if dtype == torch.float64 else SwishLayerNorm(HIDDEN),
            torch.nn.Linear(in_features=HIDDEN, out_features=num_tasks)),
        causal_multitask_weights=CMW, is_inference=False)
    m.load_state_dict(sd, strict=True)
    m.set_hammer_kernel(HammerKernel.PYTORCH)
    m = m.to(dtype)
    m.set_training_dtype(dtype)
    side = torch.float64 if dtype == torch.float64 else torch.float32
    u, i = u.clone().to(dtype).requires_grad_(), i.clone().to(dtype).requires_grad_()
    preds, _, _, losses = m(u, i, {k: v.to(side) for k, v in labels.items()}, {k: v.to(side) for k, v in weights.items()})
    (losses.sum() + (preds * r.to(side)).sum()).backward()
    out = dict(preds=preds, losses=losses, gu=u.grad, gi=i.grad)
    for k, p in m.named_parameters():
        out["gp:" + k] = p.grad
    return out


def make_case(name, seed):
    li, L, wkinds = CASES[name]
    configs = [M.TaskConfig(task_name=n, task_weight=w, task_type=t) for n, w, t in TASK_LISTS[li]]
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    proto = torch.nn.Sequential(torch.nn.Linear(D, HIDDEN), SwishLayerNorm(HIDDEN), torch.nn.Linear(HIDDEN, len(configs)))
    sd = {}
    for k, v in proto.state_dict().items():
        # the norm starts at (1, 0) and the biases small: move every parameter off its default so that a swapped or dropped one shows
        sd["_prediction_module." + k] = bf16_round(v + 0.1 * torch.randn(v.shape, generator=g))
    u, i = bf16_round(torch.randn(L, D, generator=g)), bf16_round(torch.randn(L, D, generator=g))
    labels, weights = {}, {}
    for c in configs:
        if c.task_type == R:
            labels[c.task_name] = bf16_round(torch.randn(L, generator=g))
        else:
            labels[c.task_name] = torch.randint(0, 11, (L,), generator=g).to(torch.float32)
        kind = wkinds.get(c.task_name)
        if kind == "rand":
            weights[c.task_name] = bf16_round(2 * torch.rand(L, generator=g))
        elif kind == "small":
            weights[c.task_name] = bf16_round(0.5 * torch.rand(L, generator=g) / L)
        elif kind == "zero":
            weights[c.task_name] = torch.zeros(L)
    r = bf16_round(torch.randn(len(configs), L, generator=g))
    z = dict(cmw=np.float64(CMW), task_names=np.array([c.task_name for c in configs]),
             task_types=np.array([int(c.task_type) for c in configs], dtype=np.int64),
             weighted_tasks=np.array(sorted(weights), dtype="U16"), u=store(u, True), i=store(i, True), r=store(r, True))
    for k, v in sd.items():
        z["sd:" + k] = store(v, True)
    for k, v in labels.items():
        z["label:" + k] = store(v)
    for k, v in weights.items():
        z["weight:" + k] = store(v)
    res = {tag: run(configs, sd, u, i, labels, weights, r, dt) for tag, dt in DTYPES.items()}
    for tag in ("f32", "bf16"):
        for k, v in res[tag].items():
            truth = res["f64"][k].detach().double()
            err = float((v.detach().double() - truth).norm() / truth.norm())
            assert err > 0.0, f"{name}: {tag}:{k} equals the fp64 truth exactly: a relative gate on it would be vacuous"
    for tag, d in res.items():
        for k, v in d.items():
            z[f"{tag}:{k}"] = store(v)
    return z


def reference_names():
    """what a drop-in has to reproduce by name: the enum, the dataclass fields, the two signatures, the state_dict keys"""
    m = M.DefaultMultitaskModule(
        task_configs=[M.TaskConfig("a", 1, B)], embedding_dim=8,
        prediction_fn=lambda in_dim, num_tasks: torch.nn.Sequential(
            torch.nn.Linear(in_dim, 16), SwishLayerNorm(16), torch.nn.Linear(16, num_tasks)),
        causal_multitask_weights=1.0, is_inference=False)
    return dict(
        task_types=np.array([f"{e.name}={int(e)}" for e in M.MultitaskTaskType]),
        task_config_fields=np.array([f.name for f in M.TaskConfig.__dataclass_fields__.values()]),
        init_args=np.array(list(inspect.signature(M.DefaultMultitaskModule.__init__).parameters)),
        forward_args=np.array(list(inspect.signature(M.DefaultMultitaskModule.forward).parameters)),
        base_forward_args=np.array(list(inspect.signature(M.MultitaskModule.forward).parameters)),
        state_dict_keys=np.array(list(m.state_dict())),
    )


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    set_dev_mode(True)
    torch.set_num_threads(1)   # one summation order whatever the host
    for n, name in enumerate(CASES):
        np.savez_compressed(os.path.join(args.out, f"case_{name}.npz"), **make_case(name, 500 + n))
    np.savez_compressed(os.path.join(args.out, "reference_names.npz"), **reference_names())


if __name__ == "__main__":
    main()
