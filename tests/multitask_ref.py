"""fp64 restatement of the multitask prediction head and of DefaultMultitaskModule (torch float64 + autograd over the
formulas of the issue; no code under test is involved), the loader of the fixtures under tests/golden/multitask/ and the
parity gate shared by the CPU and GPU tests."""

import glob
import os

import numpy as np
import torch

from conftest import GOLDEN

FIXTURES = os.path.join(GOLDEN, "multitask")
PARAMS = ("_prediction_module.0.weight", "_prediction_module.0.bias", "_prediction_module.1.weight",
          "_prediction_module.1.bias", "_prediction_module.2.weight", "_prediction_module.2.bias")
HEAD_GRADS = ("dx", "dg", "db", "dw", "dc")


def rel_fro(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def _f64(t):
    if t is None:
        return None
    t = torch.as_tensor(np.asarray(t)) if not torch.is_tensor(t) else t
    return t.detach().to("cpu", torch.float64)


def head_terms(x, g, b, eps, w, c, labels, weights, num_binary, loss_scale):
    """(preds (T, L), losses (T) or None) of the head in the dtype of its (torch) arguments"""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    z = (x - mean) / torch.sqrt(var + eps) * g + b
    y = x * torch.sigmoid(z)
    logits = (y @ w.t() + c).t()
    preds = torch.cat([torch.sigmoid(logits[:num_binary]), logits[num_binary:]], 0)
    if labels is None:
        return preds, None
    wt = torch.ones_like(labels) if weights is None else weights
    zb, lb = logits[:num_binary], labels[:num_binary]
    bce = torch.clamp(zb, min=0) - zb * lb + torch.log1p(torch.exp(-zb.abs()))
    mse = (logits[num_binary:] - labels[num_binary:]) ** 2
    per = torch.cat([bce, mse], 0) * wt
    return preds, per.sum(-1) / wt.sum(-1).clamp(min=1.0) * loss_scale


def head_fp64(x, g, b, eps, w, c, labels, weights, num_binary, loss_scale, r=None, grad_losses=True):
    """preds, losses and the gradients of  [losses.sum()] + (preds * r).sum()  w.r.t. x, g, b, w, c -- all numpy fp64"""
    x, g, b, w, c = (_f64(t).requires_grad_() for t in (x, g, b, w, c))
    labels, weights, r = _f64(labels), _f64(weights), _f64(r)
    preds, losses = head_terms(x, g, b, eps, w, c, labels, weights, num_binary, loss_scale)
    out = dict(preds=preds.detach().numpy())
    obj = 0.0
    if losses is not None:
        out["losses"] = losses.detach().numpy()
        if grad_losses:
            obj = obj + losses.sum()
    if r is not None:
        obj = obj + (preds * r).sum()
    if torch.is_tensor(obj):
        obj.backward()
        for name, t in zip(HEAD_GRADS, (x, g, b, w, c)):
            out[name] = np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    return out


def module_fp64(u, i, params, labels, weights, num_binary, loss_scale, r, eps=1e-5):
    """DefaultMultitaskModule with Linear -> SwishLayerNorm -> Linear in fp64: preds, losses, and the gradients of
    losses.sum() + (preds * r).sum() w.r.t. u, i (`gu`, `gi`) and every parameter (`gp:<state_dict name>`)"""
    u, i = _f64(u).requires_grad_(), _f64(i).requires_grad_()
    p = {k: _f64(params[k]).requires_grad_() for k in PARAMS}
    h = (u * i) @ p[PARAMS[0]].t() + p[PARAMS[1]]
    preds, losses = head_terms(h, p[PARAMS[2]], p[PARAMS[3]], eps, p[PARAMS[4]], p[PARAMS[5]], _f64(labels), _f64(weights),
                               num_binary, loss_scale)
    (losses.sum() + (preds * _f64(r)).sum()).backward()
    out = dict(preds=preds.detach().numpy(), losses=losses.detach().numpy(), gu=u.grad.numpy(), gi=i.grad.numpy())
    for k in PARAMS:
        out["gp:" + k] = p[k].grad.numpy()
    return out


def single_linear_fp64(u, i, w, c, labels, weights, num_binary, loss_scale):
    """a prediction module that is ONE Linear(D, T): logits = (u * i) W^T + c, then the same predictions and losses"""
    logits = ((_f64(u) * _f64(i)) @ _f64(w).t() + _f64(c)).t()
    labels, weights = _f64(labels), _f64(weights)
    preds = torch.cat([torch.sigmoid(logits[:num_binary]), logits[num_binary:]], 0)
    zb, lb = logits[:num_binary], labels[:num_binary]
    per = torch.cat([torch.clamp(zb, min=0) - zb * lb + torch.log1p(torch.exp(-zb.abs())),
                     (logits[num_binary:] - labels[num_binary:]) ** 2], 0) * weights
    return preds.numpy(), (per.sum(-1) / weights.sum(-1).clamp(min=1.0) * loss_scale).numpy()


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _widen(a):
    """bf16 bit patterns (uint16) -> the float32 values they stand for"""
    return (a.astype(np.uint32) << 16).view(np.float32) if a.dtype == np.uint16 else a


def case_files():
    return sorted(glob.glob(os.path.join(FIXTURES, "case_*.npz")))


def load_case(path):
    z = np.load(path, allow_pickle=False)
    c = {k: _widen(z[k]) for k in z.files}
    c["name"] = os.path.basename(path)[5:-4]
    c["task_names"] = [str(s) for s in z["task_names"]]
    c["task_types"] = [int(t) for t in z["task_types"]]
    c["weighted_tasks"] = [str(s) for s in z["weighted_tasks"]]
    c["num_binary"] = sum(1 for t in c["task_types"] if t == 0)
    c["cmw"] = float(z["cmw"])
    c["params"] = {k: c["sd:" + k] for k in PARAMS}
    c["labels_tl"] = np.stack([c["label:" + n] for n in c["task_names"]])
    ones = np.ones(c["u"].shape[0], dtype=np.float32)
    c["weights_tl"] = np.stack([c["weight:" + n] if n in c["weighted_tasks"] else ones for n in c["task_names"]])
    return c


def result_names():
    return ("preds", "losses", "gu", "gi") + tuple("gp:" + k for k in PARAMS)


def load_names():
    z = np.load(os.path.join(FIXTURES, "reference_names.npz"), allow_pickle=False)
    return {k: [str(s) for s in z[k]] for k in z.files}


# ---------------------------------------------------------------------------------------------------------------- the gate
# sqrt of the 99 % point of the F(n, n) distribution, n = 1 .. 8 (F tables: 4052, 99.0, 29.46, 15.98, 10.97, 8.47, 6.99, 6.03)
_RATIO_Q99 = {1: 63.7, 2: 9.95, 3: 5.43, 4: 4.00, 5: 3.31, 6: 2.91, 7: 2.64, 8: 2.46}


def gate_multiplier(dtype_name, n_elements):
    """e_hip <= m * e_ref, e = relative Frobenius error against the fp64 truth, per tensor of n_elements numbers.

    16-bit (m = 1.5, the precedent of tests/jagged_bmm_ref.py): the reference rounds y, the logits and every gradient on
    the way to the activation dtype; the kernel keeps them in fp32 and rounds only what it stores, so it should sit at or
    below the reference -- 1.5 covers a tensor on which both sit on the same output-rounding floor and differ by the draw.
    fp32 (m = 8): e_ref is summation-order and libm noise itself (~1e-7); another order over 512 terms, or over the rows,
    may legitimately be several times larger.

    Tensors of n <= 8 numbers (`losses` and the gradient of the last bias: one number per task) get max(m, q(n)).  Both
    errors are then the norm of n rounding outcomes, not an average over many, and the two sides do not share them (their
    first GEMMs round different bits): even with EQUAL error scales e_hip / e_ref is the ratio of two independent chi(n)
    variables, i.e. sqrt(F(n, n)).  For n = 1 that is |Cauchy|: it exceeds 1.5 in 37 % and 8 in 8 % of all draws -- the
    plain gate would fail a correct kernel on one single-task fixture in three.  q(n) is the 99 % point of that ratio
    (63.7, 9.95, 5.43, 4.00, 3.31 for n = 1 .. 5): a gate that a kernel as accurate as the reference passes 99 times in
    100, whatever the draw.  It is weak for one number by necessity; what a loss must equal is checked to 4e-6 against the
    restatement at the op level (test_op_against_the_restatement), where no draw is involved."""
    m = 8.0 if dtype_name == "float32" else 1.5
    return max(m, _RATIO_Q99.get(int(n_elements), 0.0))
