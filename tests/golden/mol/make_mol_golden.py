#!/usr/bin/env python3
"""Mint the Mixture-of-Logits fixtures from the REFERENCE's modules on the CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/mol/make_mol_golden.py [--out DIR]

The reference is imported unmodified.  Two things make that possible without its optional dependencies:
``TORCHDYNAMO_DISABLE=1`` is set before torch is imported, so its ``@torch.compile`` decorators are inert, and a stand-in
``gin`` module whose ``configurable`` passes the function through sits in ``sys.modules``.

Per case (P_Q, P_X, D_P, H, combination, B, X) one module is built with ``create_mol_interaction_module``; its biases,
which the factory zeroes, get a non-zero draw.  Stored:

* ``<case>.module``: the fp32 ``state_dict`` (``sd:<key>``) and its key order, the raw queries, items and item ids, and
  from the module's ``.double()`` copy the scores, ``mi_loss`` (train mode, every dropout rate 0) and the gradient of
  ``scores.sum()`` with respect to the queries;
* ``<case>.<dtype>`` for fp32, bf16 and fp16: the operands of ``hstu_mol_scores`` exactly as the reference's submodules
  produce them at that dtype -- ``qc``, ``xc``, ``gq``, ``gi`` and the ``_qi_partial_module`` weights -- the reference's
  scores at that dtype (``ref``), an fp64 evaluation of the SAME stored operands (``s64``: the reference's own
  ``_qi_partial_module`` cast to double and its ``SoftmaxDropoutCombiner``) and ``e_ref = max |ref - s64|``.  The fp64
  evaluation procedure is itself checked: fed the operands of the ``.double()`` module it reproduces that module's
  forward to 1e-12.

Asserted while minting: 16 e_ref(fp32) < 1e-3 max|s| and e_ref(16-bit) < 0.1 max|s|, so that a gate set from e_ref cannot
hide a wrong term.  16-bit arrays are stored as their int16 bit patterns.  A group of arrays is written as one or more
``.partN.npz`` files of at most 300 kB each (larger arrays are cut along their first axis), with fixed zip timestamps:
the files regenerate bit for bit."""

import argparse
import copy
import io
import os
import sys
import types
import zipfile

os.environ["TORCHDYNAMO_DISABLE"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

_gin = types.ModuleType("gin")
_gin.configurable = lambda f=None, **kw: f if callable(f) else (lambda g: g)
sys.modules["gin"] = _gin

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from generative_recommenders.research.modeling.similarity_utils import create_mol_interaction_module  # noqa: E402
from generative_recommenders.research.rails.indexing.mol_top_k import MoLBruteForceTopK  # noqa: E402

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
TEMPERATURE = 0.05
QUERY_DIM, ITEM_DIM = 24, 20

# (P_Q, P_X, D_P, H, combination, B, X)
CASES = [
    (1, 1, 8, 0, "glu_silu", 1, 1),
    (4, 2, 16, 16, "glu_silu", 5, 70),
    (3, 5, 10, 100, "glu_silu_ln", 65, 257),
    (8, 8, 32, 128, "glu_silu", 33, 1000),
    (8, 8, 64, 0, "glu_silu_ln", 17, 513),
]
PART_BYTES = 300_000


def case_name(pq, px, dp, h, comb, B, X):
    return f"mol_{pq}x{px}x{dp}_h{h}_{comb}_b{B}_x{X}"


def factory_kwargs(pq, px, dp, h, comb):
    return dict(query_embedding_dim=QUERY_DIM, item_embedding_dim=ITEM_DIM, dot_product_dimension=dp, query_dot_product_groups=pq,
                item_dot_product_groups=px, temperature=TEMPERATURE, query_dropout_rate=0.0, query_hidden_dim=32,
                item_dropout_rate=0.0, item_hidden_dim=32, gating_query_hidden_dim=16, gating_qi_hidden_dim=h,
                gating_item_hidden_dim=16, softmax_dropout_rate=0.0, bf16_training=False, gating_combination_type=comb)


def to_numpy(t):
    t = t.detach().contiguous()
    return t.view(torch.int16).numpy() if t.dtype in (torch.bfloat16, torch.float16) else t.numpy()


def write_parts(out_dir, name, arrays):
    """name.partN.npz, each a group of arrays of at most PART_BYTES, deflated, with fixed timestamps; a larger array is cut
    along its first axis into ``key@0``, ``key@1``, ... (the loader concatenates them)"""
    pieces = {}
    for key, a in arrays.items():
        a = np.asarray(a, order="C")
        n = -(-a.nbytes // PART_BYTES)
        if n <= 1:
            pieces[key] = a
        else:
            pieces.update({f"{key}@{i}": c for i, c in enumerate(np.array_split(a, n, axis=0))})
    groups, cur, size = [], {}, 0
    for key, a in pieces.items():
        a = np.asarray(a, order="C")
        if cur and size + a.nbytes > PART_BYTES:
            groups.append(cur)
            cur, size = {}, 0
        cur[key] = a
        size += a.nbytes
    groups.append(cur)
    for i, g in enumerate(groups):
        with zipfile.ZipFile(os.path.join(out_dir, f"{name}.part{i}.npz"), "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
            for key, a in g.items():
                buf = io.BytesIO()
                np.lib.format.write_array(buf, a, allow_pickle=False)
                info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
                info.compress_type = zipfile.ZIP_DEFLATED
                z.writestr(info, buf.getvalue(), compresslevel=9)


def operands(model, queries, items):
    """what the reference's forward feeds its logits / gating, from the same submodule calls"""
    qc = model.get_query_component_embeddings(queries)[0]
    xc = model.get_item_component_embeddings(items)[0].squeeze(0)
    gq = model._gating_fn._query_only_partial_module(queries)
    gi = model._gating_fn._item_only_partial_module(items).squeeze(0)
    return qc, xc, gq, gi


def eval_fp64(model, qc, xc, gq, gi):
    """fp64 evaluation of given operands with the reference's own qi module (cast to double) and combiner"""
    g = model._gating_fn
    L = g._num_logits
    logits = torch.einsum("bnd,xmd->bxnm", qc.double(), xc.double()).reshape(qc.size(0), xc.size(0), L) / model._temperature
    t = copy.deepcopy(g._qi_partial_module).double()(logits)
    gates = gq.double().unsqueeze(1) * gi.double().unsqueeze(0) + t
    arg = gates if g._combination_type == "glu_silu" else F.layer_norm(gates, normalized_shape=[L])
    return g._normalization_fn(gates * torch.sigmoid(arg), logits)[0]


def make_case(case, seed, out_dir):
    pq, px, dp, h, comb, B, X = case
    name = case_name(*case)
    torch.manual_seed(seed)
    model, debug_str = create_mol_interaction_module(**factory_kwargs(pq, px, dp, h, comb))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for key, p in model.named_parameters():
            if key.endswith("bias") or key.endswith("_b"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
    model.eval()
    queries = torch.randn((B, QUERY_DIM), generator=g)
    items = torch.randn((1, X, ITEM_DIM), generator=g)
    item_ids = (torch.randperm(4 * X + 11, generator=g)[:X] + 1).to(torch.int64).unsqueeze(0)

    # ---- module level, fp64
    m64 = copy.deepcopy(model).double()
    q64 = queries.double().requires_grad_(True)
    m64.train()
    s_train, aux = m64(q64, items.double())
    (grad64,) = torch.autograd.grad(s_train.sum(), q64)
    m64.eval()
    with torch.no_grad():
        s64_module = m64(queries.double(), items.double())[0]
        assert torch.equal(s_train.detach(), s64_module)            # every dropout rate is 0
        check = eval_fp64(m64, *operands(m64, queries.double(), items.double()))
        assert (check - s64_module).abs().max().item() <= 1e-12, name
        # the reference's own brute-force top-k runs on these inputs (not stored: ties and order are the test's to judge)
        MoLBruteForceTopK(model, items, item_ids)(queries, k=min(X, 10))
    sd = model.state_dict()
    module = {"queries": queries.numpy(), "items": items.numpy(), "item_ids": item_ids.numpy(), "s64": s64_module.numpy(),
              "mi_loss": aux["mi_loss"].detach().numpy(), "grad_queries": grad64.numpy(),
              "state_dict_keys": np.array(list(sd.keys())), "debug_str": np.array(debug_str)}
    module.update({f"sd:{k}": v.numpy() for k, v in sd.items()})
    write_parts(out_dir, f"{name}.module", module)

    # ---- op level, per dtype
    report = {}
    for dname, dt in DTYPES.items():
        mt = copy.deepcopy(model).to(dt)
        with torch.no_grad():
            qt, it = queries.to(dt), items.to(dt)
            qc, xc, gq, gi = operands(mt, qt, it)
            ref = mt(qt, it)[0]
            s64 = eval_fp64(mt, qc, xc, gq, gi)
        assert ref.dtype == dt and qc.dtype == dt and xc.dtype == dt and gq.dtype == dt and gi.dtype == dt
        e_ref = (ref.double() - s64).abs().max().item()
        smax = s64.abs().max().item()
        if dname == "float32":
            assert 16 * e_ref < 1e-3 * smax, (name, e_ref, smax)
        else:
            assert e_ref < 0.1 * smax, (name, dname, e_ref, smax)
        qi = mt._gating_fn._qi_partial_module
        lin = [m for m in qi if isinstance(m, torch.nn.Linear)]
        arrays = {"qc": to_numpy(qc), "gq": to_numpy(gq), "w1": to_numpy(lin[0].weight)}
        if h > 0:
            arrays.update({"b1": to_numpy(lin[0].bias), "w2": to_numpy(lin[1].weight), "b2": to_numpy(lin[1].bias)})
        else:
            arrays["b2"] = to_numpy(lin[0].bias)
        arrays.update({"e_ref": np.float64(e_ref), "ref": to_numpy(ref), "gi": to_numpy(gi), "s64": s64.numpy(), "xc": to_numpy(xc)})
        write_parts(out_dir, f"{name}.{dname}", arrays)
        report[dname] = (e_ref, smax)
    return name, report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(1)             # one accumulation order, whatever the machine
    for i, case in enumerate(CASES):
        name, report = make_case(case, seed=31000 + 10 * i, out_dir=args.out)
        print(name, "  ".join(f"{d}: e_ref {e:.3g} max|s| {s:.3g}" for d, (e, s) in report.items()))


if __name__ == "__main__":
    main()
