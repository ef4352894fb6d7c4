"""Loader of the Mixture-of-Logits fixtures (tests/golden/mol, minted by make_mol_golden.py) for test_mol_host.py and
test_mol_gpu.py: the case table, the part files put back together, 16-bit arrays back in their dtype."""

import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mol")
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
TEMPERATURE = 0.05
QUERY_DIM, ITEM_DIM = 24, 20

# (P_Q, P_X, D_P, H, combination, B, X): make_mol_golden.py's table
CASES = [
    (1, 1, 8, 0, "glu_silu", 1, 1),
    (4, 2, 16, 16, "glu_silu", 5, 70),
    (3, 5, 10, 100, "glu_silu_ln", 65, 257),
    (8, 8, 32, 128, "glu_silu", 33, 1000),
    (8, 8, 64, 0, "glu_silu_ln", 17, 513),
]
OPERANDS = ("qc", "xc", "gq", "gi", "w1", "b1", "w2", "b2")


def case_name(pq, px, dp, h, comb, B, X):
    return f"mol_{pq}x{px}x{dp}_h{h}_{comb}_b{B}_x{X}"


def case_id(case):
    return case_name(*case)


def factory_kwargs(pq, px, dp, h, comb):
    return dict(query_embedding_dim=QUERY_DIM, item_embedding_dim=ITEM_DIM, dot_product_dimension=dp, query_dot_product_groups=pq,
                item_dot_product_groups=px, temperature=TEMPERATURE, query_dropout_rate=0.0, query_hidden_dim=32,
                item_dropout_rate=0.0, item_hidden_dim=32, gating_query_hidden_dim=16, gating_qi_hidden_dim=h,
                gating_item_hidden_dim=16, softmax_dropout_rate=0.0, bf16_training=False, gating_combination_type=comb)


_CACHE = {}


def load_group(case, group):
    """the arrays of ``<case>.<group>.part*.npz`` by name; pieces ``key@i`` concatenated along their first axis"""
    key = (case_name(*case), group)
    if key not in _CACHE:
        paths = sorted(glob.glob(os.path.join(GOLDEN, f"{key[0]}.{group}.part*.npz")))
        assert paths, f"no fixture {key[0]}.{group}"
        raw = {}
        for p in paths:
            with np.load(p, allow_pickle=False) as z:
                raw.update({k: z[k] for k in z.files})
        out, cut = {}, {}
        for k, a in raw.items():
            if "@" in k:
                name, i = k.rsplit("@", 1)
                cut.setdefault(name, {})[int(i)] = a
            else:
                out[k] = a
        for name, pieces in cut.items():
            out[name] = np.concatenate([pieces[i] for i in range(len(pieces))], axis=0)
        _CACHE[key] = out
    return _CACHE[key]


def load_operands(case, dtype_name):
    """(operands as torch tensors of that dtype, on the CPU; None for an absent b1 / w2), ref, s64, e_ref"""
    g = load_group(case, dtype_name)
    dt = DTYPES[dtype_name]

    def tensor(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.view(dt) if dt != torch.float32 else t

    ops = {k: (tensor(g[k]) if k in g else None) for k in OPERANDS}
    return ops, tensor(g["ref"]), torch.from_numpy(g["s64"]), float(g["e_ref"])


def load_module_fixture(case):
    g = load_group(case, "module")
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd:")}
    return g, {k: sd[k] for k in [str(x) for x in g["state_dict_keys"]]}
