"""fp64 restatement of jagged_dense_bmm_broadcast_add and its gradients (a per-user numpy loop over the four formulas)
plus the loader of the fixtures under tests/golden/jagged_bmm/.  Shared by the CPU and GPU tests of the op; no code under
test is involved."""

import glob
import os

import numpy as np

from conftest import GOLDEN

FIXTURES = os.path.join(GOLDEN, "jagged_bmm")
OP_TENSORS = ("out", "d_jagged", "d_dense", "d_bias")


def bmm_fp64(seq_offsets, jagged, dense, bias, d_out):
    """(out, d_jagged, d_dense, d_bias) in fp64: for user b with rows [s, e)
    out[s:e] = jagged[s:e] @ dense[b] + bias[b];  d_jagged[s:e] = d_out[s:e] @ dense[b]^T;
    d_dense[b] = jagged[s:e]^T @ d_out[s:e];  d_bias[b] = column sums of d_out[s:e]  (zeros for an empty user)"""
    off = np.asarray(seq_offsets).astype(np.int64)
    j, d, b, g = (np.asarray(t, dtype=np.float64) for t in (jagged, dense, bias, d_out))
    B, K, N = d.shape
    out, dj = np.zeros((j.shape[0], N)), np.zeros((j.shape[0], K))
    dd, db = np.zeros((B, K, N)), np.zeros((B, N))
    for u in range(B):
        s, e = int(off[u]), int(off[u + 1])
        out[s:e] = j[s:e] @ d[u] + b[u]
        dj[s:e] = g[s:e] @ d[u].T
        dd[u] = j[s:e].T @ g[s:e]
        db[u] = g[s:e].sum(0)
    return dict(out=out, d_jagged=dj, d_dense=dd, d_bias=db)


def rel_fro(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def _widen(a, dtype_name):
    """stored array -> float32 array holding the same values (bf16 is stored as its uint16 bit pattern)"""
    if dtype_name == "bfloat16" and a.dtype == np.uint16:
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32) if a.dtype.kind == "f" else a


def op_case_files():
    return sorted(glob.glob(os.path.join(FIXTURES, "op_*.npz")))


def load_op_case(path):
    z = np.load(path, allow_pickle=False)
    dtype_name = str(z["dtype"])
    case = {k: _widen(z[k], dtype_name) for k in z.files if k != "dtype"}
    case["dtype"] = dtype_name
    case["name"] = os.path.basename(path)[3:-4]
    return case


def load_module_case(kind):
    z = np.load(os.path.join(FIXTURES, f"module_{kind}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def gate_multiplier(dtype_name):
    """e_hip <= m * e_ref.  16-bit: both sides accumulate in fp32 and round once, so both sit on the output-rounding floor and
    differ by fp32 summation order only (m = 1.5).  fp32: e_ref is summation-order noise itself, and another order over up
    to a few hundred terms may legitimately be several times larger (m = 8)."""
    return 8.0 if dtype_name == "float32" else 1.5
