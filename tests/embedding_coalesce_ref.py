"""fp64 restatement of the row-gradient coalesce (one fp32 row per distinct id of a batch) and of the replicated row-wise
Adagrad step built on it, with the bounds the GPU tests hold the kernels to.  Next to embedding_optim_ref.py, whose
convention the bounds follow: first-order bounds of an fp32 evaluation in ANY summation order, constants doubled, u = 2^-24.

Coalesce, per distinct id with m duplicates, G_ref = scale * sum_i dout_i and A = sum_i |dout_i| (per column):
    |G - G_ref| <= |scale| 2 m u A + 4u |G_ref|
(the sum of m terms: (m - 1) u A first order, doubled and rounded up; the scale's own rounding to fp32 and the one multiply:
2u |G_ref| first order, doubled).

Replicated step over W ranks that average: the formula of embedding_optim_ref.py on the concatenated batch with dout / W
taken in fp64, its bounds with every duplicate count raised by 2 -- one rounding for the scale, one for the extra level of
summation (a row's W partial sums are added again).  Derived, not measured."""

import numpy as np

import embedding_optim_ref as ER

U = ER.U


def _segments(idx, dout):
    """rows (sorted unique ids), their duplicate counts, and the fp64 sums of dout and |dout| per id"""
    idx = np.asarray(idx, dtype=np.int64)
    g = np.asarray(dout, dtype=np.float64)
    if idx.size == 0:
        z = np.zeros((0, g.shape[1]))
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), z, z
    order = np.argsort(idx, kind="stable")
    rows, starts, counts = np.unique(idx[order], return_index=True, return_counts=True)
    g = g[order]
    return rows, counts, np.add.reduceat(g, starts, axis=0), np.add.reduceat(np.abs(g), starts, axis=0)


def coalesce_ref(idx, dout, scale=1.0):
    """-> dict(rows, G (len(rows), dim) fp64, tol (the same shape), counts).  dout is taken as the exact values it holds."""
    rows, counts, S, A = _segments(idx, dout)
    G = float(scale) * S
    tol = abs(float(scale)) * 2 * counts[:, None] * U * A + 4 * U * np.abs(G)
    return dict(rows=rows, G=G, tol=tol, counts=counts)


def replicated_adagrad_ref(weight, momentum1, idx, dout, lr, eps, scale, extra=2):
    """The step every replica takes for the concatenated batch (idx, dout) of all ranks with gradients scaled by ``scale``
    (1 / world when averaging) in fp64: embedding_optim_ref.rowwise_adagrad_ref's result and bounds, the bounds with every
    duplicate count raised by ``extra``."""
    g = np.asarray(dout, dtype=np.float64) * float(scale)
    ref = ER.rowwise_adagrad_ref(weight, momentum1, idx, g, lr, eps)
    rows, _, G, A = _segments(idx, g)
    assert np.array_equal(rows, ref["rows"])
    c = lr / (np.sqrt(ref["momentum1"][rows]) + eps)
    ref["tol_weight"] = ref["tol_weight"] + c[:, None] * (2 * extra) * U * A
    ref["tol_momentum1"] = ref["tol_momentum1"] + (2 * extra * U * A * np.abs(G)).mean(axis=1)
    return ref
