"""fp64 restatement of the in-backward row-wise Adagrad (TorchRec RowWiseAdagrad / fbgemm exact row-wise Adagrad with
weight_decay = 0, lr_decay = 0) and the per-element bounds the GPU tests hold the kernel to.

For every row r among idx, and only those:  G[r] = sum of dout rows with idx == r;  momentum1[r] += mean_d(G[r, d]^2);
W[r] -= lr / (sqrt(momentum1[r]) + eps) * G[r].

The bounds are first-order bounds of an fp32 evaluation in ANY summation order, constants doubled.  Per row: m duplicates,
A = sum_i |dout_i| (per column), u = 2^-24, c = lr / (sqrt(momentum1_ref) + eps):
    |W - W_ref|                 <= c (2m + 16) u A + 8u (|W_old| + c |G_ref|)
    |momentum1 - momentum1_ref| <= mean_d(2 m u A |G_ref| + 4u G_ref^2) + (log2(dim) + 2) u mean_d(G_ref^2) + 2u momentum1_ref
"""

import numpy as np

U = 2.0 ** -24


def rowwise_adagrad_ref(weight, momentum1, idx, dout, lr, eps=1e-8):
    """-> dict(weight, momentum1: the updated fp64 arrays (full size), rows: the sorted unique ids, tol_weight (len(rows), dim),
    tol_momentum1 (len(rows))).  Inputs are taken as the exact values they hold (16-bit dout is widened, not re-rounded)."""
    w = np.array(weight, dtype=np.float64)
    m1 = np.array(momentum1, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    g = np.asarray(dout, dtype=np.float64)
    dim = w.shape[1]
    rows, inverse, counts = np.unique(idx, return_inverse=True, return_counts=True)
    G = np.zeros((len(rows), dim))
    A = np.zeros((len(rows), dim))
    np.add.at(G, inverse, g)
    np.add.at(A, inverse, np.abs(g))
    w_old = w[rows].copy()
    m_new = m1[rows] + (G * G).mean(axis=1)
    c = lr / (np.sqrt(m_new) + eps)
    w[rows] = w_old - c[:, None] * G
    m1[rows] = m_new
    m = counts.astype(np.float64)[:, None]
    tol_w = c[:, None] * (2 * m + 16) * U * A + 8 * U * (np.abs(w_old) + c[:, None] * np.abs(G))
    tol_m = ((2 * m * U * A * np.abs(G) + 4 * U * G * G).mean(axis=1) + (np.log2(dim) + 2) * U * (G * G).mean(axis=1)
             + 2 * U * m_new)
    return dict(weight=w, momentum1=m1, rows=rows, tol_weight=tol_w, tol_momentum1=tol_m)
