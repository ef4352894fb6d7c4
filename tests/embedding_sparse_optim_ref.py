"""fp64 restatement of the in-backward sparse SGD and sparse Adam (csrc/embedding_optim.hip), restricted to the touched rows,
and the per-element bounds the GPU tests hold the kernels to.

For every row r among idx, and only those, G[r] = sum of the dout rows with idx == r and

    SGD:   W[r] -= lr G[r]
    Adam:  m[r] = b1 m[r] + (1 - b1) G[r];  v[r] = b2 v[r] + (1 - b2) G[r]^2;  t = step + 1, bc1 = 1 - b1^t, bc2 = 1 - b2^t
           W[r] -= (lr / bc1) m[r] / (sqrt(v[r]) / sqrt(bc2) + eps)

which is torch.optim.Adam (amsgrad off, weight_decay 0) on the touched rows: rows outside the batch do not decay.

The bounds are first-order bounds of an fp32 evaluation in ANY summation order.  Per row: k duplicates, A = sum_i |dout_i| per
column, u = 2^-24, a = lr / bc1, den = sqrt(v_ref) / sqrt(bc2) + eps:

    tG  = 2k u A
    tm  = (1 - b1) tG + 4u (b1 |m_old| + (1 - b1) |G|)
    tv  = (1 - b2) (2 |G| tG + tG^2) + 6u (b2 v_old + (1 - b2) G^2)
    tsq = min(tv / sqrt(v_ref), sqrt(tv))            (sqrt(tv) where v_ref = 0)
    tden = tsq / sqrt(bc2) + 4u den
    tW(Adam) = a (tm / den + |m_ref| tden / den^2) + 8u (|W_old| + |upd|)
    tW(SGD)  = lr (2k + 4) u A + 4u (|W_old| + lr |G|)

Inputs are taken as the exact values they hold: 16-bit dout is widened, not re-rounded, and lr, betas and eps are the numbers
the caller passes -- the kernels take them as fp32, so a test passes fp32-representable values (``f32``) to both sides."""

import numpy as np

U = 2.0 ** -24


def f32(x):
    """the fp32 value nearest to x, as a Python float: what an entry point that takes a `float` computes with"""
    return float(np.float32(x))


def _segments(weight, idx, dout):
    w = np.array(weight, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    g = np.asarray(dout, dtype=np.float64)
    rows, inverse, counts = np.unique(idx, return_inverse=True, return_counts=True)
    G = np.zeros((len(rows), w.shape[1]))
    A = np.zeros((len(rows), w.shape[1]))
    np.add.at(G, inverse, g)
    np.add.at(A, inverse, np.abs(g))
    return w, rows, G, A, counts.astype(np.float64)[:, None]


def sparse_sgd_ref(weight, idx, dout, lr):
    """-> dict(weight: the updated fp64 array (full size), rows: the sorted unique ids, tol_weight (len(rows), dim))"""
    w, rows, G, A, k = _segments(weight, idx, dout)
    w_old = w[rows].copy()
    w[rows] = w_old - lr * G
    tol_w = lr * (2 * k + 4) * U * A + 4 * U * (np.abs(w_old) + lr * np.abs(G))
    return dict(weight=w, rows=rows, tol_weight=tol_w)


def sparse_adam_ref(weight, exp_avg, exp_avg_sq, idx, dout, lr, betas, eps, step, variant="adam"):
    """-> dict(weight, exp_avg, exp_avg_sq: the updated fp64 arrays (full size), rows, tol_weight, tol_exp_avg, tol_exp_avg_sq
    (len(rows), dim) each).  ``step``: the updates applied before this one (t = step + 1).  ``variant`` other than "adam" gives
    the WRONG forms the bounds must reject: "no_bias_correction", "sparse_adam_eps" (torch.optim.SparseAdam: sqrt(v) + eps, with
    sqrt(bc2) in the step size), "eps_under_sqrt" (sqrt(v / bc2 + eps))."""
    w, rows, G, A, k = _segments(weight, idx, dout)
    m = np.array(exp_avg, dtype=np.float64)
    v = np.array(exp_avg_sq, dtype=np.float64)
    b1, b2 = (float(b) for b in betas)
    t = int(step) + 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    w_old, m_old, v_old = w[rows].copy(), m[rows].copy(), v[rows].copy()
    m_new = b1 * m_old + (1 - b1) * G
    v_new = b2 * v_old + (1 - b2) * G * G
    a = lr / bc1
    den = np.sqrt(v_new) / np.sqrt(bc2) + eps
    if variant == "adam":
        upd = a * m_new / den
    elif variant == "no_bias_correction":
        upd = lr * m_new / (np.sqrt(v_new) + eps)
    elif variant == "sparse_adam_eps":
        upd = lr * np.sqrt(bc2) / bc1 * m_new / (np.sqrt(v_new) + eps)
    elif variant == "eps_under_sqrt":
        upd = a * m_new / np.sqrt(v_new / bc2 + eps)
    else:
        raise ValueError(variant)
    w[rows] = w_old - upd
    m[rows] = m_new
    v[rows] = v_new
    tG = 2 * k * U * A
    tm = (1 - b1) * tG + 4 * U * (b1 * np.abs(m_old) + (1 - b1) * np.abs(G))
    tv = (1 - b2) * (2 * np.abs(G) * tG + tG * tG) + 6 * U * (b2 * v_old + (1 - b2) * G * G)
    root = np.sqrt(v_new)
    with np.errstate(divide="ignore", invalid="ignore"):
        tsq = np.where(root > 0, np.minimum(tv / root, np.sqrt(tv)), np.sqrt(tv))
    tden = tsq / np.sqrt(bc2) + 4 * U * den
    true_upd = a * m_new / den
    tW = a * (tm / den + np.abs(m_new) * tden / (den * den)) + 8 * U * (np.abs(w_old) + np.abs(true_upd))
    return dict(weight=w, exp_avg=m, exp_avg_sq=v, rows=rows, tol_weight=tW, tol_exp_avg=tm, tol_exp_avg_sq=tv)


def worst(err, tol):
    """largest error over its bound; a bound of exactly 0 admits only an error of 0 (inf otherwise)"""
    err, tol = np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    if ((tol == 0) & (err != 0)).any():
        return float("inf")
    live = tol > 0
    return float((err[live] / tol[live]).max()) if live.any() else 0.0


def within(err, tol):
    return bool((np.asarray(err) <= np.asarray(tol)).all())


# ---- what the GPU tests and the host tests share: ids, state with sentinels, and the cases
def make_ids(kind, n, rows, rng):
    """n ids in [0, rows); except when all are equal, id 0 and id rows - 1 occur whenever there is room for both (the id
    distributions of test_embedding_optim_gpu.py, on numpy's generator)"""
    if kind == "equal":
        return np.full(n, rows - 1, dtype=np.int64)
    if kind == "distinct":
        assert 2 <= n <= rows
        inner = 1 + rng.permutation(rows - 2)[:n - 2]
        return rng.permutation(np.concatenate([[0, rows - 1], inner]).astype(np.int64))
    p = 1.0 / np.arange(1, rows + 1, dtype=np.float64)
    idx = rng.permutation(rows)[rng.choice(rows, size=n, p=p / p.sum())].astype(np.int64)
    idx[0], idx[-1] = 0, rows - 1
    return idx


def make_state(rows, dim, rng, zero_state=False):
    """random fp32 table, random exp_avg, exp_avg_sq >= 0 (zeros on request), and a NaN-free sentinel pattern on every other row"""
    w = rng.standard_normal((rows, dim)).astype(np.float32)
    m = (rng.standard_normal((rows, dim)) * 0.1).astype(np.float32)
    v = (rng.random((rows, dim)) * 0.01).astype(np.float32)
    if zero_state:
        m[:], v[:] = 0, 0
    w[1::2], m[1::2], v[1::2] = -12345.671875, 321.125, 6789.0625
    return w, m, v


def make_problem(n, dim, rows, kind, tag, zero_state=False):
    """-> (idx, dout, w, m, v): the ids, the gradient rows as fp32 values that ``tag`` ("bf16" / "f16" / "f32") holds exactly, and
    make_state's table; a function of the arguments alone, so the host and the GPU tests see the same problem"""
    import torch

    rng = np.random.default_rng(n * 1000 + dim)
    idx = make_ids(kind, n, rows, rng)
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[tag]
    dout = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32)).to(dt).float().numpy()
    return (idx, dout) + make_state(rows, dim, rng, zero_state)


# (n, dim, table_rows, id distribution): the geometry classes of test_embedding_optim_gpu.py
SHAPES = [(1, 8, 1, "equal"), (63, 64, 8192, "distinct"), (64, 192, 8193, "distinct"), (65, 64, 100_003, "zipf"),
          (257, 8, 2, "zipf"), (257, 64, 8193, "equal"), (257, 192, 8192, "zipf"), (257, 256, 8193, "distinct"),
          (64, 256, 1, "equal"), (65, 64, 2, "zipf")]
CASES = [(n, d, r, k, t) for (n, d, r, k) in SHAPES for t in ("bf16", "f16", "f32")] + [
    (257, 1024, 8193, "zipf", "f32"), (257, 2048, 2, "zipf", "f16"),          # the row-width limits
    (257, 512, 2, "zipf", "f32"), (257, 520, 2, "zipf", "bf16"),              # the last dim with 32-row chunks, the first with 128
    # the chunk-size switch, with two runs of ~131,000 rows through the combine kernel
    (262_143, 8, 8193, "zipf", "bf16"), (262_144, 8, 8193, "zipf", "bf16"),
    # row classes no case above reaches with a cut segment (3 ids, n = 2 * 128 + 1: one id's run crosses both chunk boundaries):
    # four pieces of fp32 at their smallest dim, eight pieces (fp32 rows above 4 KiB, the coalesced lists), and the narrowest
    # fp32 row in 128-row chunks
    (257, 516, 3, "zipf", "f32"), (257, 1028, 3, "zipf", "f32"), (262_144, 4, 3, "zipf", "f32")]
# the two cases that pin where eps sits (eps = 1e-2): (n, dim, rows, kind, zero state, step)
EPS_CASES = [(65, 256, 1003, "zipf", False, 2), (64, 192, 8193, "distinct", True, 0)]
