"""Helper of the SASRec tests: fixture loaders, an fp64 restatement of the jagged causal softmax attention and its gradients,
the padded math path of ``torch.nn.MultiheadAttention`` (``need_weights=True``) in any dtype on the CPU, and the gate.

The restatement (``restate``) works per user and per head with keys j <= i of the same user only, in numpy fp64, with the
gradients written out by hand:
    S = scale q k^T,  P = softmax_j(S),  Pd = P keep ks,  O = Pd V,
    dV = Pd^T dO,  dP = (dO V^T) keep ks,  delta = rowsum(P dP) (= rowsum(dO O)),  dS = P (dP - delta),
    dQ = scale dS K,  dK = scale dS^T Q.
``keep`` is the oracle's mask, ``oracle.hstu_oracle.dropout_keep_mask(seed, L H, N, p)`` reshaped to (L, H, N): element
[r, h, j] belongs to global query row r, head h and the key at position j of r's user.  Its ``wrong`` switches restate the
obvious wrong kernels (tests/test_sasrec_host.py shows that the fixtures catch each).

``math_path`` is what the fixtures' op cases were minted with and what gives ``e_ref`` for inputs drawn inside a test: q
scaled, ``baddbmm`` onto a -inf causal mask, ``softmax``, (dropout as a multiplication with keep ks,) ``bmm``, on the padded
batch in the given dtype, gradients by autograd.  It reads nothing of the reference.

The gate: ``e_hip <= m e_ref`` per tensor over the whole batch, both relative Frobenius errors against the fp64 truth,
``m = multitask_ref.gate_multiplier(dtype, n)``: the project's 1.5 for 16-bit and 8 for fp32 I/O.  Whole-batch tensors only:
for a user of one row the true dq and dk are zero and the kernel's dP - delta is the difference of two fp32 sums taken in
different orders, so a per-user relative error is meaningless there.
"""

import glob
import os

import numpy as np
import torch

from multitask_ref import gate_multiplier

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sasrec")
TAGS = ("f64", "f32", "bf16")
TORCH_DTYPE = {"f64": torch.float64, "f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTYPE_NAME = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}
GRADS = ("out", "dq", "dk", "dv")


# ------------------------------------------------------------------------------------------------------------------ storage
def to_bits(t: torch.Tensor) -> np.ndarray:
    """bf16 bit patterns (uint16) of a tensor whose values are bf16-representable"""
    b = t.detach().to(torch.bfloat16)
    assert torch.equal(b.to(t.dtype), t.detach()), "value not representable in bf16"
    return b.view(torch.int16).numpy().view(np.uint16).copy()


def from_bits(a: np.ndarray) -> np.ndarray:
    """uint16 bf16 bit patterns -> float64"""
    return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _merge(prefix):
    out = {}
    files = sorted(glob.glob(os.path.join(FIXTURES, prefix + "__*.npz")))
    assert files, prefix
    for f in files:
        with np.load(f) as z:
            for k in z.files:
                out[k] = z[k]
    return out


def op_case_names():
    return sorted({os.path.basename(f).split("__")[0] for f in glob.glob(os.path.join(FIXTURES, "op_*__*.npz"))})


def model_case_names():
    return sorted({os.path.basename(f).split("__")[0] for f in glob.glob(os.path.join(FIXTURES, "model_*__*.npz"))})


def load_op_case(name):
    """inputs as float64 (bf16-exact values): q, k, v, dout (L, H, d); lengths; max_seq_len; results '<tag>:<name>' float64"""
    z = _merge(name)
    c = {"name": name, "lengths": z["lengths"].astype(np.int64), "max_seq_len": int(z["max_seq_len"])}
    for k in ("q", "k", "v", "dout"):
        c[k] = from_bits(z[k])
    for tag in TAGS:
        for g in GRADS:
            a = z[f"{tag}:{g}"]
            c[f"{tag}:{g}"] = from_bits(a) if a.dtype == np.uint16 else a.astype(np.float64)
    return c


def load_model_case(name):
    z = _merge(name)
    c = {"name": name}
    for k, a in z.items():
        c[k] = from_bits(a) if a.dtype == np.uint16 else a
    return c


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])


# -------------------------------------------------------------------------------------------------------------- restatement
def restate(q, k, v, dout, lengths, scale=None, keep=None, keep_scale=1.0, wrong=None):
    """fp64 truth: dict(out, dq, dk, dv), each (L, H, d).  ``wrong``: None | 'no_causal' | 'ignore_offsets' |
    'lse_after_dropout' (the normaliser sums the kept keys only)."""
    q, k, v, dout = (np.asarray(t, dtype=np.float64) for t in (q, k, v, dout))
    L, H, d = q.shape
    scale = float(d) ** -0.5 if scale is None else float(scale)
    offs = offsets_of(lengths)
    if wrong == "ignore_offsets":
        offs = np.array([0, L])
    res = {g: np.zeros_like(q) for g in GRADS}
    for b in range(len(offs) - 1):
        s0, s1 = int(offs[b]), int(offs[b + 1])
        n = s1 - s0
        if n == 0:
            continue
        vis = np.ones((n, n), dtype=bool) if wrong == "no_causal" else np.tril(np.ones((n, n), dtype=bool))
        for h in range(H):
            qb, kb, vb, gb = q[s0:s1, h], k[s0:s1, h], v[s0:s1, h], dout[s0:s1, h]
            s = np.where(vis, scale * (qb @ kb.T), -np.inf)
            e = np.exp(s - s.max(axis=1, keepdims=True))
            kf = np.ones((n, n)) if keep is None else np.where(keep[s0:s1, h, :n], keep_scale, 0.0)
            if wrong == "lse_after_dropout":
                den = (e * (kf != 0)).sum(axis=1, keepdims=True)
                p = e / np.where(den == 0, 1.0, den)
            else:
                p = e / e.sum(axis=1, keepdims=True)
            pd = p * kf
            res["out"][s0:s1, h] = pd @ vb
            res["dv"][s0:s1, h] = pd.T @ gb
            dp = (gb @ vb.T) * kf
            ds = p * (dp - (p * dp).sum(axis=1, keepdims=True))
            res["dq"][s0:s1, h] = scale * (ds @ kb)
            res["dk"][s0:s1, h] = scale * (ds.T @ qb)
    return res


def lse_of(q, k, lengths, scale=None):
    """(L, H) fp64: ln sum_j exp(scale q_i k_j) over the visible keys"""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    L, H, d = q.shape
    scale = float(d) ** -0.5 if scale is None else float(scale)
    offs = offsets_of(lengths)
    out = np.zeros((L, H))
    for b in range(len(offs) - 1):
        s0, s1 = int(offs[b]), int(offs[b + 1])
        n = s1 - s0
        for h in range(H if n else 0):
            s = np.where(np.tril(np.ones((n, n), dtype=bool)), scale * (q[s0:s1, h] @ k[s0:s1, h].T), -np.inf)
            m = s.max(axis=1)
            out[s0:s1, h] = m + np.log(np.exp(s - m[:, None]).sum(axis=1))
    return out


# ---------------------------------------------------------------------------------------------------------------- math path
def _pad(x, lengths, n):
    """(L, H, d) -> (B H, n, d), zero padded"""
    L, H, d = x.shape
    B = len(lengths)
    out = x.new_zeros((B, n, H, d))
    offs = offsets_of(lengths)
    for b in range(B):
        out[b, : int(lengths[b])] = x[int(offs[b]): int(offs[b + 1])]
    return out.permute(0, 2, 1, 3).reshape(B * H, n, d)


def _unpad(x, lengths, H):
    """(B H, n, d) -> (L, H, d)"""
    B = len(lengths)
    x = x.reshape(B, H, x.shape[1], x.shape[2]).permute(0, 2, 1, 3)
    return torch.cat([x[b, : int(lengths[b])] for b in range(B)], dim=0) if B else x.reshape(0, H, x.shape[-1])


def math_path(q, k, v, dout, lengths, max_seq_len, dtype, scale=None, keep=None, keep_scale=1.0):
    """dict(out, dq, dk, dv) as float64 (L, H, d): torch's math path in ``dtype`` on the padded batch, gradients by autograd.
    q, k, v, dout: float64 arrays whose values are representable in ``dtype``."""
    n = int(max_seq_len)
    lengths = [int(x) for x in lengths]
    L, H, d = q.shape
    scale = float(d) ** -0.5 if scale is None else float(scale)
    leaves = [torch.from_numpy(np.ascontiguousarray(t)).to(dtype).requires_grad_(True) for t in (q, k, v)]
    qp, kp, vp = (_pad(t, lengths, n) for t in leaves)
    mask = torch.zeros((n, n), dtype=dtype).masked_fill_(torch.triu(torch.ones((n, n), dtype=torch.bool), diagonal=1), float("-inf"))
    w = torch.softmax(torch.baddbmm(mask, qp * scale, kp.transpose(-2, -1)), dim=-1)
    if keep is not None:
        kf = torch.zeros((len(lengths), H, n, n), dtype=dtype)
        offs = offsets_of(lengths)
        kt = torch.from_numpy(np.ascontiguousarray(keep))
        for b, ln in enumerate(lengths):
            kf[b, :, :ln, :] = (kt[int(offs[b]): int(offs[b]) + ln].permute(1, 0, 2)[:, :, :n]).to(dtype) * keep_scale
        w = w * kf.reshape(len(lengths) * H, n, n)
    out = _unpad(torch.bmm(w, vp), lengths, H)
    out.backward(torch.from_numpy(np.ascontiguousarray(dout)).to(dtype))
    res = {"out": out.detach()}
    res.update({g: t.grad for g, t in zip(("dq", "dk", "dv"), leaves)})
    return {g: t.double().numpy() for g, t in res.items()}


# --------------------------------------------------------------------------------------------------------------------- gate
def rel_fro(a, truth):
    a, truth = np.asarray(a, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    den = np.linalg.norm(truth.ravel())
    return float(np.linalg.norm((a - truth).ravel()) / den) if den > 0 else float(np.linalg.norm(a.ravel()))


def gate(what, got, ref, truth, dtype_name, names=GRADS, multiplier=None):
    """prints e_hip / e_ref of every tensor and returns the list of tensors that miss e_hip <= m e_ref; ``multiplier(tensor,
    n_elements)`` replaces ``gate_multiplier`` (the model cases: ``model_multiplier``)"""
    bad = []
    for g in names:
        e_hip, e_ref = rel_fro(got[g], truth[g]), rel_fro(ref[g], truth[g])
        n_el = np.asarray(truth[g]).size
        m = gate_multiplier(dtype_name, n_el) if multiplier is None else multiplier(g, n_el)
        ratio = e_hip / e_ref if e_ref > 0 else float("inf") if e_hip > 0 else 0.0
        print(f"gate {what} {dtype_name} {g}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {ratio:.3f} (m = {m})")
        if not e_hip <= m * e_ref:
            bad.append((g, e_hip, e_ref))
    return bad


def model_multiplier(dtype_name, tensor, n_elements, relu_flips):
    """The gate's multiplier for one tensor of a MODEL case: ``gate_multiplier``, except for 16-bit gradients behind a ReLU.

    A ReLU unit whose pre-activation lies within the 16-bit error of zero is open in a 16-bit run and closed in the truth,
    or the other way round.  That is not a rounding of the size of an ulp: the unit's whole contribution to every gradient
    that passes through it appears or vanishes.  In the relu fixture the reference's OWN bf16 run flips 36 of its 20,000
    units, and those few events ARE its gradient error: 4 to 5 % against 0.5 to 0.8 % in the gelu fixture, which has no
    such events (the forward output is continuous in a flip -- the unit's value is next to zero there -- and keeps 0.5 %).
    Which units flip depends on every rounding in front of them, and the kernel does not round where the reference does (it
    scales q in fp32 and rounds the un-normalised P), so the two sides do not share their events.  Both errors are then norms
    of K independent outcomes, K small, and, as for the few-number tensors of ``gate_multiplier``, e_hip / e_ref is the ratio
    of two independent chi(K) variables, sqrt(F(K, K)), even when the two sides are equally accurate.  The multiplier is its
    99 % point, never below the plain one: 1.5 is reached from K = 34 on; K = 18 gives 1.76.
    K is counted on the reference alone (``bf16:relu_flips``, per block, minted with the fixture: the units whose gate
    differs between its bf16 and its fp64 run) for the blocks a gradient passes through: block i's own ReLU and every later
    one for the tensors in front of block i's ReLU (the attention and the first convolution of block i, the embeddings),
    the later blocks only for block i's second convolution.  Unequal contributions make the effective K smaller, never
    larger, so the bound is not generous.  fp32, the output, gelu and tensors that no flip reaches keep the plain multiplier."""
    m = gate_multiplier(dtype_name, n_elements)
    if dtype_name == "float32" or not tensor.startswith("g:") or not int(np.sum(relu_flips)):
        return m
    if tensor == "g:emb":
        first = 0
    else:
        block = int(tensor.split(".")[1])
        first = block + 1 if "_conv1d.3" in tensor else block
    k = int(np.sum(relu_flips[first:]))
    if k == 0:
        return m
    return max(m, ratio_q99(k))


def ratio_q99(k):
    """99 % point of sqrt(F(k, k)), the ratio of two independent chi(k) variables: with X = a / (a + b) ~ Beta(k/2, k/2) the
    ratio exceeds r exactly when X exceeds r^2 / (1 + r^2); the Beta distribution function by the trapezoid rule on 2^18
    points (numpy only), the quantile by bisection"""
    x = np.linspace(0.0, 1.0, (1 << 18) + 1)[1:-1]
    logpdf = (k / 2.0 - 1.0) * (np.log(x) + np.log1p(-x))
    pdf = np.exp(logpdf - logpdf.max())
    cdf = np.cumsum(pdf)
    cdf /= cdf[-1]
    xq = float(x[np.searchsorted(cdf, 0.99)])
    return float(np.sqrt(xq / (1.0 - xq)))


def round_to(x, dtype):
    """float64 array rounded to the values of ``dtype``"""
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).double().numpy()


def keep_mask(seed, rows, heads, max_seq_len, p):
    """the oracle's mask as (L, H, N) bool and the survivor scale"""
    from oracle.hstu_oracle import dropout_keep_mask

    keep, ks = dropout_keep_mask(seed, rows * heads, max_seq_len, p)
    return keep.reshape(rows, heads, max_seq_len), ks
