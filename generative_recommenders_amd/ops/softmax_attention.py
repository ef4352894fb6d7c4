"""Jagged causal softmax attention: the attention of the SASRec baseline
(generative_recommenders/research/modeling/sequential/sasrec.py:209-214, ``torch.nn.MultiheadAttention`` on a padded
(B, N, D) batch with an (N, N) mask) on jagged rows.  Row i of user b sees rows j <= i of user b:

    P = softmax_j(scale <q_i, k_j>),   O = dropout(P) V

``jagged_causal_softmax_attention`` runs the fused HIP kernels (csrc/softmax_attn.hip: no (N, N) object in memory, P
recomputed from a saved log-sum-exp in backward, the dropout mask regenerated from a seed) inside their range
(bf16 / fp16 / fp32, head dim <= 64, max_seq_len <= 512) and ``jagged_causal_softmax_attention_composed`` -- the same
function from this package's jagged <-> padded kernels and torch ops on the padded (B, H, N, N) scores -- outside it.
"""

from typing import Optional

import torch
import torch.nn.functional as F

from generative_recommenders_amd import _lib as L
from generative_recommenders_amd.ops import _launch
from generative_recommenders_amd.ops.hstu_attention import _pad_head_dim


class _SoftmaxAttnFunction(torch.autograd.Function):
    """saves q, k, v, out, lse and the seed; the backward recomputes P and regenerates the dropout mask"""

    @staticmethod
    def forward(ctx, max_seq_len, q, k, v, seq_offsets, scale, dropout_pr, seed):
        out, lse = _launch.softmax_attn_fwd(q, k, v, seq_offsets, max_seq_len, scale, dropout_pr, seed)
        ctx.save_for_backward(q, k, v, out, lse, seq_offsets)
        ctx.args = (max_seq_len, scale, dropout_pr, seed)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse, seq_offsets = ctx.saved_tensors
        max_seq_len, scale, dropout_pr, seed = ctx.args
        dq, dk, dv = _launch.softmax_attn_bwd(dout, q, k, v, out, lse, seq_offsets, max_seq_len, scale, dropout_pr, seed)
        return None, dq, dk, dv, None, None, None, None


def _check(max_seq_len, q, k, v, seq_offsets, dropout_pr):
    for name, t in (("q", q), ("k", k), ("v", v), ("seq_offsets", seq_offsets)):
        L.require_gpu_tensor(t, name)
    torch._assert(max_seq_len > 0, "max_seq_len must be larger than 0")
    torch._assert(q.dim() == 3 and q.shape == k.shape == v.shape, "q, k, v must be (L, H, d) with one head dim")
    torch._assert(0.0 <= dropout_pr < 1.0, "dropout_pr must be in [0, 1)")


def jagged_causal_softmax_attention(max_seq_len: int, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                    seq_offsets: torch.Tensor, scale: Optional[float] = None, dropout_pr: float = 0.0,
                                    training: bool = True, seed: Optional[int] = None) -> torch.Tensor:
    """q, k, v (L, H, d) -> (L, H, d).  ``scale=None``: d ** -0.5 with the REAL head dim d.  Dropout acts on P when
    ``training``; ``seed=None`` draws one from torch's CPU generator (``torch.manual_seed`` and
    ``torch.utils.checkpoint`` reproduce it).  Outside the fused range the composition runs."""
    _check(max_seq_len, q, k, v, seq_offsets, dropout_pr)
    d = q.shape[2]
    if not _launch.softmax_attn_supported(q.dtype, d, max_seq_len):
        return jagged_causal_softmax_attention_composed(max_seq_len, q, k, v, seq_offsets, scale, dropout_pr, training, seed)
    scale = float(d) ** -0.5 if scale is None else float(scale)
    p = float(dropout_pr) if training else 0.0
    if p > 0.0 and seed is None:
        from generative_recommenders_amd.ops.hstu_compute import draw_dropout_seed

        seed = draw_dropout_seed()
    out, _ = _SoftmaxAttnFunction.apply(int(max_seq_len), _pad_head_dim(q), _pad_head_dim(k), _pad_head_dim(v), seq_offsets,
                                        scale, p, int(seed) if p > 0.0 else 0)
    return out[..., :d] if out.shape[2] != d else out


def jagged_causal_softmax_attention_composed(max_seq_len: int, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                             seq_offsets: torch.Tensor, scale: Optional[float] = None,
                                             dropout_pr: float = 0.0, training: bool = True,
                                             seed: Optional[int] = None) -> torch.Tensor:
    """The same function on the padded batch, the way ``torch.nn.MultiheadAttention`` computes it with
    ``need_weights=True``: scaled q, scores added onto a -inf causal mask, softmax, dropout from torch's own stream
    (``seed`` is not used), P V.  The (B, H, N, N) scores exist in memory, forward and backward."""
    from generative_recommenders_amd.ops.jagged_tensors import dense_to_jagged, jagged_to_padded_dense

    _check(max_seq_len, q, k, v, seq_offsets, dropout_pr)
    del seed
    rows, H, d = q.shape
    n = int(max_seq_len)
    scale = float(d) ** -0.5 if scale is None else float(scale)
    B = seq_offsets.numel() - 1
    if rows == 0 or B == 0:
        return (q + k + v) * 0
    pad = lambda t: jagged_to_padded_dense(t.reshape(rows, H * d), seq_offsets, n).view(B, n, H, d).transpose(1, 2)
    qp, kp, vp = pad(q) * scale, pad(k), pad(v)
    mask = torch.zeros((n, n), dtype=q.dtype, device=q.device).masked_fill_(
        torch.triu(torch.ones((n, n), dtype=torch.bool, device=q.device), diagonal=1), float("-inf"))
    p = torch.softmax(mask + torch.matmul(qp, kp.transpose(-1, -2)), dim=-1)
    if training and dropout_pr > 0.0:
        p = F.dropout(p, p=float(dropout_pr))
    o = torch.matmul(p, vp).transpose(1, 2).reshape(B, n, H * d)
    return dense_to_jagged(o, seq_offsets, rows).view(rows, H, d)
