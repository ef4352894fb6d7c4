"""The two fused row passes of DLRM-v3's input stage (csrc/preprocess_ops.hip), as autograd functions:

* ``action_encode``: ``ActionEncoder.forward`` (modules/action_encoder.py:73-112) -- bit tests, the product with the
  embedding table, the tiled target table, the cast and the ``concat_2D_jagged`` -- writes the (sum L, T * Da) result once.
* ``combine_embeddings``: ``ContextualInterleavePreprocessor.combine_embeddings``
  (modules/contextual_interleave_preprocessor.py:101-224) -- stack, mask, ``dense_to_jagged``, the boolean index (a host
  sync through ``nonzero``) and two ``concat_2D_jagged`` -- as one gather of every output row and timestamp.

Both are bit-exact against the reference's composition: every output value is a copy, a parameter rounded once, or one
add in fp32 rounded once.  Neither reads anything back from the device; the totals come from the caller's integers."""

from typing import List, Optional, Sequence, Tuple

import torch

from generative_recommenders_amd.ops import _launch
from generative_recommenders_amd.ops._launch import COMBINE_INTERLEAVE_ALL, COMBINE_INTERLEAVE_UIH, COMBINE_SUM  # noqa: F401


class _ActionEncodeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, target_table, actions, watchtimes, uih_offsets, target_offsets, weights, thresholds,
                total_uih_len, total_targets, dtype):
        out = _launch.action_encode_fwd(actions, watchtimes, uih_offsets, target_offsets, table, target_table, weights,
                                        thresholds, total_uih_len, total_targets, dtype)
        ctx.save_for_backward(actions, watchtimes, uih_offsets, target_offsets)
        ctx.meta = (weights, thresholds, total_uih_len, total_targets, table.shape[1], table.dtype, target_table.dtype,
                    tuple(target_table.shape))
        return out

    @staticmethod
    def backward(ctx, d_out):
        actions, watchtimes, uih_offsets, target_offsets = ctx.saved_tensors
        weights, thresholds, total_uih_len, total_targets, da, table_dtype, target_dtype, target_shape = ctx.meta
        d_table, d_target = _launch.action_encode_bwd(d_out, actions, watchtimes, uih_offsets, target_offsets, weights,
                                                      thresholds, total_uih_len, total_targets, da)
        return (d_table.to(table_dtype), d_target.view(target_shape).to(target_dtype)) + (None,) * 9


def action_encode(
    actions: torch.Tensor,
    watchtimes: Optional[torch.Tensor],
    uih_offsets: torch.Tensor,
    target_offsets: torch.Tensor,
    table: torch.Tensor,
    target_table: torch.Tensor,
    action_weights: Sequence[int],
    watchtime_to_action_thresholds_and_weights: Sequence[Tuple[int, int]],
    total_uih_len: int,
    total_targets: int,
    dtype: Optional[torch.dtype] = None,
) -> torch.Tensor:
    """actions (and watchtimes, when there are thresholds) int64 (total_uih_len); table (T, Da), target_table (1, T * Da);
    ``action_weights``: the T combined weights -- the action weights followed by the weights of the watchtime rule.
    Returns (total_uih_len + total_targets, T * Da) in ``dtype`` (default: the table's): per user the UIH rows, then the
    target rows.  Gradients flow to the two tables (fp32 sums in a fixed order: bit-identical run to run)."""
    weights: List[int] = [int(w) for w in action_weights]
    thresholds = [(int(t), int(w)) for t, w in watchtime_to_action_thresholds_and_weights]
    if table.dim() != 2 or target_table.numel() != table.numel():
        raise RuntimeError(f"action_encode: table (T, Da) and target_table (1, T * Da) expected, got {tuple(table.shape)} "
                           f"and {tuple(target_table.shape)}")
    if thresholds and watchtimes is None:
        raise RuntimeError("action_encode: watchtime thresholds without watchtimes")
    if dtype is None:
        dtype = table.dtype
    return _ActionEncodeFunction.apply(table, target_table, actions, watchtimes if thresholds else None, uih_offsets,
                                       target_offsets, weights, thresholds, int(total_uih_len), int(total_targets), dtype)


class _CombineFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, content, action, contextual, timestamps, seq_offsets, num_targets, out_offsets, mode, total_uih_len,
                total_targets):
        out, out_ts = _launch.combine_embeddings_fwd(content, action, contextual, timestamps, seq_offsets, num_targets,
                                                     out_offsets, mode, total_uih_len, total_targets)
        ctx.save_for_backward(seq_offsets, num_targets, out_offsets)
        ctx.meta = (mode, total_uih_len, total_targets, 0 if contextual is None else contextual.shape[1], action is not None)
        ctx.mark_non_differentiable(out_ts)
        return out, out_ts

    @staticmethod
    def backward(ctx, d_out, _d_ts):
        seq_offsets, num_targets, out_offsets = ctx.saved_tensors
        mode, total_uih_len, total_targets, contextual_len, has_action = ctx.meta
        d_content, d_action, d_ctx = _launch.combine_embeddings_bwd(d_out, seq_offsets, num_targets, out_offsets, mode,
                                                                    total_uih_len, total_targets, contextual_len, has_action)
        return (d_content, d_action, d_ctx) + (None,) * 7


def combine_embeddings(
    content_embeddings: torch.Tensor,
    action_embeddings: Optional[torch.Tensor],
    contextual_embeddings: Optional[torch.Tensor],
    seq_timestamps: torch.Tensor,
    seq_lengths: torch.Tensor,
    seq_offsets: torch.Tensor,
    num_targets: torch.Tensor,
    total_uih_len: int,
    total_targets: int,
    mode: int,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """content / action (sum L, D), contextual (B, C, D) or None, timestamps int64 (sum L).  Per user: the C contextual
    rows (timestamp 0), then -- COMBINE_SUM: content + action, L rows; COMBINE_INTERLEAVE_ALL: content and action rows
    alternating, 2 L rows; COMBINE_INTERLEAVE_UIH: alternating over the UIH rows, then the target rows of content,
    2 L - T rows.  Returns (embeddings, timestamps, lengths, offsets) of the output sequence."""
    if content_embeddings.dim() != 2:
        raise RuntimeError(f"content_embeddings must be (sum L, D), got {tuple(content_embeddings.shape)}")
    if mode != COMBINE_SUM and action_embeddings is None:
        raise RuntimeError("combine_embeddings: interleaving needs action_embeddings")
    if contextual_embeddings is not None and contextual_embeddings.dim() == 2:
        contextual_embeddings = contextual_embeddings.view(seq_lengths.numel(), -1, content_embeddings.shape[1])
    C = 0 if contextual_embeddings is None else contextual_embeddings.shape[1]
    if mode == COMBINE_SUM:
        out_lengths = seq_lengths + C if C > 0 else seq_lengths
    elif mode == COMBINE_INTERLEAVE_ALL:
        out_lengths = seq_lengths * 2 + C
    elif mode == COMBINE_INTERLEAVE_UIH:
        out_lengths = seq_lengths * 2 - num_targets.to(seq_lengths.dtype) + C
    else:
        raise RuntimeError(f"combine_embeddings: unknown mode {mode}")
    out_offsets = seq_offsets if out_lengths is seq_lengths else _launch.complete_cumsum(out_lengths)
    out, out_ts = _CombineFunction.apply(content_embeddings, action_embeddings, contextual_embeddings, seq_timestamps,
                                         seq_offsets, num_targets if mode == COMBINE_INTERLEAVE_UIH else None, out_offsets,
                                         mode, int(total_uih_len), int(total_targets))
    return out, out_ts, out_lengths, out_offsets
