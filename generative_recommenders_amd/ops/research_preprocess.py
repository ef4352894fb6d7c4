"""The input-feature preprocessors of the research path (csrc/research_preprocess.hip) as one autograd function.

``research_input_preprocess``: ``out = m * dropout(src * Do ** 0.5 + pos_table[n'])`` with ``m = past_ids != 0`` -- the
reference's scale, (B, N, D) positional gather, add, dropout and mask multiply (plus the rating gather and ``cat`` of the
rated variants) in one read and one write per direction:

* ``PREPROCESS_PLAIN``: ``LearnablePositionalEmbeddingInputFeaturesPreprocessor``
* ``PREPROCESS_CONCAT``: ``LearnablePositionalEmbeddingRatedInputFeaturesPreprocessor`` (rating columns behind the item's)
* ``PREPROCESS_INTERLEAVE``: ``CombinedItemAndRatingInputFeaturesPreprocessor`` (item row, rating row, item row, ...)

fp32 with dropout off is bit-exact against the reference's composition (forward and ``d_past_embeddings``); 16-bit computes
in fp32 and rounds once.  The dropout mask is a function of (seed, element index) -- the generator of
``hstu_norm_mul_dropout_fwd`` -- and is regenerated in the backward.  The gradients of the two tables are fp32 sums in a fixed
order: bit-identical run to run.  Nothing is read back from the device."""

from typing import Optional, Tuple

import torch

from generative_recommenders_amd.ops import _launch
from generative_recommenders_amd.ops._launch import PREPROCESS_CONCAT, PREPROCESS_INTERLEAVE, PREPROCESS_PLAIN  # noqa: F401


class _InputPreprocessFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, past_embeddings, pos_table, rating_table, past_ids, ratings, layout, dropout_ratio, seed):
        out, valid = _launch.input_preprocess_fwd(layout, past_ids, past_embeddings, ratings, pos_table, rating_table,
                                                  dropout_ratio, seed)
        ctx.save_for_backward(past_ids, ratings)
        ctx.meta = (layout, dropout_ratio, seed, past_embeddings.dtype, past_embeddings.shape[-1], pos_table.shape[0],
                    pos_table.dtype, None if rating_table is None else (tuple(rating_table.shape), rating_table.dtype))
        ctx.mark_non_differentiable(valid)
        return out, valid

    @staticmethod
    def backward(ctx, d_out, _d_valid):
        past_ids, ratings = ctx.saved_tensors
        layout, dropout_ratio, seed, emb_dtype, item_dim, num_positions, pos_dtype, rating_meta = ctx.meta
        need_emb, need_pos, need_rating = ctx.needs_input_grad[:3]
        d_emb, d_pos, d_rat = _launch.input_preprocess_bwd(
            layout, d_out, past_ids, ratings, emb_dtype, item_dim, num_positions, rating_meta[0] if rating_meta else None,
            dropout_ratio, seed, need_emb, need_pos, need_rating and rating_meta is not None)
        if d_pos is not None:
            d_pos = d_pos.to(pos_dtype)
        if d_rat is not None:
            d_rat = d_rat.to(rating_meta[1])
        return (d_emb, d_pos, d_rat) + (None,) * 5


def research_input_preprocess(
    past_ids: torch.Tensor,
    past_embeddings: torch.Tensor,
    pos_table: torch.Tensor,
    layout: int = PREPROCESS_PLAIN,
    ratings: Optional[torch.Tensor] = None,
    rating_table: Optional[torch.Tensor] = None,
    dropout_ratio: float = 0.0,
    seed: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """past_ids (B, N) int64, past_embeddings (B, N, Di), pos_table (P, Do), ratings (B, N) integer and rating_table
    (R, Dr) for the rated layouts.  Returns (out (B, N', Do) in ``torch.result_type(past_embeddings, pos_table)``,
    valid_mask (B, N', 1) fp32); N' = 2 N for ``PREPROCESS_INTERLEAVE``, else N.  ``dropout_ratio == 0`` is the plain op;
    otherwise ``seed`` fixes the mask.  Gradients flow to past_embeddings, pos_table and rating_table."""
    layout = int(layout)
    dropout_ratio = float(dropout_ratio)
    if not 0.0 <= dropout_ratio < 1.0:
        raise RuntimeError(f"research_input_preprocess: dropout_ratio must be in [0, 1), got {dropout_ratio}")
    if layout == PREPROCESS_PLAIN:
        ratings = rating_table = None
    _launch.input_preprocess_dims(layout, past_ids, past_embeddings, ratings, pos_table, rating_table)
    return _InputPreprocessFunction.apply(past_embeddings, pos_table, rating_table, past_ids, ratings, layout, dropout_ratio,
                                          int(seed))
