"""``SequentialFeatures`` of generative_recommenders/research/modeling/sequential/features.py: what the research encoders
and the evaluation exchange."""

from typing import Dict, NamedTuple, Optional

import torch


class SequentialFeatures(NamedTuple):
    past_lengths: torch.Tensor                 # (B,) int64, every entry > 0
    past_ids: torch.Tensor                     # (B, N) int64, 0 = padding
    past_embeddings: Optional[torch.Tensor]    # (B, N, D)
    past_payloads: Dict[str, torch.Tensor]     # implementation-specific: timestamps, ratings, ...
