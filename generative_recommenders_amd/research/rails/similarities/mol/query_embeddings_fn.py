"""Query-side component embeddings of MoL (research/rails/similarities/mol/query_embeddings_fn.py): a projection of the
query embedding to (P_Q - U) x D_P plus one hashed user-id embedding per entry of ``uid_embedding_hash_sizes`` (U of
them, read from ``kwargs["user_ids"]``), optionally L2-normalised per component.  Plain torch ops."""

from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from generative_recommenders_amd.research.rails.similarities.mol.embeddings_fn import MoLEmbeddingsFn
from generative_recommenders_amd.research.rails.similarities.mol.item_embeddings_fn import l2_normalize_components


class RecoMoLQueryEmbeddingsFn(MoLEmbeddingsFn):
    def __init__(self, query_embedding_dim: int, query_dot_product_groups: int, dot_product_dimension: int, dot_product_l2_norm: bool,
                 proj_fn: Callable[[int, int], torch.nn.Module], eps: float, uid_embedding_hash_sizes: Optional[List[int]] = None,
                 uid_dropout_rate: float = 0.0, uid_embedding_level_dropout: bool = False) -> None:
        super().__init__()
        self._uid_embedding_hash_sizes: List[int] = uid_embedding_hash_sizes or []
        self._query_emb_based_dot_product_groups: int = query_dot_product_groups - len(self._uid_embedding_hash_sizes)
        self._query_emb_proj_module: torch.nn.Module = proj_fn(
            query_embedding_dim, dot_product_dimension * self._query_emb_based_dot_product_groups)
        self._dot_product_dimension: int = dot_product_dimension
        self._dot_product_l2_norm: bool = dot_product_l2_norm
        for i, hash_size in enumerate(self._uid_embedding_hash_sizes):       # row 0 is the padding row
            setattr(self, f"_uid_embeddings_{i}", torch.nn.Embedding(hash_size + 1, dot_product_dimension, padding_idx=0))
        self._uid_dropout_rate: float = uid_dropout_rate
        self._uid_embedding_level_dropout: bool = uid_embedding_level_dropout
        self._eps: float = eps

    def _uid_component(self, i: int, hash_size: int, user_ids: torch.Tensor, aux_losses: Dict[str, torch.Tensor]) -> torch.Tensor:
        emb = getattr(self, f"_uid_embeddings_{i}")(user_ids % hash_size + 1)
        if self.training:
            l2 = (emb * emb).sum(-1).mean()
            aux_losses["uid_embedding_l2_norm"] = aux_losses["uid_embedding_l2_norm"] + l2 if i else l2
        if self._uid_dropout_rate > 0.0:
            if not self._uid_embedding_level_dropout:
                emb = F.dropout(emb, p=self._uid_dropout_rate, training=self.training)
            elif self.training:                                               # drop whole embeddings
                keep = torch.rand(emb.shape[:-1], device=emb.device) > self._uid_dropout_rate
                emb = emb * keep.unsqueeze(-1) / (1.0 - self._uid_dropout_rate)
        return emb.unsqueeze(1)

    def forward(self, input_embeddings: torch.Tensor, **kwargs) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        """(B, query_embedding_dim) -> (B, P_Q, D_P)"""
        split = self._query_emb_proj_module(input_embeddings).reshape(
            (input_embeddings.size(0), self._query_emb_based_dot_product_groups, self._dot_product_dimension))
        aux_losses: Dict[str, torch.Tensor] = {}
        if self._uid_embedding_hash_sizes:
            uid = [self._uid_component(i, h, kwargs["user_ids"], aux_losses) for i, h in enumerate(self._uid_embedding_hash_sizes)]
            split = torch.cat([split] + uid, dim=1)
        if self._dot_product_l2_norm:
            split = l2_normalize_components(split, self._eps)
        return split, aux_losses
