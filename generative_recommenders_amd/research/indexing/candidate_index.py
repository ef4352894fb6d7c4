"""Drop-in for generative_recommenders/research/indexing/candidate_index.py: the item corpus of an evaluation and the
row-wise filtering of ids a user has already seen."""

from typing import Optional, Tuple

import torch

from generative_recommenders_amd.ops.jagged_tensors import asynchronous_complete_cumsum, jagged_to_padded_dense
from generative_recommenders_amd.research.rails.indexing.candidate_index import TopKModule


class CandidateIndex(object):
    def __init__(self, ids: torch.Tensor, embeddings: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None,
                 debug_path: Optional[str] = None) -> None:
        super().__init__()
        self._ids: torch.Tensor = ids
        self._embeddings: torch.Tensor = embeddings
        self._invalid_ids: Optional[torch.Tensor] = invalid_ids
        self._debug_path: Optional[str] = debug_path

    @property
    def ids(self) -> torch.Tensor:
        """(1, X) or (B, X); valid ids are positive"""
        return self._ids

    @property
    def num_objects(self) -> int:
        return self._ids.size(1)

    @property
    def embeddings(self) -> torch.Tensor:
        """(1, X, D) or (B, X, D), matching ``ids``"""
        return self._embeddings

    def filter_invalid_ids(self, invalid_ids: torch.Tensor) -> "CandidateIndex":
        """A per-row index without ``invalid_ids`` (B, N): rows packed to the front, padded with id 0 / zero embeddings."""
        if self._ids.size(0) != 1:
            assert self._invalid_ids is None
            return CandidateIndex(ids=self.ids, embeddings=self.embeddings, invalid_ids=invalid_ids, debug_path=self._debug_path)
        B, D = invalid_ids.size(0), self._embeddings.size(-1)
        keep = ~(self._ids.unsqueeze(2) == invalid_ids.unsqueeze(1)).any(dim=2)      # (B, X)
        lengths = keep.sum(dim=1)
        flat = keep.reshape(-1)
        jagged_ids = self._ids.expand(B, -1).reshape(-1)[flat]
        jagged_embeddings = self._embeddings.expand(B, -1, -1).reshape(-1, D)[flat]
        max_len = int(lengths.max().item())
        offsets = asynchronous_complete_cumsum(lengths)
        return CandidateIndex(
            ids=jagged_to_padded_dense(jagged_ids.unsqueeze(-1), offsets, max_len).squeeze(-1),
            embeddings=jagged_to_padded_dense(jagged_embeddings, offsets, max_len),
            debug_path=self._debug_path,
        )

    def get_top_k_outputs(self, query_embeddings: torch.Tensor, k: int, top_k_module: TopKModule,
                          invalid_ids: Optional[torch.Tensor], r: int = 1,
                          return_embeddings: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """(top_k_ids, top_k_scores, None), each (B, k): the best k of the index per query row that are not among the row's
        ``invalid_ids`` (B, N0).  k + N0 results are fetched -- filtering can remove at most N0 -- and the first k survivors of
        every row are kept in order."""
        n_invalid = invalid_ids.size(1) if invalid_ids is not None else 0
        k_prime = min(k + n_invalid, self.num_objects)
        scores, ids = top_k_module(query_embeddings=query_embeddings, k=k_prime)
        if invalid_ids is not None:
            valid = ~(ids.unsqueeze(2) == invalid_ids.unsqueeze(1)).any(dim=2)       # (B, k')
            valid = valid & (valid.cumsum(dim=1) <= k)
            columns = valid.nonzero(as_tuple=True)[1].view(-1, k)                    # row-major: k survivors per row, in order
            scores, ids = scores.gather(1, columns), ids.gather(1, columns)
        if return_embeddings:
            raise ValueError("return_embeddings not supported yet.")
        return ids, scores, None

    def apply_object_filter(self) -> "CandidateIndex":
        raise NotImplementedError("not implemented.")
