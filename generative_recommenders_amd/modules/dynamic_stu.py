"""Drop-in for generative_recommenders/modules/dynamic_stu.py: STUs that decide at run time how much of the batch an inner STU
sees.  ``DynamicSTU`` (:53-126) is the frame -- ``_preprocess``, the wrapped ``_stu``, ``_postprocess``; ``SDSTU`` (:129-204) is
stochastic depth over a whole STU; ``L2STU`` (:215-304) runs the inner STU on the last ``max_l2_len`` positions of every user
(plus the contextual rows in front and the targets behind) and passes the prefix rows through unchanged.  Class names,
constructor arguments, attribute names and forward signatures are the reference's.

The rows are moved by this package's jagged kernels (``hstu_split_l2_embeddings`` / ``hstu_concat_l2_embeddings``,
csrc/jagged_ops.hip) and the offsets by ``asynchronous_complete_cumsum``; neither wrapper defines ``cached_forward`` (the
reference defines none)."""

import abc
import contextlib
from typing import Any, Generator, Optional, Tuple

import torch

from generative_recommenders_amd.common import fx_infer_max_len
from generative_recommenders_amd.modules.stu import STU
from generative_recommenders_amd.ops.jagged_tensors import (
    asynchronous_complete_cumsum,
    hstu_concat_l2_embeddings,
    hstu_split_l2_embeddings,
)


@contextlib.contextmanager
def _freeze_rng_state() -> Generator[Any, None, None]:
    """the CPU generator and the current device's, saved and restored (dynamic_stu.py:38-50)"""
    rng_state = torch.get_rng_state()
    cuda_rng_state = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
    try:
        yield
    finally:
        if cuda_rng_state is not None:
            torch.cuda.set_rng_state(cuda_rng_state)
        torch.set_rng_state(rng_state)


_Preprocessed = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int, torch.Tensor, int, Optional[torch.Tensor]]


class DynamicSTU(STU):
    def __init__(self, stu: STU, is_inference: bool) -> None:
        super().__init__(is_inference)
        self._stu = stu

    @abc.abstractmethod
    def _preprocess(self, x: torch.Tensor, x_lengths: torch.Tensor, x_offsets: torch.Tensor, max_seq_len: int,
                    num_targets: torch.Tensor, max_kv_caching_len: int = 0,
                    kv_caching_lengths: Optional[torch.Tensor] = None) -> _Preprocessed:
        pass

    @abc.abstractmethod
    def _postprocess(self, stu_output: torch.Tensor) -> torch.Tensor:
        pass

    def forward(self, x: torch.Tensor, x_lengths: torch.Tensor, x_offsets: torch.Tensor, max_seq_len: int,
                num_targets: torch.Tensor, max_kv_caching_len: int = 0,
                kv_caching_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        (x, x_lengths, x_offsets, max_seq_len, num_targets, max_kv_caching_len, kv_caching_lengths) = self._preprocess(
            x=x, x_lengths=x_lengths, x_offsets=x_offsets, max_seq_len=max_seq_len, num_targets=num_targets,
            max_kv_caching_len=max_kv_caching_len, kv_caching_lengths=kv_caching_lengths)
        stu_output = self._stu(x=x, x_lengths=x_lengths, x_offsets=x_offsets, max_seq_len=max_seq_len, num_targets=num_targets,
                               max_kv_caching_len=max_kv_caching_len, kv_caching_lengths=kv_caching_lengths)
        return self._postprocess(stu_output=stu_output)


class SDSTU(DynamicSTU):
    """Stochastic depth: in training, call ``i`` (counted in ``_iter``) skips the wrapped STU iff the first uniform of a
    generator seeded with ``i + seed`` is ``<= dropout_ratio`` -- every rank draws the same decision, and the caller's CPU and
    device generators are left as they were.  On a skip the wrapped STU is still called, as in the reference, with an empty
    batch (``x`` of shape (0, D), all-zero lengths and offsets, ``max_seq_len`` 1) and the module returns the caller's ``x``
    itself.  Eval never skips.

    The empty tensor takes ``x``'s dtype; the reference's is always fp32 (``torch.empty`` without a dtype), an accident nothing
    observes: its values do not exist and its result is dropped."""

    def __init__(self, stu: STU, is_inference: bool, dropout_ratio: float = 0.5, seed: int = 0) -> None:
        super().__init__(stu=stu, is_inference=is_inference)
        self._dropout_ratio: float = dropout_ratio
        self._iter: int = 0
        self._seed: int = seed
        self._skip_x: Optional[torch.Tensor] = None

    def _preprocess(self, x: torch.Tensor, x_lengths: torch.Tensor, x_offsets: torch.Tensor, max_seq_len: int,
                    num_targets: torch.Tensor, max_kv_caching_len: int = 0,
                    kv_caching_lengths: Optional[torch.Tensor] = None) -> _Preprocessed:
        new_x, new_x_lengths, new_x_offsets, new_max_seq_len = x, x_lengths, x_offsets, max_seq_len
        if self.training:
            with _freeze_rng_state():
                torch.manual_seed(self._iter + self._seed)
                prob = torch.rand(1)
                if prob.item() <= self._dropout_ratio:
                    new_x = torch.empty(size=(0, x.shape[1]), device=x.device, dtype=x.dtype)
                    self._skip_x = x
                    new_x_lengths = torch.zeros_like(x_lengths)
                    new_x_offsets = torch.zeros_like(x_offsets)
                    new_max_seq_len = 1
            self._iter += 1
        return (new_x, new_x_lengths, new_x_offsets, new_max_seq_len, num_targets, max_kv_caching_len, kv_caching_lengths)

    def _postprocess(self, stu_output: torch.Tensor) -> torch.Tensor:
        if self.training and self._skip_x is not None:
            ret = self._skip_x
            self._skip_x = None
            return ret
        return stu_output


def _fx_unwrap_optional_tuple_tensor(
    optional: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]],
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    assert optional is not None, "Expected optional to be non-None"
    return optional


class L2STU(DynamicSTU):
    """The wrapped STU sees, per user, the contextual rows and the last ``max_l2_len`` history rows with the targets; the
    ``prefix`` in between -- max(length - max_l2_len - num_targets - contextual_seq_len, 0) rows -- goes around it."""

    def __init__(self, stu: STU, max_l2_len: int, is_inference: bool, contextual_seq_len: int = 0) -> None:
        super().__init__(stu=stu, is_inference=is_inference)
        self._max_l2_len: int = max_l2_len
        self._contextual_seq_len: int = contextual_seq_len
        self._saved_tensors: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
        self._runtime_max_l2_len: int = 0
        self._runtime_prefix_len: int = 0

    def _preprocess(self, x: torch.Tensor, x_lengths: torch.Tensor, x_offsets: torch.Tensor, max_seq_len: int,
                    num_targets: torch.Tensor, max_kv_caching_len: int = 0,
                    kv_caching_lengths: Optional[torch.Tensor] = None) -> _Preprocessed:
        prefix_lengths = x_lengths - self._max_l2_len - num_targets - self._contextual_seq_len
        prefix_lengths = torch.clamp(prefix_lengths, min=0)
        prefix_offsets = asynchronous_complete_cumsum(prefix_lengths)
        l2_lengths = x_lengths - prefix_lengths
        l2_offsets = x_offsets - prefix_offsets
        self._runtime_max_l2_len = fx_infer_max_len(l2_lengths)
        self._runtime_prefix_len = fx_infer_max_len(prefix_lengths)
        prefix_x, l2_x = hstu_split_l2_embeddings(
            max_seq_len=max_seq_len, x=x, prefix_offsets=prefix_offsets, l2_offsets=l2_offsets,
            contextual_seq_len=self._contextual_seq_len, kernel=self.hammer_kernel())
        self._saved_tensors = (prefix_offsets, prefix_x, l2_offsets)
        return (l2_x, l2_lengths, l2_offsets, self._runtime_max_l2_len, num_targets, max_kv_caching_len, kv_caching_lengths)

    def _postprocess(self, stu_output: torch.Tensor) -> torch.Tensor:
        prefix_offsets, prefix_x, l2_offsets = _fx_unwrap_optional_tuple_tensor(self._saved_tensors)
        self._saved_tensors = None
        return hstu_concat_l2_embeddings(
            max_prefix_len=self._runtime_prefix_len, prefix_x=prefix_x, prefix_offsets=prefix_offsets,
            max_l2_len=self._runtime_max_l2_len, l2_x=stu_output, l2_offsets=l2_offsets,
            contextual_seq_len=self._contextual_seq_len, kernel=self.hammer_kernel())
