"""Embedding tables trained in backward: the sparse row-wise Adagrad the reference's DLRM-v3 configurations apply through
``apply_optimizer_in_backward`` (dlrm_v3/train/utils.py:190-227; TorchRec's ``RowWiseAdagrad`` / fbgemm's exact row-wise
Adagrad with ``weight_decay = 0`` and ``lr_decay = 0``).  For every table row r among the batch's ids, and only those:

    G[r, :]      = sum over i with idx[i] == r of dout[i, :]                       (fp32)
    momentum1[r] = momentum1[r] + mean_d(G[r, d]^2)
    W[r, :]      = W[r, :] - lr / (sqrt(momentum1[r]) + eps) * G[r, :]              (the updated momentum1)

One HIP pass (csrc/embedding_optim.hip) that reads the gradient rows and touches only those table rows: no table-sized
gradient exists at any point.

Data-parallel ranks that each hold a copy of a table (``RowWiseAdagradConfig.replicated``) keep the copies bit-identical
without ever broadcasting them: every rank coalesces its batch to one fp32 row per distinct id
(``coalesce_row_gradients``), the ranks all-gather those short lists (``exchange_row_gradients``), and every rank applies
the same update to the same concatenation in rank order.  The update is deterministic and its summation order depends
only on that list, so equal inputs give equal bits.  PRECONDITION: the copies start identical
(``broadcast_fused_tables``) and every rank runs backward for the same tables in the same order -- the collectives pair
up by issue order.  ``assert_fused_tables_in_sync`` checks the outcome.

Tables stored in 16 bits (fp16 / bf16: what the reference's configurations declare, ``data_type=DataType.FP16``) keep an
fp32 ``momentum1``; the update is computed in fp32 -- the same fp32 value as for an fp32 table, bit for bit -- and the row is
written back with STOCHASTIC ROUNDING (csrc/stochastic_round.h), since round-to-nearest drops every step smaller than half
an ulp of the weight.  The random bits of an element are a function of (seed, table row, column); the seed of an update
is ``update_seed(cfg.seed, step)`` with ``step`` the table's count of applied updates, so no two steps share their draws
and a resumed run continues the sequence.  Replicated copies apply the same list with the same seed: equal bits again."""

import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

import torch

from generative_recommenders_amd import _lib as L


_LOWP = (torch.float16, torch.bfloat16)


class _FusedTableConfig:
    """What the settings of every in-backward optimizer share; mutable, read at every forward / backward
    (``set_learning_rate``).  ``rows_dtype``: the dtype of the gathered rows (None: the table's).  ``replicated``: every rank of
    ``process_group`` (None: the default group) holds a copy of the table and backward applies all ranks' row gradients to it,
    averaged over the ranks (``average``, the ``GradientAllReducer`` default) or summed; off by default.  ``seed``: the base seed
    of the stochastic rounding of a 16-bit table (``update_seed``); fp32 tables ignore it.

    A subclass states its optimizer once: ``STATE``, the per-row state keys in ``gather_rows_fused``'s order, each with the
    number of leading weight dimensions its fp32 tensor has (1: one value per row, 2: the weight's shape); ``STEP_KEY`` /
    ``COUNTS_ALWAYS``, the key of its count of applied updates and whether an fp32 table keeps one too; ``update``, the step."""

    STATE: Dict[str, int] = {}
    STEP_KEY = "rounding_step"
    COUNTS_ALWAYS = False

    def _common(self, lr: float, rows_dtype: Optional[torch.dtype], replicated: bool, process_group: Any, average: bool,
                seed: int) -> None:
        self.lr = float(lr)
        self.rows_dtype = rows_dtype
        self.replicated = bool(replicated)
        self.process_group = process_group
        self.average = bool(average)
        self.seed = int(seed)

    @classmethod
    def step_key(cls, weight_dtype: torch.dtype) -> Optional[str]:
        """the key of the table's count of applied updates, None where it keeps none"""
        return cls.STEP_KEY if cls.COUNTS_ALWAYS or weight_dtype in _LOWP else None


class RowWiseAdagradConfig(_FusedTableConfig):
    """step size and epsilon of a table trained by in-backward row-wise Adagrad (``rowwise_adagrad_update_``); the state is
    ``momentum1``, one value per row."""

    STATE = {"momentum1": 1}

    def __init__(self, lr: float, eps: float = 1e-8, rows_dtype: Optional[torch.dtype] = None, replicated: bool = False,
                 process_group: Any = None, average: bool = True, seed: int = 0) -> None:
        self._common(lr, rows_dtype, replicated, process_group, average, seed)
        self.eps = float(eps)

    def update(cfg, weight, state, idx, g, step, **rounding) -> None:        # cfg: anything with lr and eps (optimizer_of)
        rowwise_adagrad_update_(weight, state[0], idx, g, cfg.lr, cfg.eps, **rounding)


class SparseSGDConfig(_FusedTableConfig):
    """``RowWiseAdagradConfig``'s fields without ``eps`` for a table trained by in-backward sparse SGD (``sparse_sgd_update_``;
    no momentum, no weight decay, no state)."""

    def __init__(self, lr: float, rows_dtype: Optional[torch.dtype] = None, replicated: bool = False, process_group: Any = None,
                 average: bool = True, seed: int = 0) -> None:
        self._common(lr, rows_dtype, replicated, process_group, average, seed)

    def update(cfg, weight, state, idx, g, step, **rounding) -> None:
        sparse_sgd_update_(weight, idx, g, cfg.lr, **rounding)


def check_betas(betas: Any) -> Tuple[float, float]:
    """``(beta1, beta2)`` as floats; refused outside [0, 1) (NaN included)"""
    try:
        beta1, beta2 = (float(b) for b in betas)
    except (TypeError, ValueError):
        raise RuntimeError(f"betas must be a pair of numbers, got {betas!r}") from None
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise RuntimeError(f"betas must lie in [0, 1), got {(beta1, beta2)}")
    return beta1, beta2


class SparseAdamConfig(_FusedTableConfig):
    """``RowWiseAdagradConfig``'s fields plus ``betas`` for a table trained by in-backward sparse Adam (``sparse_adam_update_``).
    The count of applied updates is Adam's own ``step``, kept by every table: a 16-bit table's rounding seed is
    ``update_seed(seed, step)``."""

    STATE = {"exp_avg": 2, "exp_avg_sq": 2}
    STEP_KEY = "step"
    COUNTS_ALWAYS = True

    def __init__(self, lr: float, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 rows_dtype: Optional[torch.dtype] = None, replicated: bool = False, process_group: Any = None,
                 average: bool = True, seed: int = 0) -> None:
        self._common(lr, rows_dtype, replicated, process_group, average, seed)
        self.betas = check_betas(betas)
        self.eps = float(eps)

    def update(cfg, weight, state, idx, g, step, **rounding) -> None:
        sparse_adam_update_(weight, state[0], state[1], idx, g, cfg.lr, cfg.betas, cfg.eps, int(step), **rounding)


def optimizer_of(cfg: Any) -> type:
    """the class that describes ``cfg``'s optimizer: its own, or -- a config that is neither the Adam nor the SGD class still
    means row-wise Adagrad (``gather_rows_fused``) -- ``RowWiseAdagradConfig``"""
    return type(cfg) if isinstance(cfg, _FusedTableConfig) else RowWiseAdagradConfig


_M64 = (1 << 64) - 1


def update_seed(seed: int, step: int) -> int:
    """The 64-bit seed of a 16-bit table's update number ``step`` (0 for the first) under the base seed ``seed``: splitmix64's
    output function on ``seed + (step + 1) * 0x9E3779B97F4A7C15`` (mod 2^64) -- a bijection of the sum, so the steps of one
    run never share a seed: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31."""
    z = (int(seed) + (int(step) + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def stochastic_round(src: torch.Tensor, dtype: torch.dtype, seed: int, row_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``src`` (n, dim) fp32 rounded stochastically to ``dtype`` (float16 or bfloat16), element (i, c) with the random bits of
    ``(seed, row_ids[i] if given else i, c)`` (csrc/stochastic_round.h): the cast of an fp32 table or checkpoint to a 16-bit
    one, and the rounding a 16-bit table's update applies to its rows."""
    L.require_gpu_tensor(src, "src")
    if src.dtype != torch.float32 or src.dim() != 2:
        raise RuntimeError(f"stochastic_round: src must be float32 (n, dim), got {src.dtype} {tuple(src.shape)}")
    if dtype not in _LOWP:
        raise RuntimeError(f"stochastic_round: dtype must be float16 or bfloat16, got {dtype}")
    n, dim = src.shape
    if row_ids is not None:
        L.require_gpu_tensor(row_ids, "row_ids")
        if row_ids.device != src.device or row_ids.shape != (n,):
            raise RuntimeError(f"stochastic_round: row_ids ({n}) on {src.device}, got {tuple(row_ids.shape)} on {row_ids.device}")
        row_ids = row_ids.detach().to(torch.int32).contiguous()
    src = src.detach().contiguous()
    dst = torch.empty((n, dim), dtype=dtype, device=src.device)
    if n == 0 or dim == 0:
        return dst
    with torch.cuda.device(src.device):
        L.check(L.lib().hstu_stochastic_round(src.data_ptr(), row_ids.data_ptr() if row_ids is not None else None, dst.data_ptr(), n,
                                              dim, L.torch_dtype_code(dtype), int(seed) & _M64, L.current_stream_ptr(src.device)))
    return dst


def _sparse_update_args(fn: str, weight: torch.Tensor, state: Dict[str, torch.Tensor], idx: torch.Tensor, dout: torch.Tensor,
                        seed: Optional[int], state_dims: int = 2) -> Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]]:
    """the checks every update shares; its fp32 state tensors have the weight's first ``state_dims`` dimensions (2: the weight's
    shape, 1: one value per row); -> (dout, idx, workspace, seed as the entry point takes it), or None when the batch is empty"""
    tensors = [("weight", weight)] + list(state.items()) + [("idx", idx), ("dout", dout)]
    for name, t in tensors:
        L.require_gpu_tensor(t, name)
    if any(t.device != weight.device for _, t in tensors):
        raise RuntimeError(f"{fn}: {', '.join(n for n, _ in tensors)} must be on one device, got "
                           f"{', '.join(str(t.device) for _, t in tensors)}")
    lowp = weight.dtype in _LOWP
    if not lowp and weight.dtype != torch.float32:
        raise RuntimeError(f"{fn}: weight must be float32, float16 or bfloat16, got {weight.dtype}")
    if lowp and seed is None:
        raise RuntimeError(f"{fn}: a {weight.dtype} weight is written back by stochastic rounding and needs a seed")
    if not lowp and seed is not None:
        raise RuntimeError(f"{fn}: seed is the stochastic rounding's and a float32 weight is not rounded; pass none")
    if weight.dim() != 2 or not weight.is_contiguous():
        raise RuntimeError(f"{fn}: weight must be a contiguous (rows, dim) tensor (it is updated in place), got {tuple(weight.shape)}")
    want, want_is = weight.shape[:state_dims], "the weight's shape" if state_dims == 2 else "one value per weight row,"
    for name, t in state.items():
        if t.dtype != torch.float32 or t.shape != want or not t.is_contiguous():
            raise RuntimeError(f"{fn}: {name} must be a contiguous float32 tensor of {want_is} {tuple(want)}, got "
                               f"{t.dtype} {tuple(t.shape)}")
    rows, dim = weight.shape
    if lowp and dim % 8:
        raise RuntimeError(f"{fn}: rows of a {weight.dtype} weight must be 16-byte multiples (dim {dim} is not a multiple of 8)")
    if dout.dim() != 2 or dout.shape[1] != dim or idx.dim() != 1 or idx.shape[0] != dout.shape[0]:
        raise RuntimeError(f"{fn}: idx (n) and dout (n, {dim}), got {tuple(idx.shape)} and {tuple(dout.shape)}")
    n = idx.shape[0]
    if n == 0:
        return None
    need = C.c_int64(0)
    L.check(L.lib().hstu_embedding_rowwise_adagrad_workspace_bytes(n, rows, C.byref(need)))
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=weight.device)
    return dout.detach().contiguous(), idx.detach().to(torch.int32).contiguous(), ws, (int(seed) & _M64) if lowp else 0


def rowwise_adagrad_update_(weight: torch.Tensor, momentum1: torch.Tensor, idx: torch.Tensor, dout: torch.Tensor, lr: float,
                            eps: float = 1e-8, seed: Optional[int] = None) -> None:
    """in place: the update above on ``weight`` (rows, dim) fp32 and ``momentum1`` (rows) fp32 for the ids ``idx`` (n) and
    their gradient rows ``dout`` (n, dim) in bf16, fp16 or fp32.  Ids outside [0, rows) are the caller's error (not checked).
    fp32 rows of more than 1024 columns (the coalesced lists of wide tables) go through ``hstu_embedding_rowwise_adagrad_coalesced``.
    A float16 / bfloat16 ``weight`` (dim a multiple of 8) is updated in fp32 and written back by stochastic rounding with the
    random bits of ``seed``, which is then required (``update_seed``); an fp32 ``weight`` takes no seed."""
    args = _sparse_update_args("rowwise_adagrad_update_", weight, {"momentum1": momentum1}, idx, dout, seed, state_dims=1)
    if args is None:
        return
    dout, idx, ws, seed = args
    (rows, dim), n = weight.shape, idx.shape[0]
    tail = (ws.data_ptr(), ws.numel())
    with torch.cuda.device(weight.device):
        stream = L.current_stream_ptr(weight.device)
        if weight.dtype in _LOWP:
            L.check(L.lib().hstu_embedding_rowwise_adagrad_lowp(
                dout.data_ptr(), idx.data_ptr(), n, dim, rows, weight.data_ptr(), L.torch_dtype_code(weight.dtype), momentum1.data_ptr(),
                float(lr), float(eps), seed, *tail, L.torch_dtype_code(dout.dtype), stream))
        elif dout.dtype == torch.float32 and dim > 1024:    # fp32 rows above 4 KiB: the coalesced lists of wide tables
            L.check(L.lib().hstu_embedding_rowwise_adagrad_coalesced(
                dout.data_ptr(), idx.data_ptr(), n, dim, rows, weight.data_ptr(), momentum1.data_ptr(), float(lr), float(eps), *tail, stream))
        else:
            L.check(L.lib().hstu_embedding_rowwise_adagrad(
                dout.data_ptr(), idx.data_ptr(), n, dim, rows, weight.data_ptr(), momentum1.data_ptr(), float(lr), float(eps), *tail,
                L.torch_dtype_code(dout.dtype), stream))


def sparse_sgd_update_(weight: torch.Tensor, idx: torch.Tensor, dout: torch.Tensor, lr: float, seed: Optional[int] = None) -> None:
    """in place: ``weight[r] -= lr * G[r]`` for every row r among the ids ``idx`` (n), ``G[r]`` the fp32 sum of its gradient rows
    ``dout`` (n, dim; bf16, fp16 or fp32) -- the sum ``rowwise_adagrad_update_`` forms, addition for addition.  SGD without
    momentum or weight decay: there is no state.  ``weight`` and ``seed`` as for ``rowwise_adagrad_update_`` (a 16-bit weight is
    updated in fp32 and written back by stochastic rounding with ``seed``)."""
    args = _sparse_update_args("sparse_sgd_update_", weight, {}, idx, dout, seed)
    if args is None:
        return
    dout, idx, ws, seed = args
    with torch.cuda.device(weight.device):
        L.check(L.lib().hstu_embedding_sparse_sgd(
            dout.data_ptr(), idx.data_ptr(), idx.shape[0], weight.shape[1], weight.shape[0], weight.data_ptr(),
            L.torch_dtype_code(weight.dtype), float(lr), seed, ws.data_ptr(), ws.numel(), L.torch_dtype_code(dout.dtype),
            L.current_stream_ptr(weight.device)))


def sparse_adam_update_(weight: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, idx: torch.Tensor, dout: torch.Tensor,
                        lr: float, betas: Tuple[float, float], eps: float, step: int, seed: Optional[int] = None) -> None:
    """in place, for every row r among the ids ``idx`` (n) and only those, with ``G[r]`` as in ``sparse_sgd_update_`` and
    ``t = step + 1`` (``step``: the updates applied to the table before this one):

        exp_avg[r]    = beta1 * exp_avg[r]    + (1 - beta1) * G[r]
        exp_avg_sq[r] = beta2 * exp_avg_sq[r] + (1 - beta2) * G[r]^2
        weight[r]    -= lr / (1 - beta1^t) * exp_avg[r] / (sqrt(exp_avg_sq[r]) / sqrt(1 - beta2^t) + eps)

    ``torch.optim.Adam``'s arithmetic (``amsgrad=False``, ``weight_decay=0``) applied lazily: rows outside the batch do not
    decay, as in fbgemm's in-backward Adam and ``torch.optim.SparseAdam`` (whose eps placement is NOT used).  ``exp_avg`` and
    ``exp_avg_sq`` are (rows, dim) fp32 whatever the weight's dtype; ``weight`` and ``seed`` as for ``rowwise_adagrad_update_``."""
    beta1, beta2 = check_betas(betas)
    if int(step) < 0:
        raise RuntimeError(f"sparse_adam_update_: step counts the updates applied so far and must be >= 0, got {step}")
    args = _sparse_update_args("sparse_adam_update_", weight, {"exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq}, idx, dout, seed)
    if args is None:
        return
    dout, idx, ws, seed = args
    with torch.cuda.device(weight.device):
        L.check(L.lib().hstu_embedding_sparse_adam(
            dout.data_ptr(), idx.data_ptr(), idx.shape[0], weight.shape[1], weight.shape[0], weight.data_ptr(),
            L.torch_dtype_code(weight.dtype), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), float(lr), beta1, beta2, float(eps), int(step),
            seed, ws.data_ptr(), ws.numel(), L.torch_dtype_code(dout.dtype), L.current_stream_ptr(weight.device)))


def coalesce_row_gradients(idx: torch.Tensor, dout: torch.Tensor, table_rows: int,
                           scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(rows, G, count)``: the distinct ids of ``idx`` (n) in ascending order, ``G[s] = scale * (sum of the dout rows whose id
    is rows[s])`` in fp32 -- the sum ``rowwise_adagrad_update_`` forms for the same ``(idx, dout)``, addition for addition, the
    multiply applied once at the end -- and their number, one int32 on the device.  ``rows`` (n) int32 and ``G`` (n, dim) fp32
    are the capacity-n buffers; only the first ``count`` entries are defined.  No synchronisation happens here: the caller
    reads ``count`` when it needs it (csrc/embedding_optim.hip, ``hstu_embedding_grad_coalesce``)."""
    L.require_gpu_tensor(idx, "idx")
    L.require_gpu_tensor(dout, "dout")
    if idx.device != dout.device:
        raise RuntimeError(f"coalesce_row_gradients: idx and dout must be on one device, got {idx.device} and {dout.device}")
    if dout.dim() != 2 or idx.dim() != 1 or idx.shape[0] != dout.shape[0]:
        raise RuntimeError(f"coalesce_row_gradients: idx (n) and dout (n, dim), got {tuple(idx.shape)} and {tuple(dout.shape)}")
    n, dim = dout.shape
    dout = dout.detach().contiguous()
    idx = idx.detach().to(torch.int32).contiguous()
    rows = torch.empty(n, dtype=torch.int32, device=dout.device)
    G = torch.empty((n, dim), dtype=torch.float32, device=dout.device)
    count = torch.empty(1, dtype=torch.int32, device=dout.device)
    need = C.c_int64(0)
    L.check(L.lib().hstu_embedding_grad_coalesce_workspace_bytes(n, int(table_rows), C.byref(need)))
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dout.device)
    with torch.cuda.device(dout.device):
        L.check(L.lib().hstu_embedding_grad_coalesce(
            dout.data_ptr(), idx.data_ptr(), n, dim, int(table_rows), float(scale), rows.data_ptr(), G.data_ptr(), count.data_ptr(),
            ws.data_ptr(), ws.numel(), L.torch_dtype_code(dout.dtype), L.current_stream_ptr(dout.device)))
    return rows, G, count


def exchange_row_gradients(rows: torch.Tensor, G: torch.Tensor, count: torch.Tensor,
                           group: Any = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """All ranks' coalesced lists, concatenated IN RANK ORDER with the padding stripped: ``(rows_all, G_all)``, the same on
    every rank of ``group``.  The counts are all-gathered first and read on the host -- the one synchronisation --, then
    ``rows`` and ``G`` travel padded to the largest count.  On ``nccl`` the collectives run on device buffers; any other
    backend (``gloo``, the rehearsal backend of ``data_parallel.init_from_env``) stages them through host memory."""
    dist = torch.distributed
    world, me = dist.get_world_size(group), dist.get_rank(group)
    dev = rows.device
    via = dev if dist.get_backend(group) == "nccl" else torch.device("cpu")
    counts_t = [torch.empty(1, dtype=torch.int32, device=via) for _ in range(world)]
    dist.all_gather(counts_t, count.reshape(1).to(device=via, dtype=torch.int32), group=group)
    counts: List[int] = torch.cat(counts_t).cpu().tolist()
    cap, mine = max(counts), counts[me]
    if cap == 0:
        return rows[:0], G[:0]

    def gathered(t: torch.Tensor) -> torch.Tensor:
        send = torch.zeros((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device=via)
        send[:mine].copy_(t[:mine])
        recv = [torch.empty_like(send) for _ in range(world)]
        dist.all_gather(recv, send, group=group)
        return torch.cat([r[:c] for r, c in zip(recv, counts)]).to(dev)

    return gathered(rows), gathered(G)


def _fused_tables(collection: Any) -> Dict[str, Tuple[torch.Tensor, ...]]:
    """table name -> (weight, its state tensors: momentum1, or exp_avg and exp_avg_sq, or none for SGD) of the tables an
    ``EmbeddingCollection`` (or the model that holds one) trains in backward"""
    collection = getattr(collection, "_embedding_collection", collection)
    state = collection.fused_optimizer_state_dict()
    return {t: (collection.embeddings[t].weight.detach(),) + tuple(state[f"{t}.{k}"].detach() for k in optimizer_of(cfg).STATE)
            for t, cfg in collection._fused.items()}


def _fused_steps(collection: Any) -> Dict[str, torch.Tensor]:
    """table name -> the int64 count of applied updates of every fused table that keeps one: ``"{table}.rounding_step"`` of a
    16-bit Adagrad or SGD table, ``"{table}.step"`` of an Adam table"""
    collection = getattr(collection, "_embedding_collection", collection)
    state = collection.fused_optimizer_state_dict()
    keys = {t: f"{t}.{optimizer_of(cfg).STEP_KEY}" for t, cfg in collection._fused.items()}
    return {t: state[k] for t, k in keys.items() if k in state}


def fused_tables_checksum(collection: Any) -> Dict[str, int]:
    """Per fused table one exact integer: the wrapping int64 sum of the fp32 bit patterns (read as int32) of ``weight`` and of
    its state (``momentum1``; ``exp_avg`` and ``exp_avg_sq`` of an Adam table).  Equal tables give equal sums; one flipped bit
    changes the sum.  A 16-bit table's weight is summed through an int16 view, and a table's count of applied updates, where it
    keeps one, is added."""
    bits = lambda t: int(t.contiguous().view(torch.int16 if t.dtype in _LOWP else torch.int32).sum(dtype=torch.int64))
    wrap = lambda v: (v + (1 << 63)) % (1 << 64) - (1 << 63)
    steps = _fused_steps(collection)
    return {t: wrap(sum(bits(x) for x in ts) + (int(steps[t]) if t in steps else 0)) for t, ts in _fused_tables(collection).items()}


def assert_fused_tables_in_sync(collection: Any, group: Any = None) -> None:
    """Raise when the ranks of ``group`` hold different fused tables or states (``fused_tables_checksum``, all-gathered).
    A collective: every rank calls it.  Without a process group there is nothing to compare."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized()):
        return
    sums = fused_tables_checksum(collection)
    if not sums:
        return
    tables = _fused_tables(collection)
    dev = next(iter(tables.values()))[0].device if dist.get_backend(group) == "nccl" else torch.device("cpu")
    mine = torch.tensor([sums[t] for t in tables], dtype=torch.int64, device=dev)
    every = [torch.empty_like(mine) for _ in range(dist.get_world_size(group))]
    dist.all_gather(every, mine, group=group)
    every = torch.stack(every).cpu()
    bad = [t for i, t in enumerate(tables) if not bool((every[:, i] == every[0, i]).all())]
    if bad:
        raise RuntimeError(f"fused tables differ between ranks: {bad} (checksums per rank: "
                           f"{ {t: every[:, list(tables).index(t)].tolist() for t in bad} }).  Replicated tables stay equal only when "
                           "they start equal (broadcast_fused_tables) and every rank runs backward for the same tables in the same order")


def broadcast_fused_tables(collection: Any, src: int = 0, group: Any = None) -> None:
    """Step 0 of replicated training: every rank's fused tables and their state (``momentum1``, ``exp_avg``, ``exp_avg_sq``) become
    rank ``src``'s, and so does a table's count of applied updates (a collective; staged through host memory on backends
    other than ``nccl``)."""
    dist = torch.distributed
    on_device = dist.get_backend(group) == "nccl"
    steps = _fused_steps(collection)
    with torch.no_grad():
        for table, tensors in _fused_tables(collection).items():
            for t in tensors + ((steps[table],) if table in steps else ()):
                buf = t.to(tensors[0].device) if on_device else t.cpu()
                dist.broadcast(buf, src=src, group=group)
                if buf is not t:
                    t.copy_(buf)


def _refuse_replicated_tables() -> None:
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(
            "in-backward row-wise Adagrad updates each rank's copy of the table with that rank's gradient: replicated tables "
            f"would diverge, and sharded tables are out of scope (world size {dist.get_world_size()})")


def _apply_update(weight: torch.Tensor, state: Any, idx: torch.Tensor, g: torch.Tensor, cfg: Any, step: Any, seed: Optional[int]) -> None:
    """the update of ``cfg``'s optimizer; ``state``: momentum1 (Adagrad), (exp_avg, exp_avg_sq) (Adam), None (SGD)"""
    rounding = {} if seed is None else {"seed": seed}           # fp32 tables: the call is the one it was
    state = () if state is None else (state,) if isinstance(state, torch.Tensor) else tuple(state)
    optimizer_of(cfg).update(cfg, weight, state, idx, g, step, **rounding)


class _GatherRowsFusedFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, momentum1, idx, cfg, rows_dtype, step=None):
        ctx.save_for_backward(idx)
        ctx.table = (weight, momentum1, cfg)        # the parameter and its state themselves: the update is in place
        ctx.step = step                             # the table's count of applied updates (int64, in place too), where it keeps one
        rows = weight.index_select(0, idx)
        return rows if rows_dtype is None else rows.to(rows_dtype)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        weight, state, cfg = ctx.table
        step, seed = ctx.step, None
        none = (None,) * (5 if step is None else 6)
        lowp, adam = weight.dtype in _LOWP, optimizer_of(cfg).COUNTS_ALWAYS
        counts = optimizer_of(cfg).step_key(weight.dtype) is not None   # Adam's bias correction and a 16-bit table's rounding seed need the count
        if counts:
            if step is None:
                raise RuntimeError(f"a {weight.dtype} table trained in backward" + (" by Adam" if adam else "")
                                   + " needs its step counter (gather_rows_fused's step)")
            if idx.numel() == 0 and not getattr(cfg, "replicated", False):
                return none                         # an empty batch applies nothing and does not count
            if lowp:
                seed = update_seed(getattr(cfg, "seed", 0), int(step))
        dist = torch.distributed
        if getattr(cfg, "replicated", False) and dist.is_available() and dist.is_initialized():
            # every rank applies every rank's row gradients, in rank order: the copies of the table keep equal bits.  The
            # update's stable sort puts a row's up-to-world partial sums in rank order on every rank.
            group = cfg.process_group
            scale = 1.0 / dist.get_world_size(group) if cfg.average else 1.0
            with torch.no_grad():
                rows, G, count = coalesce_row_gradients(idx, g, weight.shape[0], scale)
                rows_all, G_all = exchange_row_gradients(rows, G, count, group)
                _apply_update(weight, state, rows_all, G_all, cfg, step, seed)
                if counts and rows_all.numel() > 0:             # the same list on every rank: the same count
                    step += 1
            return none
        _refuse_replicated_tables()
        with torch.no_grad():
            _apply_update(weight, state, idx, g, cfg, step, seed)
            if counts:
                step += 1
        return none


def gather_rows_fused(weight: torch.Tensor, momentum1: Any, idx: torch.Tensor, cfg: Any,
                      rows_dtype: Optional[torch.dtype] = None, step: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``weight[idx]`` (cast to ``rows_dtype`` when given) whose backward applies the optimizer step of ``cfg`` to ``weight`` and
    its state in place and hands autograd no gradient for the table: ``weight.grad`` stays None.  ``cfg`` picks the update: a
    ``SparseAdamConfig`` (``momentum1`` is then the pair ``(exp_avg, exp_avg_sq)``), a ``SparseSGDConfig`` (``momentum1`` is None),
    anything else with ``lr`` and ``eps`` the row-wise Adagrad step on ``momentum1``.  An Adam table and every float16 / bfloat16
    ``weight`` need ``step``, the table's int64 count of applied updates: backward takes Adam's ``t = step + 1`` and the rounding
    seed ``update_seed(cfg.seed, step)`` from it and adds 1 to it (an empty batch applies nothing and does not count)."""
    if step is None:
        return _GatherRowsFusedFunction.apply(weight, momentum1, idx, cfg, rows_dtype)
    return _GatherRowsFusedFunction.apply(weight, momentum1, idx, cfg, rows_dtype, step)
