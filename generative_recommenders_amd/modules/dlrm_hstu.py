"""Drop-in for generative_recommenders/modules/dlrm_hstu.py: ``SequenceEmbedding`` (:59-61), ``DlrmHSTUConfig`` (:64-97, the
same fields and defaults), ``_get_supervision_labels_and_weights`` (:100-116) and ``DlrmHSTU`` (:119-547), the DLRM-v3
ranking model the reference trains and serves -- with the reference's constructor arguments, attribute names, methods,
signatures and return tuples, every sub-module from this package: the multitask head, the contextual preprocessor, the
positional encoder, the STU stack, the ``HSTUTransducer`` and, by default, the fused ``TimestampLayerNormPostprocessor``.

torchrec is not a dependency, and TorchRec's sharding is out of scope.  ``_embedding_collection`` is
``EmbeddingCollection`` below: one ``torch.nn.Embedding`` per table in a ModuleDict named ``embeddings`` -- the state-dict
keys are TorchRec's ``embeddings.<table>.weight`` -- whose forward is a row gather per feature and whose backward is the
deterministic sorted segment sum of ``hstu_embedding_grad`` (no atomic scatter); ``apply_rowwise_adagrad_in_backward``
switches tables to the reference's training mode, row-wise Adagrad applied in backward to the touched rows only.
``embedding_tables`` and the two feature arguments are duck-typed: a table needs ``name``, ``embedding_dim``,
``num_embeddings`` and ``feature_names``; a feature container needs ``keys()``, ``values()``, ``lengths()`` and ``[key]`` (whose result has ``values()`` and ``lengths()``).
``EmbeddingConfig`` and ``KeyedJaggedTensor`` below are minimal local dataclasses of those shapes; real TorchRec objects work
unchanged.  For serving, ``quantize_embeddings`` turns the trained collection into a ``QuantEmbeddingCollection`` of int8 row-wise
quantized tables, as the reference's inference flow does (dlrm_v3/inference/model_family.py:122-143).  (The reference's ``set_static_max_seq_lens`` call configures its Triton autotuner and has no counterpart here.)"""

import copy
import logging
from dataclasses import dataclass, field
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import torch
from torch.autograd.profiler import record_function

from generative_recommenders_amd.common import HammerModule
from generative_recommenders_amd.modules.contextualize_mlps import init_mlp_weights_optional_bias
from generative_recommenders_amd.modules.hstu_transducer import HSTUTransducer
from generative_recommenders_amd.modules.multitask_module import DefaultMultitaskModule, MultitaskTaskType, TaskConfig
from generative_recommenders_amd.modules.positional_encoder import HSTUPositionalEncoder
from generative_recommenders_amd.modules.postprocessors import LayerNormPostprocessor, TimestampLayerNormPostprocessor
from generative_recommenders_amd.modules.preprocessors import ContextualPreprocessor
from generative_recommenders_amd.modules.stu import STU, STULayer, STULayerConfig, STUStack
from generative_recommenders_amd.ops.embedding import (RowWiseAdagradConfig, SparseAdamConfig, SparseSGDConfig, check_betas,
                                                       gather_rows_fused, optimizer_of)
from generative_recommenders_amd.ops.jagged_tensors import asynchronous_complete_cumsum, concat_2D_jagged
from generative_recommenders_amd.ops.layer_norm import LayerNorm, SwishLayerNorm
from generative_recommenders_amd.ops.position import _table_grad
from generative_recommenders_amd.ops.quant_embedding import gather_rows_int8, int8_row_stride, quantize_rows_int8

logger: logging.Logger = logging.getLogger(__name__)


class SequenceEmbedding(NamedTuple):
    lengths: torch.Tensor
    embedding: torch.Tensor


@dataclass
class DlrmHSTUConfig:
    max_seq_len: int = 2056
    max_num_candidates: int = 10
    max_num_candidates_inference: int = 5
    hstu_num_heads: int = 1
    hstu_attn_linear_dim: int = 256
    hstu_attn_qk_dim: int = 128
    hstu_attn_num_layers: int = 12
    hstu_embedding_table_dim: int = 192
    hstu_transducer_embedding_dim: int = 0
    hstu_group_norm: bool = False
    hstu_input_dropout_ratio: float = 0.2
    hstu_linear_dropout_rate: float = 0.2
    contextual_feature_to_max_length: Dict[str, int] = field(default_factory=dict)
    contextual_feature_to_min_uih_length: Dict[str, int] = field(default_factory=dict)
    candidates_weight_feature_name: str = ""
    candidates_watchtime_feature_name: str = ""
    candidates_querytime_feature_name: str = ""
    causal_multitask_weights: float = 0.2
    multitask_configs: List[TaskConfig] = field(default_factory=list)
    user_embedding_feature_names: List[str] = field(default_factory=list)
    item_embedding_feature_names: List[str] = field(default_factory=list)
    uih_post_id_feature_name: str = ""
    uih_action_time_feature_name: str = ""
    uih_weight_feature_name: str = ""
    hstu_uih_feature_names: List[str] = field(default_factory=list)
    hstu_candidate_feature_names: List[str] = field(default_factory=list)
    merge_uih_candidate_feature_mapping: List[Tuple[str, str]] = field(default_factory=list)
    action_weights: Optional[List[int]] = None
    enable_postprocessor: bool = True
    use_layer_norm_postprocessor: bool = False


# ------------------------------------------------------------------------------------------- the TorchRec-shaped stand-ins
_TABLE_DTYPES = {"FP32": torch.float32, "FP16": torch.float16, "BF16": torch.bfloat16}


def table_dtype(data_type: Any) -> torch.dtype:
    """The torch dtype of a table's declared ``data_type``: TorchRec's ``DataType.FP32 / FP16 / BF16`` (duck-typed: an enum
    member's ``.name`` or ``.value``), the strings ``"FP32" / "FP16" / "BF16"`` in any case, or a torch dtype.  The
    reference's DLRM-v3 tables are all ``DataType.FP16`` (dlrm_v3/configs.py:293-440)."""
    if isinstance(data_type, torch.dtype):
        if data_type in _TABLE_DTYPES.values():
            return data_type
    else:
        for key in (data_type, getattr(data_type, "name", None), getattr(data_type, "value", None)):
            if isinstance(key, str) and key.upper() in _TABLE_DTYPES:
                return _TABLE_DTYPES[key.upper()]
    raise ValueError(f"embedding table data_type {data_type!r} is not supported: accepted are DataType.FP32 / FP16 / BF16 (or their "
                     f"names {sorted(_TABLE_DTYPES)}) and torch.float32 / float16 / bfloat16")


@dataclass
class EmbeddingConfig:
    """the attributes of torchrec.modules.embedding_configs.EmbeddingConfig that DlrmHSTU touches; ``data_type``: what
    ``table_dtype`` accepts (checked on construction)"""
    num_embeddings: int
    embedding_dim: int
    name: str = ""
    feature_names: List[str] = field(default_factory=list)
    data_type: Any = "FP32"

    def __post_init__(self) -> None:
        table_dtype(self.data_type)


@dataclass
class JaggedTensor:
    """values of one feature and its per-user lengths"""
    _values: torch.Tensor
    _lengths: torch.Tensor

    def values(self) -> torch.Tensor:
        return self._values

    def lengths(self) -> torch.Tensor:
        return self._lengths


@dataclass
class KeyedJaggedTensor:
    """keys, the concatenated values of every key (key-major) and the (num_keys * batch) lengths, as TorchRec lays them out"""
    _keys: List[str]
    _values: torch.Tensor
    _lengths: torch.Tensor

    @staticmethod
    def from_lengths_sync(keys: List[str], values: torch.Tensor, lengths: torch.Tensor) -> "KeyedJaggedTensor":
        return KeyedJaggedTensor(list(keys), values, lengths)

    def keys(self) -> List[str]:
        return self._keys

    def values(self) -> torch.Tensor:
        return self._values

    def lengths(self) -> torch.Tensor:
        return self._lengths

    def __getitem__(self, key: str) -> JaggedTensor:
        k = self._keys.index(key)
        per_key = self._lengths.view(len(self._keys), -1)
        totals = per_key.sum(dim=1).tolist()
        start = int(sum(totals[:k]))
        return JaggedTensor(self._values[start:start + int(totals[k])], per_key[k])


class _GatherRowsFunction(torch.autograd.Function):
    """table[idx]; the table gradient is the sorted segment sum of hstu_embedding_grad: fixed order, no atomics"""

    @staticmethod
    def forward(ctx, table, idx):
        ctx.save_for_backward(idx)
        ctx.meta = (table.shape[0], table.dtype)
        return table.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        rows, dtype = ctx.meta
        if idx.numel() == 0:
            return g.new_zeros((rows, g.shape[1]), dtype=dtype), None
        return _table_grad(g.contiguous(), idx.to(torch.int32).contiguous(), rows).to(dtype), None


class EmbeddingCollection(torch.nn.Module):
    """one torch.nn.Embedding per table in ``embeddings`` (TorchRec's state-dict keys); forward: every key of the feature
    container that belongs to a table -> JaggedTensor(rows of its table, the key's lengths)"""

    def __init__(self, tables: List[Any], need_indices: bool = False, device: Optional[torch.device] = None) -> None:
        super().__init__()
        del need_indices
        self.embeddings = torch.nn.ModuleDict(
            {t.name: torch.nn.Embedding(t.num_embeddings, t.embedding_dim, device=device) for t in tables})
        # the declared dtype per table (no data_type attribute: fp32).  A 16-bit table is the fp32 initial values
        # rounded to nearest: the same RNG stream gives the same table up to the cast
        self._table_dtype: Dict[str, torch.dtype] = {t.name: table_dtype(getattr(t, "data_type", "FP32")) for t in tables}
        for name, dtype in self._table_dtype.items():
            if dtype != torch.float32:
                self.embeddings[name].to(dtype)
        self._feature_to_table: Dict[str, str] = {f: t.name for t in tables for f in t.feature_names}
        self._fused: Dict[str, Any] = {}        # tables trained in backward -> their optimizer's config (apply_optimizer_in_backward)

    def forward(self, features: Any) -> Dict[str, JaggedTensor]:
        fused_rows = self._fused_forward(features) if self._fused else {}
        out: Dict[str, JaggedTensor] = {}
        for key in features.keys():
            table = self._feature_to_table.get(key)
            if table is None:
                continue
            jt = features[key]
            if key in fused_rows:
                out[key] = JaggedTensor(fused_rows[key], jt.lengths())
                continue
            weight = self.embeddings[table].weight
            idx = jt.values().to(torch.int64)
            rows = _GatherRowsFunction.apply(weight, idx) if weight.is_cuda else weight.index_select(0, idx)
            out[key] = JaggedTensor(rows, jt.lengths())
        return out

    # ----------------------------------------------------------------------------- tables trained in backward (opt-in)
    def _fused_forward(self, features: Any) -> Dict[str, torch.Tensor]:
        """ONE gather per fused table over the ids of all its features, split back per feature: backward then sees the
        table's summed gradient once (what a table-batched lookup does; Adagrad applied per feature is not Adagrad)"""
        keys_of: Dict[str, List[str]] = {}
        for key in features.keys():
            table = self._feature_to_table.get(key)
            if table in self._fused:
                keys_of.setdefault(table, []).append(key)
        rows_of: Dict[str, torch.Tensor] = {}
        for table, keys in keys_of.items():
            weight = self.embeddings[table].weight
            cfg = self._fused[table]
            opt = optimizer_of(cfg)
            state = [getattr(self, _buffer_name(key, table)) for key in opt.STATE]
            declared = self._table_dtype.get(table, torch.float32)
            if weight.dtype != declared or any(t.dtype != torch.float32 for t in state):
                raise RuntimeError(f"table {table!r} is trained in backward and must stay {_dtype_name(declared)} (got {weight.dtype}, "
                                   f"state {', '.join(str(t.dtype) for t in state) or 'none'}); ask for 16-bit rows with rows_dtype "
                                   "instead of casting the table")
            ids = [features[k].values().to(torch.int64) for k in keys]
            # what gather_rows_fused takes as the state: Adagrad's momentum1, Adam's pair, None for SGD
            packed = tuple(state) if len(state) > 1 else state[0] if state else None
            step = getattr(self, _buffer_name(opt.STEP_KEY, table), None)
            rows = gather_rows_fused(weight, packed, ids[0] if len(ids) == 1 else torch.cat(ids), cfg, cfg.rows_dtype, step)
            rows_of.update(zip(keys, rows.split([i.numel() for i in ids]) if len(ids) > 1 else (rows,)))
        return rows_of

    def apply_rowwise_adagrad_in_backward(self, lr: float, eps: float = 1e-8, weight_decay: float = 0.0,
                                          rows_dtype: Optional[torch.dtype] = None, tables: Optional[List[str]] = None,
                                          replicated: bool = False, process_group: Any = None, average: bool = True,
                                          seed: int = 0) -> None:
        apply_rowwise_adagrad_in_backward(self, lr, eps=eps, weight_decay=weight_decay, rows_dtype=rows_dtype, tables=tables,
                                          replicated=replicated, process_group=process_group, average=average, seed=seed)

    def apply_optimizer_in_backward(self, optimizer_name: str, learning_rate: float, betas: Tuple[float, float] = (0.9, 0.999),
                                    eps: float = 1e-8, weight_decay: float = 0.0, momentum: float = 0.0,
                                    rows_dtype: Optional[torch.dtype] = None, tables: Optional[List[str]] = None,
                                    replicated: bool = False, process_group: Any = None, average: bool = True, seed: int = 0,
                                    amsgrad: bool = False) -> None:
        apply_optimizer_in_backward(self, optimizer_name, learning_rate, betas=betas, eps=eps, weight_decay=weight_decay,
                                    momentum=momentum, rows_dtype=rows_dtype, tables=tables, replicated=replicated,
                                    process_group=process_group, average=average, seed=seed, amsgrad=amsgrad)

    def set_learning_rate(self, lr: float) -> None:
        for cfg in self._fused.values():
            cfg.lr = float(lr)

    def fused_optimizer_state_dict(self) -> Dict[str, torch.Tensor]:
        """Per fused table, by its optimizer.  Row-wise Adagrad: ``"{table}.momentum1"``, and ``"{table}.rounding_step"`` -- the int64
        count of applied updates that, with the configured seed, determines the next update's stochastic rounding -- for a
        16-bit table.  Adam: ``"{table}.exp_avg"``, ``"{table}.exp_avg_sq"`` and ``"{table}.step"``, the count of applied updates
        behind the bias correction and, for a 16-bit table, behind the rounding seed as well.  SGD: ``"{table}.rounding_step"``
        for a 16-bit table, else nothing."""
        state: Dict[str, torch.Tensor] = {}
        for table, cfg in self._fused.items():
            opt = optimizer_of(cfg)
            for key in tuple(opt.STATE) + ((opt.STEP_KEY,) if hasattr(self, _buffer_name(opt.STEP_KEY, table)) else ()):
                state[f"{table}.{key}"] = getattr(self, _buffer_name(key, table))
        return state

    def load_fused_optimizer_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        want = set(self.fused_optimizer_state_dict())
        if set(state) != want:
            raise KeyError(f"fused optimizer state: expected the keys {sorted(want)}, got {sorted(state)}")
        with torch.no_grad():
            for key, mine in self.fused_optimizer_state_dict().items():
                mine.copy_(state[key])


def _buffer_name(key: str, table: str) -> str:
    """the non-persistent buffer behind ``"{table}.{key}"`` of ``fused_optimizer_state_dict``"""
    return f"_{key}_" + table.replace(".", "_")


def _dtype_name(dtype: torch.dtype) -> str:
    return str(dtype).replace("torch.", "")


def apply_rowwise_adagrad_in_backward(collection: Any, lr: float, eps: float = 1e-8, weight_decay: float = 0.0,
                                      rows_dtype: Optional[torch.dtype] = None, tables: Optional[List[str]] = None,
                                      replicated: bool = False, process_group: Any = None, average: bool = True,
                                      seed: int = 0) -> None:
    """Train the named tables of an ``EmbeddingCollection`` (default: all; a ``DlrmHSTU`` stands for its collection) with
    row-wise Adagrad applied in backward -- what ``apply_optimizer_in_backward(RowWiseAdagrad, ...)`` does to the reference's
    TorchRec modules (dlrm_v3/train/utils.py:190-227).  Afterwards the forward issues one gather per table, backward updates
    the touched rows in place (ops/embedding.py) and leaves ``weight.grad`` None, so a dense optimizer over
    ``model.parameters()`` skips these tables.  ``lr``, ``eps`` and ``rows_dtype`` are kept per table: a later call that names
    other tables leaves the earlier ones as they were.  The state is one fp32 ``momentum1`` per table row, a non-persistent buffer
    (the module's state_dict keeps TorchRec's keys; see ``fused_optimizer_state_dict``).

    ``replicated=True``: data-parallel training with a copy of the table on every rank of ``process_group`` (None: the default
    group).  Backward then applies the row gradients of ALL ranks -- their mean with ``average`` (what ``GradientAllReducer``
    does to the dense gradients), else their sum -- in rank order on every rank, so the copies keep equal bits
    (ops/embedding.py).  PRECONDITION: the copies start identical (``ops.embedding.broadcast_fused_tables``) and every rank calls
    backward for the same tables in the same order.  Off by default: without it more than one rank is refused.  The three
    settings are kept per table like ``lr``.

    A table declared FP16 / BF16 (``EmbeddingConfig.data_type``) keeps its 16-bit weight and an fp32 ``momentum1``; its update
    is computed in fp32 and written back by stochastic rounding (ops/embedding.py).  ``seed`` is the rounding's base seed; an
    int64 count of applied updates, a second non-persistent buffer kept in host memory (reading it never waits for the
    GPU), makes every step's draws its own.  Every table must still have the dtype it was declared with."""
    collection = getattr(collection, "_embedding_collection", collection)
    if weight_decay != 0.0:
        raise NotImplementedError(f"weight_decay = {weight_decay}: TorchRec's RowWiseAdagrad and fbgemm's exact row-wise Adagrad "
                                  "apply it differently and no reference configuration sets it; only 0 is supported")
    for table in _checked_tables(collection, rows_dtype, tables):
        _set_table_optimizer(collection, table, RowWiseAdagradConfig(lr, eps, rows_dtype, replicated, process_group, average, seed))


def _checked_tables(collection: Any, rows_dtype: Optional[torch.dtype], tables: Optional[List[str]]) -> List[str]:
    """the named tables (default: all), each still of the dtype it was declared with"""
    if rows_dtype not in (None, torch.float32, torch.bfloat16, torch.float16):
        raise RuntimeError(f"rows_dtype must be float32, bfloat16 or float16, got {rows_dtype}")
    names = list(collection.embeddings.keys()) if tables is None else list(tables)
    for table in names:
        if table not in collection.embeddings:
            raise KeyError(f"no embedding table named {table!r}")
        weight = collection.embeddings[table].weight
        declared = getattr(collection, "_table_dtype", {}).get(table, torch.float32)
        if weight.dtype != declared:
            raise RuntimeError(f"table {table!r} is {weight.dtype}: tables trained in backward must be {_dtype_name(declared)}"
                               + ("" if declared == torch.float32 else ", the data_type they were declared with"))
    return names


def _set_table_optimizer(collection: Any, table: str, cfg: Any) -> None:
    """``cfg`` becomes the table's settings.  A table named again with the optimizer it has keeps its state; with another
    optimizer the old state is dropped and the new one starts from zero."""
    old = collection._fused.get(table)
    if old is not None and type(old) is type(cfg):
        old.__dict__.update(cfg.__dict__)                # named again: this call's settings replace the table's
        return
    if old is not None:
        for key in tuple(optimizer_of(old).STATE) + (optimizer_of(old).STEP_KEY,):
            if hasattr(collection, _buffer_name(key, table)):
                delattr(collection, _buffer_name(key, table))
    weight, opt = collection.embeddings[table].weight, optimizer_of(cfg)
    for key, dims in opt.STATE.items():
        collection.register_buffer(_buffer_name(key, table), torch.zeros(weight.shape[:dims], dtype=torch.float32, device=weight.device),
                                   persistent=False)
    if opt.step_key(weight.dtype) is not None:
        collection.register_buffer(_buffer_name(opt.step_key(weight.dtype), table), torch.zeros((), dtype=torch.int64, device="cpu"),
                                   persistent=False)
    collection._fused[table] = cfg


def apply_optimizer_in_backward(collection: Any, optimizer_name: str, learning_rate: float, betas: Tuple[float, float] = (0.9, 0.999),
                                eps: float = 1e-8, weight_decay: float = 0.0, momentum: float = 0.0,
                                rows_dtype: Optional[torch.dtype] = None, tables: Optional[List[str]] = None, replicated: bool = False,
                                process_group: Any = None, average: bool = True, seed: int = 0, amsgrad: bool = False) -> None:
    """The front door with the argument names of the reference's ``sparse_optimizer_factory_and_class``
    (dlrm_v3/train/utils.py:169-206): train the named tables (default: all) in backward with ``optimizer_name`` =
    ``"RowWiseAdagrad"`` (``apply_rowwise_adagrad_in_backward``, unchanged), ``"Adam"`` or ``"SGD"`` (ops/embedding.py:
    ``sparse_adam_update_``, ``sparse_sgd_update_``).  Tables of one collection may use different optimizers; settings and state
    are kept per table, and everything ``apply_rowwise_adagrad_in_backward`` says about ``rows_dtype``, replicated tables and
    16-bit tables holds for all three.

    Adam is ``torch.optim.Adam``'s arithmetic applied LAZILY: only the rows of the batch move, the others' moments do not
    decay (dense ``torch.optim.Adam`` moves every row whose moments are non-zero).  Its state is ``exp_avg`` and
    ``exp_avg_sq``, (rows, dim) fp32 each, and one int64 ``step`` per table in host memory that counts APPLIED updates: an empty
    batch does not count (``torch.optim.Adam`` counts it), a replicated table counts when the ranks' concatenated list is
    non-empty.  A 16-bit Adam table takes its rounding seed from the same counter.

    Refused: ``weight_decay != 0``, SGD ``momentum != 0`` (every reference configuration sets 0 and fbgemm's exact SGD has none),
    ``amsgrad``, betas outside [0, 1)."""
    if optimizer_name == "RowWiseAdagrad":
        apply_rowwise_adagrad_in_backward(collection, learning_rate, eps=eps, weight_decay=weight_decay, rows_dtype=rows_dtype,
                                          tables=tables, replicated=replicated, process_group=process_group, average=average,
                                          seed=seed)
        return
    if optimizer_name not in ("Adam", "SGD"):
        raise ValueError(f"optimizer_name must be 'RowWiseAdagrad', 'Adam' or 'SGD', got {optimizer_name!r}")
    if weight_decay != 0.0:
        raise NotImplementedError(f"weight_decay = {weight_decay}: the in-backward {optimizer_name} has none and no reference "
                                  "configuration sets it; only 0 is supported")
    if optimizer_name == "SGD" and momentum != 0.0:
        raise NotImplementedError(f"momentum = {momentum}: the in-backward SGD keeps no state (fbgemm's exact SGD has no momentum and "
                                  "every reference configuration sets 0); only 0 is supported")
    if amsgrad:
        raise NotImplementedError("amsgrad: the in-backward Adam keeps no running maximum of exp_avg_sq; only amsgrad=False is supported")
    if optimizer_name == "Adam":
        betas = check_betas(betas)
    collection = getattr(collection, "_embedding_collection", collection)
    for table in _checked_tables(collection, rows_dtype, tables):
        cfg = (SparseAdamConfig(learning_rate, betas, eps, rows_dtype, replicated, process_group, average, seed)
               if optimizer_name == "Adam" else SparseSGDConfig(learning_rate, rows_dtype, replicated, process_group, average, seed))
        _set_table_optimizer(collection, table, cfg)


# --------------------------------------------------------------------------- int8 row-wise quantized tables (inference)
class _QuantTable(torch.nn.Module):
    """one quantized table: the persistent buffer ``weight``, uint8 (rows, int8_row_stride(dim)) (ops/quant_embedding.py)"""

    def __init__(self, num_embeddings: int, embedding_dim: int, device: Optional[torch.device] = None) -> None:
        super().__init__()
        self.num_embeddings, self.embedding_dim = int(num_embeddings), int(embedding_dim)
        self.register_buffer("weight", torch.zeros((self.num_embeddings, int8_row_stride(self.embedding_dim)), dtype=torch.uint8,
                                                   device=device))


class QuantEmbeddingCollection(torch.nn.Module):
    """``EmbeddingCollection`` over int8 row-wise quantized tables, what the reference's DLRM-v3 inference flow serves
    (dlrm_v3/inference/model_family.py:122-143: ``quantize_dynamic`` of every EmbeddingCollection, int8 weights, float
    activations).  The same ``forward(features) -> Dict[str, JaggedTensor]`` and feature-to-table mapping; the state-dict keys
    are ``embeddings.<table>.weight``, uint8 (rows, stride) buffers.  The forward issues ONE dequantizing gather per table over
    the concatenated ids of all its features (``hstu_gather_rows_int8``) and splits the rows back per feature; the rows come
    out in ``output_dtype``.  Inference only: nothing here has a gradient."""

    def __init__(self, tables: List[Any], output_dtype: torch.dtype = torch.float32, device: Optional[torch.device] = None) -> None:
        super().__init__()
        if output_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"output_dtype must be float32, float16 or bfloat16, got {output_dtype}")
        self.embeddings = torch.nn.ModuleDict({t.name: _QuantTable(t.num_embeddings, t.embedding_dim, device) for t in tables})
        self._output_dtype = output_dtype
        self._feature_to_table: Dict[str, str] = {f: t.name for t in tables for f in t.feature_names}

    @classmethod
    def from_float(cls, collection: EmbeddingCollection, output_dtype: torch.dtype = torch.float32) -> "QuantEmbeddingCollection":
        """quantize every table (FP32, FP16 or BF16) of an ``EmbeddingCollection``, on the device it lives on"""
        names = list(collection.embeddings.keys())
        weights = {n: collection.embeddings[n].weight.detach() for n in names}
        tables = [EmbeddingConfig(num_embeddings=w.shape[0], embedding_dim=w.shape[1], name=n,
                                  feature_names=[f for f, t in collection._feature_to_table.items() if t == n])
                  for n, w in weights.items()]
        out = cls(tables, output_dtype=output_dtype, device=torch.device("meta"))
        for n, w in weights.items():
            out.embeddings[n]._buffers["weight"] = quantize_rows_int8(w)
        return out

    def forward(self, features: Any) -> Dict[str, JaggedTensor]:
        keys_of: Dict[str, List[str]] = {}
        for key in features.keys():
            table = self._feature_to_table.get(key)
            if table is not None:
                keys_of.setdefault(table, []).append(key)
        rows_of: Dict[str, torch.Tensor] = {}
        for table, keys in keys_of.items():
            module = self.embeddings[table]
            ids = [features[k].values().to(torch.int64) for k in keys]
            rows = gather_rows_int8(module.weight, module.embedding_dim, ids[0] if len(ids) == 1 else torch.cat(ids), self._output_dtype)
            rows_of.update(zip(keys, rows.split([i.numel() for i in ids]) if len(ids) > 1 else (rows,)))
        return {key: JaggedTensor(rows_of[key], features[key].lengths()) for key in features.keys() if key in rows_of}


def quantize_embeddings(module: Any, output_dtype: torch.dtype = torch.float32, inplace: bool = False) -> Any:
    """The conversion after training, as in the reference: an ``EmbeddingCollection`` -> its ``QuantEmbeddingCollection``; a
    ``DlrmHSTU`` -> the model with ``_embedding_collection`` replaced (a copy that shares nothing with ``module`` unless
    ``inplace``; the float tables are not copied).  A model must be ``is_inference`` and in eval mode.  In-backward optimizer
    state is not carried over."""
    if isinstance(module, EmbeddingCollection):
        return QuantEmbeddingCollection.from_float(module, output_dtype)
    if not isinstance(module, DlrmHSTU):
        raise TypeError(f"quantize_embeddings takes an EmbeddingCollection or a DlrmHSTU, got {type(module).__name__}")
    if not module._is_inference:
        raise RuntimeError("quantize_embeddings: int8 tables are for serving; the model must be built with is_inference=True")
    if module.training:
        raise RuntimeError("quantize_embeddings: the model is in training mode; call eval() first")
    collection = module._embedding_collection
    if not isinstance(collection, EmbeddingCollection):
        raise RuntimeError(f"quantize_embeddings: the model's tables are already a {type(collection).__name__}")
    quantized = QuantEmbeddingCollection.from_float(collection, output_dtype)
    if not inplace:
        module = copy.deepcopy(module, {id(collection): None})      # everything but the float tables
    module._embedding_collection = quantized
    return module


def _get_supervision_labels_and_weights(
    supervision_bitmasks: torch.Tensor,
    watchtime_sequence: torch.Tensor,
    task_configs: List[TaskConfig],
) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    supervision_labels: Dict[str, torch.Tensor] = {}
    supervision_weights: Dict[str, torch.Tensor] = {}
    for task in task_configs:
        if task.task_type == MultitaskTaskType.REGRESSION:
            supervision_labels[task.task_name] = watchtime_sequence.to(torch.float32)
        elif task.task_type == MultitaskTaskType.BINARY_CLASSIFICATION:
            supervision_labels[task.task_name] = (torch.bitwise_and(supervision_bitmasks, task.task_weight) > 0).to(torch.float32)
        else:
            raise RuntimeError("Unsupported MultitaskTaskType")
    return supervision_labels, supervision_weights


class DlrmHSTU(HammerModule):
    def __init__(  # noqa C901
        self,
        hstu_configs: DlrmHSTUConfig,
        embedding_tables: Dict[str, Any],
        is_inference: bool,
    ) -> None:
        super().__init__(is_inference=is_inference)
        logger.info(f"Initialize HSTU module with configs {hstu_configs}")
        self._hstu_configs = hstu_configs

        self._embedding_collection = EmbeddingCollection(tables=list(embedding_tables.values()), need_indices=False)

        # multitask configs must be sorted by task types
        self._multitask_configs: List[TaskConfig] = hstu_configs.multitask_configs
        self._multitask_module = DefaultMultitaskModule(
            task_configs=self._multitask_configs,
            embedding_dim=hstu_configs.hstu_transducer_embedding_dim,
            prediction_fn=lambda in_dim, num_tasks: torch.nn.Sequential(
                torch.nn.Linear(in_features=in_dim, out_features=512),
                SwishLayerNorm(512),
                torch.nn.Linear(in_features=512, out_features=num_tasks),
            ).apply(init_mlp_weights_optional_bias),
            causal_multitask_weights=hstu_configs.causal_multitask_weights,
            is_inference=self._is_inference,
        )

        # preprocessor setup
        preprocessor = ContextualPreprocessor(
            input_embedding_dim=hstu_configs.hstu_embedding_table_dim,
            output_embedding_dim=hstu_configs.hstu_transducer_embedding_dim,
            contextual_feature_to_max_length=hstu_configs.contextual_feature_to_max_length,
            contextual_feature_to_min_uih_length=hstu_configs.contextual_feature_to_min_uih_length,
            action_embedding_dim=8,
            action_feature_name=self._hstu_configs.uih_weight_feature_name,
            action_weights=self._hstu_configs.action_weights,
            is_inference=is_inference,
        )

        # positional encoder
        positional_encoder = HSTUPositionalEncoder(
            num_position_buckets=8192,
            num_time_buckets=2048,
            embedding_dim=hstu_configs.hstu_transducer_embedding_dim,
            contextual_seq_len=sum(dict(hstu_configs.contextual_feature_to_max_length).values()),
            is_inference=self._is_inference,
        )

        if hstu_configs.enable_postprocessor:
            if hstu_configs.use_layer_norm_postprocessor:
                postprocessor = LayerNormPostprocessor(
                    embedding_dim=hstu_configs.hstu_transducer_embedding_dim,
                    eps=1e-5,
                    is_inference=self._is_inference,
                )
            else:
                postprocessor = TimestampLayerNormPostprocessor(
                    embedding_dim=hstu_configs.hstu_transducer_embedding_dim,
                    time_duration_features=[
                        (60 * 60, 24),  # hour of day
                        (24 * 60 * 60, 7),  # day of week
                    ],
                    eps=1e-5,
                    is_inference=self._is_inference,
                )
        else:
            postprocessor = None

        # construct HSTU
        stu_module: STU = STUStack(
            stu_list=[
                STULayer(
                    config=STULayerConfig(
                        embedding_dim=hstu_configs.hstu_transducer_embedding_dim,
                        num_heads=hstu_configs.hstu_num_heads,
                        hidden_dim=hstu_configs.hstu_attn_linear_dim,
                        attention_dim=hstu_configs.hstu_attn_qk_dim,
                        output_dropout_ratio=hstu_configs.hstu_linear_dropout_rate,
                        use_group_norm=hstu_configs.hstu_group_norm,
                        causal=True,
                        target_aware=True,
                        max_attn_len=None,
                        attn_alpha=None,
                        recompute_normed_x=True,
                        recompute_uvqk=True,
                        recompute_y=True,
                        sort_by_length=True,
                        contextual_seq_len=0,
                    ),
                    is_inference=is_inference,
                )
                for _ in range(hstu_configs.hstu_attn_num_layers)
            ],
            is_inference=is_inference,
        )
        self._hstu_transducer: HSTUTransducer = HSTUTransducer(
            stu_module=stu_module,
            input_preprocessor=preprocessor,
            output_postprocessor=postprocessor,
            input_dropout_ratio=hstu_configs.hstu_input_dropout_ratio,
            positional_encoder=positional_encoder,
            is_inference=self._is_inference,
            return_full_embeddings=False,
            listwise=False,
        )

        # item embeddings
        self._item_embedding_mlp: torch.nn.Module = torch.nn.Sequential(
            torch.nn.Linear(
                in_features=hstu_configs.hstu_embedding_table_dim * len(self._hstu_configs.item_embedding_feature_names),
                out_features=512,
            ),
            SwishLayerNorm(512),
            torch.nn.Linear(in_features=512, out_features=hstu_configs.hstu_transducer_embedding_dim),
            LayerNorm(hstu_configs.hstu_transducer_embedding_dim),
        ).apply(init_mlp_weights_optional_bias)

    def _construct_payload(
        self,
        payload_features: Dict[str, torch.Tensor],
        seq_embeddings: Dict[str, SequenceEmbedding],
    ) -> Dict[str, torch.Tensor]:
        contextual = list(self._hstu_configs.contextual_feature_to_max_length.keys())
        contextual_offsets = [asynchronous_complete_cumsum(seq_embeddings[x].lengths) for x in contextual]
        return {
            **payload_features,
            **{x: seq_embeddings[x].embedding for x in contextual},
            **{x + "_offsets": contextual_offsets[i] for i, x in enumerate(contextual)},
        }

    def _user_forward(
        self,
        max_uih_len: int,
        max_candidates: int,
        seq_embeddings: Dict[str, SequenceEmbedding],
        payload_features: Dict[str, torch.Tensor],
        num_candidates: torch.Tensor,
    ) -> torch.Tensor:
        source_lengths = seq_embeddings[self._hstu_configs.uih_post_id_feature_name].lengths
        source_timestamps = concat_2D_jagged(
            max_seq_len=max_uih_len + max_candidates,
            max_len_left=max_uih_len,
            offsets_left=payload_features["uih_offsets"],
            values_left=payload_features[self._hstu_configs.uih_action_time_feature_name].unsqueeze(-1),
            max_len_right=max_candidates,
            offsets_right=payload_features["candidate_offsets"],
            values_right=payload_features[self._hstu_configs.candidates_querytime_feature_name].unsqueeze(-1),
            kernel=self.hammer_kernel(),
        ).squeeze(-1)
        total_targets = int(num_candidates.sum().item())
        candidates_user_embeddings, _ = self._hstu_transducer(
            max_uih_len=max_uih_len,
            max_targets=max_candidates,
            total_uih_len=source_timestamps.numel() - total_targets,
            total_targets=total_targets,
            seq_embeddings=seq_embeddings[self._hstu_configs.uih_post_id_feature_name].embedding,
            seq_lengths=source_lengths,
            seq_timestamps=source_timestamps,
            seq_payloads=self._construct_payload(payload_features=payload_features, seq_embeddings=seq_embeddings),
            num_targets=num_candidates,
        )
        return candidates_user_embeddings

    def _item_forward(self, seq_embeddings: Dict[str, SequenceEmbedding]) -> torch.Tensor:  # [L, D]
        all_embeddings = [
            torch.cat([seq_embeddings[name].embedding for name in self._hstu_configs.item_embedding_feature_names], dim=-1)
        ]
        return self._item_embedding_mlp(torch.cat(all_embeddings, dim=-1))

    def preprocess(
        self,
        uih_features: Any,
        candidates_features: Any,
    ) -> Tuple[Dict[str, SequenceEmbedding], Dict[str, torch.Tensor], int, torch.Tensor, int, torch.Tensor]:
        # embedding lookup for uih and candidates
        merged_sparse_features = KeyedJaggedTensor.from_lengths_sync(
            keys=uih_features.keys() + candidates_features.keys(),
            values=torch.cat([uih_features.values(), candidates_features.values()], dim=0),
            lengths=torch.cat([uih_features.lengths(), candidates_features.lengths()], dim=0),
        )
        seq_embeddings_dict = self._embedding_collection(merged_sparse_features)
        num_candidates = candidates_features.lengths().view(len(candidates_features.keys()), -1)[0]
        max_num_candidates = int(num_candidates.max().item())
        uih_seq_lengths = uih_features[self._hstu_configs.uih_post_id_feature_name].lengths()
        max_uih_len = int(uih_seq_lengths.max().item())

        # prepare payload features
        payload_features: Dict[str, torch.Tensor] = {}
        for uih_feature_name, candidate_feature_name in self._hstu_configs.merge_uih_candidate_feature_mapping:
            if (candidate_feature_name not in self._hstu_configs.item_embedding_feature_names
                    and uih_feature_name not in self._hstu_configs.user_embedding_feature_names):
                values_left = uih_features[uih_feature_name].values()
                if self._is_inference and (
                    candidate_feature_name == self._hstu_configs.candidates_weight_feature_name
                    or candidate_feature_name == self._hstu_configs.candidates_watchtime_feature_name
                ):
                    total_candidates = int(torch.sum(num_candidates).item())
                    values_right = torch.zeros(total_candidates, dtype=torch.int64, device=values_left.device)
                else:
                    values_right = candidates_features[candidate_feature_name].values()
                payload_features[uih_feature_name] = values_left
                payload_features[candidate_feature_name] = values_right
        payload_features["uih_offsets"] = asynchronous_complete_cumsum(uih_seq_lengths)
        payload_features["candidate_offsets"] = asynchronous_complete_cumsum(num_candidates)

        seq_embeddings = {
            k: SequenceEmbedding(lengths=seq_embeddings_dict[k].lengths(), embedding=seq_embeddings_dict[k].values())
            for k in self._hstu_configs.user_embedding_feature_names + self._hstu_configs.item_embedding_feature_names
        }
        return seq_embeddings, payload_features, max_uih_len, uih_seq_lengths, max_num_candidates, num_candidates

    def main_forward(
        self,
        seq_embeddings: Dict[str, SequenceEmbedding],
        payload_features: Dict[str, torch.Tensor],
        max_uih_len: int,
        uih_seq_lengths: torch.Tensor,
        max_num_candidates: int,
        num_candidates: torch.Tensor,
    ) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor],
               Optional[torch.Tensor]]:
        # merge uih and candidates embeddings
        for uih_feature_name, candidate_feature_name in self._hstu_configs.merge_uih_candidate_feature_mapping:
            if uih_feature_name in seq_embeddings:
                seq_embeddings[uih_feature_name] = SequenceEmbedding(
                    lengths=uih_seq_lengths + num_candidates,
                    embedding=concat_2D_jagged(
                        max_seq_len=max_uih_len + max_num_candidates,
                        max_len_left=max_uih_len,
                        offsets_left=asynchronous_complete_cumsum(uih_seq_lengths),
                        values_left=seq_embeddings[uih_feature_name].embedding,
                        max_len_right=max_num_candidates,
                        offsets_right=asynchronous_complete_cumsum(num_candidates),
                        values_right=seq_embeddings[candidate_feature_name].embedding,
                        kernel=self.hammer_kernel(),
                    ),
                )

        with record_function("## item_forward ##"):
            candidates_item_embeddings = self._item_forward(seq_embeddings)
        with record_function("## user_forward ##"):
            candidates_user_embeddings = self._user_forward(
                max_uih_len=max_uih_len,
                max_candidates=max_num_candidates,
                seq_embeddings=seq_embeddings,
                payload_features=payload_features,
                num_candidates=num_candidates,
            )
        with record_function("## multitask_module ##"):
            supervision_labels, supervision_weights = _get_supervision_labels_and_weights(
                supervision_bitmasks=payload_features[self._hstu_configs.candidates_weight_feature_name],
                watchtime_sequence=payload_features[self._hstu_configs.candidates_watchtime_feature_name],
                task_configs=self._multitask_configs,
            )
            mt_target_preds, mt_target_labels, mt_target_weights, mt_losses = self._multitask_module(
                encoded_user_embeddings=candidates_user_embeddings,
                item_embeddings=candidates_item_embeddings,
                supervision_labels=supervision_labels,
                supervision_weights=supervision_weights,
            )

        aux_losses: Dict[str, torch.Tensor] = {}
        if not self._is_inference and self.training:
            for i, task in enumerate(self._multitask_configs):
                aux_losses[task.task_name] = mt_losses[i]

        return (
            candidates_user_embeddings,
            candidates_item_embeddings,
            aux_losses,
            mt_target_preds,
            mt_target_labels,
            mt_target_weights,
        )

    def forward(
        self,
        uih_features: Any,
        candidates_features: Any,
    ) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor],
               Optional[torch.Tensor]]:
        with record_function("## preprocess ##"):
            (seq_embeddings, payload_features, max_uih_len, uih_seq_lengths, max_num_candidates,
             num_candidates) = self.preprocess(uih_features=uih_features, candidates_features=candidates_features)

        with record_function("## main_forward ##"):
            return self.main_forward(
                seq_embeddings=seq_embeddings,
                payload_features=payload_features,
                max_uih_len=max_uih_len,
                uih_seq_lengths=uih_seq_lengths,
                max_num_candidates=max_num_candidates,
                num_candidates=num_candidates,
            )
