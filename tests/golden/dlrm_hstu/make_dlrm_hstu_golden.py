#!/usr/bin/env python3
"""Mint the fixtures of ``TimestampLayerNormPostprocessor`` (tests/golden/timestamp_ln/) and of ``DlrmHSTU``
(tests/golden/dlrm_hstu/) from the REFERENCE's modules (PyTorch path, CPU).

Run in the build container only (needs /root/reference):

    python tests/golden/dlrm_hstu/make_dlrm_hstu_golden.py [--out DIR] [--op-out DIR]

``generative_recommenders.modules.{postprocessors,dlrm_hstu}`` are imported unmodified: ``_fbgemm_shim`` stands in for the
absent fbgemm ops, a ``libfb.py.pyre.none_throws`` stand-in is planted as in ``make_preprocessor_golden.py``, and stand-ins
for ``torchrec``, ``torchrec.modules.embedding_configs`` and ``torchrec.modules.embedding_modules`` (a ``KeyedJaggedTensor``
of keys / values / lengths, an ``EmbeddingConfig`` dataclass and an ``EmbeddingCollection`` that holds one
``torch.nn.Embedding`` per table in a ModuleDict named ``embeddings``, TorchRec's state-dict layout) are planted in
``sys.modules``: torchrec is not installed.

Every case runs on the SAME values in fp32, in bf16 and in fp64, the truth -- inputs and parameters are rounded to
bf16-representable numbers first, so only the arithmetic differs.  In ALL three runs ``_period_units`` /
``_units_per_period`` and the time-feature arithmetic stay fp32 (``.double()`` would move timestamps into other buckets,
``.to(bfloat16)`` turns 86400 into 86528); in the bf16 run the concatenated row is cast to bf16 in front of the Linear, as
autocast would.  As in the other makers the reference's LayerNorm / SwishLayerNorm, whose PyTorch path casts to fp32 whatever
comes in, compute the same formula in the dtype of their input in the fp64 run.  Gradients are of ``(out * r).sum()`` (op)
and of the summed losses (model).  16-bit values are stored as bf16 bit patterns; only arrays and names are stored.

The maker asserts that plain ``floorf(a / b)`` and exact integer arithmetic each put at least one timestamp of every case
with period 3600 into another bucket than the reference does: the fixtures catch both obvious kernels."""

import argparse
import dataclasses
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import _fbgemm_shim  # noqa: F401  (registers torch.ops.fbgemm.*)

_pyre = types.ModuleType("libfb.py.pyre")


def _none_throws(x):
    assert x is not None
    return x


_pyre.none_throws = _none_throws
for _name in ("libfb", "libfb.py"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["libfb.py.pyre"] = _pyre


# ------------------------------------------------------------------------------------------------------ torchrec stand-ins
class KeyedJaggedTensor:
    """keys, concatenated values and per-(key, user) lengths: what DlrmHSTU.preprocess touches"""

    def __init__(self, keys, values, lengths):
        self._keys, self._values, self._lengths = list(keys), values, lengths

    @staticmethod
    def from_lengths_sync(keys, values, lengths):
        return KeyedJaggedTensor(keys, values, lengths)

    def keys(self):
        return self._keys

    def values(self):
        return self._values

    def lengths(self):
        return self._lengths

    def __getitem__(self, key):
        k = self._keys.index(key)
        per_key = self._lengths.view(len(self._keys), -1)
        start = int(per_key[:k].sum())
        return _Jagged(self._values[start:start + int(per_key[k].sum())], per_key[k])


class _Jagged:
    def __init__(self, values, lengths):
        self._values, self._lengths = values, lengths

    def values(self):
        return self._values

    def lengths(self):
        return self._lengths


@dataclasses.dataclass
class EmbeddingConfig:
    num_embeddings: int
    embedding_dim: int
    name: str = ""
    feature_names: list = dataclasses.field(default_factory=list)
    data_type: object = None
    weight_init_max: float = None
    weight_init_min: float = None


class EmbeddingCollection(torch.nn.Module):
    def __init__(self, tables, need_indices=False, device=None):
        super().__init__()
        del need_indices, device        # (the reference asks for the meta device: the fixtures need real weights)
        self.embeddings = torch.nn.ModuleDict({t.name: torch.nn.Embedding(t.num_embeddings, t.embedding_dim) for t in tables})
        self._feature_to_table = {f: t.name for t in tables for f in t.feature_names}

    def forward(self, features):
        return {k: _Jagged(self.embeddings[self._feature_to_table[k]](features[k].values()), features[k].lengths())
                for k in features.keys() if k in self._feature_to_table}


_torchrec = types.ModuleType("torchrec")
_torchrec.KeyedJaggedTensor = KeyedJaggedTensor
_torchrec_modules = types.ModuleType("torchrec.modules")
_torchrec_configs = types.ModuleType("torchrec.modules.embedding_configs")
_torchrec_configs.EmbeddingConfig = EmbeddingConfig
_torchrec_embmods = types.ModuleType("torchrec.modules.embedding_modules")
_torchrec_embmods.EmbeddingCollection = EmbeddingCollection
sys.modules["torchrec"] = _torchrec
sys.modules["torchrec.modules"] = _torchrec_modules
sys.modules["torchrec.modules.embedding_configs"] = _torchrec_configs
sys.modules["torchrec.modules.embedding_modules"] = _torchrec_embmods

from generative_recommenders.common import HammerKernel, set_dev_mode  # noqa: E402
from generative_recommenders.modules.dlrm_hstu import DlrmHSTU, DlrmHSTUConfig  # noqa: E402
from generative_recommenders.modules.multitask_module import MultitaskTaskType, TaskConfig  # noqa: E402
from generative_recommenders.modules.postprocessors import TimestampLayerNormPostprocessor  # noqa: E402
from generative_recommenders.ops.layer_norm import LayerNorm, SwishLayerNorm  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
HOUR_DAY, DAY_WEEK, DAY_YEAR, MIN_HOUR = (3600, 24), (86400, 7), (86400, 365), (60, 60)

# name -> (rows, dim, periods, dtypes)
OP_CASES = {
    "1_vec_23x40": (23, 40, [HOUR_DAY, DAY_WEEK], ("f32", "bf16", "f64")),
    "2_scalar_11x37": (11, 37, [HOUR_DAY], ("f32", "bf16", "f64")),
    "3_k512_70x512": (70, 512, [HOUR_DAY, DAY_WEEK], ("bf16", "f64")),
    "4_wide_9x1536": (9, 1536, [HOUR_DAY, DAY_WEEK, DAY_YEAR], ("bf16", "f64")),
    "5_periods_5x64": (5, 64, [HOUR_DAY, DAY_WEEK, DAY_YEAR, MIN_HOUR], ("f32", "f64")),
    "6_row_1x40": (1, 40, [HOUR_DAY, DAY_WEEK], ("f32", "bf16", "f64")),
}


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def store(t, as_bf16=False):
    t = t.detach().contiguous()
    if as_bf16 or t.dtype == torch.bfloat16:
        return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def truth_norms(module):
    """fp64 run: LayerNorm / SwishLayerNorm in the dtype of their input (the reference's PyTorch path drops to fp32)"""
    for m in module.modules():
        if isinstance(m, SwishLayerNorm):
            m.forward = lambda x, m=m: x * torch.sigmoid(
                torch.nn.functional.layer_norm(x, m._normalized_shape, m.weight, m.bias, m._eps))
        elif isinstance(m, LayerNorm):
            m.forward = lambda x, m=m: torch.nn.functional.layer_norm(x, m._normalized_shape, m.weight, m.bias, m._eps)


def rounded_state_dict(module, g, skip=()):
    """every float parameter moved off its default (zero biases, (1, 0) norms) and rounded to bf16-representable values;
    the buffers named in ``skip`` stay as they are"""
    sd = {}
    for k, v in module.state_dict().items():
        if v.is_floating_point() and not k.endswith(skip):
            sd[k] = bf16_round(v + 0.1 * torch.randn(v.shape, generator=g))
        else:
            sd[k] = v.clone()
    return sd


def check_differs(name, res, keys, exact_ok=()):
    for tag in ("f32", "bf16"):
        if tag not in res:
            continue
        for k in keys:
            if (tag, k) in exact_ok:
                continue
            truth = res["f64"][k].detach().double()
            err = float((res[tag][k].detach().double() - truth).norm() / truth.norm())
            assert err > 0.0, f"{name}: {tag}:{k} equals the fp64 truth exactly: a relative gate on it would be vacuous"


TIME_BUFFERS = ("_period_units", "_units_per_period")


def to_dtype_keeping_time_fp32(module, dt):
    """module.to(dt) with every postprocessor's two time buffers restored to their fp32 values, and the concatenated row
    cast to the Linear's dtype in front of it"""
    posts = [m for m in module.modules() if isinstance(m, TimestampLayerNormPostprocessor)]
    saved = [(m._period_units.clone(), m._units_per_period.clone()) for m in posts]
    module = module.to(dt)
    for m, (pu, upp) in zip(posts, saved):
        m._period_units, m._units_per_period = pu, upp
        inner = m._concat_time_features
        m._concat_time_features = lambda emb, timestamps, inner=inner, m=m: inner(emb, timestamps=timestamps).to(
            m._time_feature_combiner.weight.dtype)
    return module


# ------------------------------------------------------------------------------------------------------ timestamps
def buckets_f32(t, period):
    """the reference's own expression (postprocessors.py:145-147) on fp32"""
    return torch.div(t.unsqueeze(-1), torch.tensor([[float(period)]]), rounding_mode="floor").squeeze(-1)


def _both_wrong(t):
    """does plain floorf(a / b) AND does integer arithmetic disagree with the reference's hour bucket of t?"""
    ref = float(buckets_f32(torch.tensor([t]), 3600)[0])
    a = np.float32(t)
    return float(np.floor(a / np.float32(3600))) != ref and float(t // 3600) != ref


def timestamp_pool(g):
    k0 = 472000
    both = next(t for k in range(k0, k0 + 64) for t in range(k * 3600, k * 3600 + 64) if _both_wrong(t))
    pool = [both, 2**33 + 12345, 0]
    draws = torch.randint(1_600_000_000, 1_760_000_000, (80,), generator=g).tolist()
    pool += [draws.pop(), 3600, 1, 3599]
    for k in (k0, k0 + 1, k0 + 222):
        pool += [k * 3600 - 1, k * 3600, k * 3600 + 1, k * 3600 - 64, k * 3600 + 64]
    return pool + draws


def assert_catches_obvious_kernels(name, t, periods):
    if 3600 not in [p for p, _ in periods]:
        return
    ref = buckets_f32(t, 3600).numpy()
    plain = np.floor(t.numpy().astype(np.float32) / np.float32(3600))
    exact = (t.numpy() // 3600).astype(np.float64)
    assert (plain != ref).any(), f"{name}: floorf(a / b) reproduces every stored bucket"
    assert (exact != ref).any(), f"{name}: integer arithmetic reproduces every stored bucket"


# ------------------------------------------------------------------------------------------------------ the op
COMBINER_W = "_time_feature_combiner.weight"
FACTOR_RANK, SAMPLED_ROWS = 8, 8


def factored_weight(a, b):
    """W = A B in fp64 (exact: eight products of 8-bit mantissas), rounded to fp32 and then to bf16-representable values"""
    return bf16_round((a.double() @ b.double()).float())


def op_case(name, seed):
    rows, dim, periods, tags = OP_CASES[name]
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    t = torch.tensor(timestamp_pool(g)[:rows], dtype=torch.int64)
    assert_catches_obvious_kernels(name, t, periods)
    x = bf16_round(torch.randn(rows, dim, generator=g))
    r = torch.randn(rows, dim, generator=g)
    proto = TimestampLayerNormPostprocessor(embedding_dim=dim, time_duration_features=periods, eps=1e-5)
    sd = rounded_state_dict(proto, g, skip=TIME_BUFFERS)
    pu, upp = proto._period_units, proto._units_per_period
    units = torch.div(t.unsqueeze(-1), pu, rounding_mode="floor")
    angles = (torch.remainder(units, upp) / upp) * 2 * 3.14
    tf = proto._concat_time_features(torch.zeros(rows, 0), timestamps=t)
    assert tf.dtype == torch.float32 and units.dtype == torch.float32
    # (torch.polar's cos / sin and torch.cos / torch.sin may differ in the last bit: the stored features are polar's)
    assert torch.allclose(tf, torch.stack([torch.cos(angles), torch.sin(angles)], -1).flatten(-2, -1), rtol=0, atol=1e-6)
    z = dict(x=store(x, True), timestamps=t.numpy(), r=store(r), periods=np.array(periods, dtype=np.int64), eps=np.float64(1e-5),
             units=units.numpy(), angles=angles.numpy(), time_features=tf.numpy(), sd_keys=np.array(list(sd)),
             param_keys=np.array([k for k, _ in proto.named_parameters()]), tags=np.array(tags))
    # A (D, D + 2F) weight and its gradient pass the size limit of a committed file from D = 512 on: there the weight is the
    # product of two stored factors and its gradient is stored on SAMPLED_ROWS rows and on the 2F time columns
    w_rows = torch.arange(dim)
    if dim > 64:
        fa = bf16_round(torch.randn(dim, FACTOR_RANK, generator=g) * (2.0 / (dim * FACTOR_RANK)) ** 0.25)
        fb = bf16_round(torch.randn(FACTOR_RANK, dim + 2 * len(periods), generator=g) * (2.0 / (dim * FACTOR_RANK)) ** 0.25)
        sd[COMBINER_W] = factored_weight(fa, fb)
        z["factor_a"], z["factor_b"] = store(fa, True), store(fb, True)
        w_rows = torch.cat([torch.tensor([0, dim - 1]), torch.randperm(dim - 2, generator=g)[:SAMPLED_ROWS - 2] + 1]).sort().values
    z["w_rows"] = w_rows.numpy()
    for k, v in sd.items():
        if k == COMBINER_W and dim > 64:
            continue
        z["sd:" + k] = store(v, v.is_floating_point() and not k.endswith(TIME_BUFFERS))
    res = {}
    for tag in tags:
        dt = DTYPES[tag]
        m = TimestampLayerNormPostprocessor(embedding_dim=dim, time_duration_features=periods, eps=1e-5)
        m.load_state_dict(sd, strict=True)
        m = to_dtype_keeping_time_fp32(m, dt)
        xi = x.clone().to(dt).requires_grad_()
        out = m(seq_embeddings=xi, seq_timestamps=t, seq_payloads={})
        assert out.dtype == dt
        (out * r.to(dt)).sum().backward()
        d = {"out": out, "g:x": xi.grad}
        for k, p in m.named_parameters():
            if k == COMBINER_W:
                d[f"gp:{k}@rows"], d[f"gp:{k}@time"] = p.grad[w_rows], p.grad[:, dim:]
            else:
                d["gp:" + k] = p.grad
        res[tag] = d
    # one row: d ln_bias is r itself, in fp32 exactly as in fp64 (the gate then asks the kernel for the exact value too)
    check_differs(name, res, list(res["f64"]), exact_ok={("f32", "gp:_layer_norm.bias")} if rows == 1 else ())
    for tag, d in res.items():
        for k, v in d.items():
            z[f"{tag}:{k}"] = store(v)
    return z


# ------------------------------------------------------------------------------------------------------ the model
UIH_LENGTHS, CANDIDATES = [7, 1, 4, 3, 9, 5], [2, 1, 1, 3, 1, 0]      # the last user has no candidate
TABLE_DIM, TRANSDUCER_DIM, ITEMS, USERS = 16, 32, 50, 20
UIH_KEYS = ["user_id", "uih_item_id", "uih_action_time", "uih_weight", "uih_watchtime"]
CANDIDATE_KEYS = ["cand_item_id", "cand_query_time", "cand_weight", "cand_watchtime"]
TASKS = [("is_click", 1, 0), ("is_like", 2, 0), ("vvp", 4, 1)]       # (name, weight, MultitaskTaskType)


def model_config():
    return DlrmHSTUConfig(
        max_seq_len=32, hstu_num_heads=2, hstu_attn_linear_dim=16, hstu_attn_qk_dim=8, hstu_attn_num_layers=2,
        hstu_embedding_table_dim=TABLE_DIM, hstu_transducer_embedding_dim=TRANSDUCER_DIM, hstu_input_dropout_ratio=0.0,
        hstu_linear_dropout_rate=0.0, contextual_feature_to_max_length={"user_id": 1},
        contextual_feature_to_min_uih_length={"user_id": 2}, candidates_weight_feature_name="cand_weight",
        candidates_watchtime_feature_name="cand_watchtime", candidates_querytime_feature_name="cand_query_time",
        multitask_configs=[TaskConfig(task_name=n, task_weight=w, task_type=MultitaskTaskType(t)) for n, w, t in TASKS],
        user_embedding_feature_names=["uih_item_id", "user_id"], item_embedding_feature_names=["cand_item_id"],
        uih_post_id_feature_name="uih_item_id", uih_action_time_feature_name="uih_action_time",
        uih_weight_feature_name="uih_weight", hstu_uih_feature_names=list(UIH_KEYS),
        hstu_candidate_feature_names=list(CANDIDATE_KEYS),
        merge_uih_candidate_feature_mapping=[("uih_item_id", "cand_item_id"), ("uih_action_time", "cand_query_time"),
                                             ("uih_weight", "cand_weight"), ("uih_watchtime", "cand_watchtime")],
        action_weights=[1, 2, 4])


def model_tables():
    return {"item_id": EmbeddingConfig(num_embeddings=ITEMS, embedding_dim=TABLE_DIM, name="item_id",
                                       feature_names=["uih_item_id", "cand_item_id"]),
            "user_id": EmbeddingConfig(num_embeddings=USERS, embedding_dim=TABLE_DIM, name="user_id", feature_names=["user_id"])}


def model_features(g):
    """values per key (key-major, users inside a key) and the (keys * users) lengths of the two feature containers"""
    n_uih, n_cand, B = sum(UIH_LENGTHS), sum(CANDIDATES), len(UIH_LENGTHS)
    start = torch.randint(1_600_000_000, 1_700_000_000, (B,), generator=g)
    times, query = [], []
    for b, (n, c) in enumerate(zip(UIH_LENGTHS, CANDIDATES)):
        steps = torch.randint(30, 200_000, (n + c,), generator=g).cumsum(0) + start[b]
        times.append(steps[:n])
        query.append(steps[n:])
    uih = {"user_id": torch.randint(0, USERS, (B,), generator=g), "uih_item_id": torch.randint(0, ITEMS, (n_uih,), generator=g),
           "uih_action_time": torch.cat(times), "uih_weight": torch.randint(0, 8, (n_uih,), generator=g),
           "uih_watchtime": torch.randint(0, 4, (n_uih,), generator=g)}
    cand = {"cand_item_id": torch.randint(0, ITEMS, (n_cand,), generator=g), "cand_query_time": torch.cat(query),
            "cand_weight": torch.randint(0, 8, (n_cand,), generator=g), "cand_watchtime": torch.randint(0, 4, (n_cand,), generator=g)}
    uih_lengths = torch.tensor([1] * B + UIH_LENGTHS * 4)
    cand_lengths = torch.tensor(CANDIDATES * 4)
    return (torch.cat([uih[k] for k in UIH_KEYS]), uih_lengths, torch.cat([cand[k] for k in CANDIDATE_KEYS]), cand_lengths)


def build_model(sd, dt, is_inference):
    m = DlrmHSTU(hstu_configs=model_config(), embedding_tables=model_tables(), is_inference=is_inference)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    m.set_hammer_kernel(HammerKernel.PYTORCH)
    m = to_dtype_keeping_time_fp32(m, dt)
    m.set_training_dtype(dt)
    if dt == torch.float64:
        truth_norms(m)
    m.train(not is_inference)
    return m


RETURNED = ("user_embeddings", "item_embeddings", "preds", "labels", "weights")


def model_case(seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    uih_values, uih_lengths, cand_values, cand_lengths = model_features(g)
    proto = DlrmHSTU(hstu_configs=model_config(), embedding_tables=model_tables(), is_inference=False)
    sd = rounded_state_dict(proto, g, skip=TIME_BUFFERS)
    # the position table has 8192 rows whatever the config; the rows no sequence of this case reaches are zeroed so that the
    # fixture stays within the size limit of a committed file
    pos = [k for k in sd if k.endswith("_position_embeddings_weight")]
    assert len(pos) == 1
    sd[pos[0]][64:] = 0.0
    z = dict(uih_keys=np.array(UIH_KEYS), candidate_keys=np.array(CANDIDATE_KEYS), uih_values=uih_values.numpy(),
             uih_lengths=uih_lengths.numpy(), candidate_values=cand_values.numpy(), candidate_lengths=cand_lengths.numpy(),
             sd_keys=np.array(list(sd)), param_keys=np.array([k for k, _ in proto.named_parameters()]),
             task_names=np.array([n for n, _, _ in TASKS]))
    for k, v in sd.items():
        z["sd:" + k] = store(v, v.is_floating_point() and not k.endswith(TIME_BUFFERS))
    res = {}
    for tag, dt in DTYPES.items():
        for is_inference in (False, True):
            if is_inference and tag == "bf16":
                continue
            m = build_model(sd, dt, is_inference)
            uih = KeyedJaggedTensor(UIH_KEYS, uih_values, uih_lengths)
            cand = KeyedJaggedTensor(CANDIDATE_KEYS, cand_values, cand_lengths)
            with torch.set_grad_enabled(not is_inference):
                out = m(uih_features=uih, candidates_features=cand)
            user, item, aux, preds, labels, weights = out
            if is_inference:
                assert aux == {} and labels is None and weights is None
                res[tag + "_infer"] = dict(user_embeddings=user, item_embeddings=item, preds=preds)
                continue
            d = dict(zip(RETURNED, (user, item, preds, labels, weights)))
            d["losses"] = torch.stack([aux[n] for n, _, _ in TASKS])
            sum(aux.values()).backward()
            for k, p in m.named_parameters():
                d["gp:" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
            res[tag] = d
    gated = [k for k in res["f64"] if k not in ("labels", "weights") and float(res["f64"][k].detach().double().norm()) > 0.0]
    z["gated"] = np.array(gated)
    check_differs("model", res, gated)
    # one file for the inputs and parameters and one per run: every committed file stays under the size limit
    files = {"model_small": z}
    for tag, d in res.items():
        files["model_small_" + tag] = {k: store(v) for k, v in d.items()}
    return files


def reference_names():
    cfg = DlrmHSTUConfig()
    fields = dataclasses.fields(DlrmHSTUConfig)
    m = DlrmHSTU(hstu_configs=model_config(), embedding_tables=model_tables(), is_inference=False)
    import inspect
    return dict(state_dict_keys=np.array(list(m.state_dict())), config_fields=np.array([f.name for f in fields]),
                config_defaults=np.array([repr(getattr(cfg, f.name)) for f in fields]),
                init_args=np.array(list(inspect.signature(DlrmHSTU.__init__).parameters)),
                methods=np.array([f"{n}({', '.join(inspect.signature(getattr(DlrmHSTU, n)).parameters)})" for n in
                                  ("_construct_payload", "_user_forward", "_item_forward", "preprocess", "main_forward", "forward")]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--op-out", default=os.path.join(os.path.dirname(HERE), "timestamp_ln"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    os.makedirs(args.op_out, exist_ok=True)
    set_dev_mode(True)
    torch.set_num_threads(1)   # one summation order whatever the host
    for n, name in enumerate(OP_CASES):
        np.savez_compressed(os.path.join(args.op_out, f"case_{name}.npz"), **op_case(name, 900 + n))
    for name, arrays in model_case(950).items():
        np.savez_compressed(os.path.join(args.out, name + ".npz"), **arrays)
    np.savez_compressed(os.path.join(args.out, "reference_names.npz"), **reference_names())


if __name__ == "__main__":
    main()
