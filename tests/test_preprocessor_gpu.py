"""The input preprocessors on the GPU.

* Both fused ops against the numpy restatement (tests/preprocessor_ref.py, itself pinned to the reference's fixtures by
  tests/test_preprocessor_host.py): forward and the combine backward bit for bit -- fp32 / bf16 / fp16, int32 / int64 offsets,
  the three combine modes, with and without contextual rows and action rows, row widths on the 16-byte path and off it,
  users with L = 0, T = 0, U = 0 and T = L, one user, no user.
* The action-encode backward against the fp64 sum of the same d_out under the bound of an fp32 sum in ANY order,
  |err| <= n * 2^-24 * sum |terms|, and bit-identical across two calls.
* The modules against the fixtures minted from the reference: what is a copy or an integer must be equal, float outputs and
  gradients are gated as tests/multitask_ref.gate_multiplier defines (e_hip <= m * e_ref against the fp64 truth; the ratios
  are printed); the reference's state_dict loads with strict=True.
* HSTUTransducer against the hand-written composition of its parts, bit for bit."""

import os

import numpy as np
import pytest
import torch

import preprocessor_ref as R
from multitask_ref import gate_multiplier, rel_fro

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ["float32", "bfloat16", "float16"]
# users with L = 0 (1), T = 0 (2, 6), U = 0 and T = L (3, 8), one row (3, 7); 17 users, N <= 40
LENGTHS = [7, 0, 4, 3, 9, 40, 12, 1, 5, 2, 31, 8, 16, 6, 23, 11, 3]
TARGETS = [2, 0, 0, 3, 1, 7, 0, 0, 5, 1, 4, 8, 3, 2, 9, 1, 1]
BATCHES = [(LENGTHS, TARGETS), ([5], [2]), ([], [])]


def bits(t):
    """a float tensor as the numpy array of its bit patterns"""
    t = t.detach().contiguous().cpu()
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int32).numpy().view(np.uint32)


def same_bits(t, ref_bits):
    t = t.detach().contiguous().cpu()
    it = torch.int16 if t.element_size() == 2 else torch.int32
    want = torch.from_numpy(np.ascontiguousarray(ref_bits).view(np.int16 if t.element_size() == 2 else np.int32))
    return t.shape == want.shape and torch.equal(t.view(it), want)


def dev_i(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dtype).to(DEV)


# ------------------------------------------------------------------------------------------------------ action encode
# (action weights, [(threshold, weight)], Da): T * Da = 15 (elements), 40 (16-byte rows), 256 (the DLRM-v3 width)
ACTION_CASES = [([2], [(10, 1), (50, 4)], 5), ([1, 2, 4, 8], [(30, 16)], 8), ([1, 2, 4, 8, 16, 32, 64, 128], [], 32)]


def _action_inputs(case, lengths, targets, seed):
    weights, thresholds, da = case
    combined = weights + [w for _, w in thresholds]
    g = torch.Generator().manual_seed(seed)
    uih = [l - t for l, t in zip(lengths, targets)]
    n = sum(uih)
    actions = torch.randint(0, 2 * max(combined), (n,), generator=g)
    watch = torch.randint(0, 100, (n,), generator=g)
    if thresholds and n > 1:
        watch[0], watch[1] = thresholds[0][0], thresholds[0][0] - 1          # ">=": at the threshold and just below it
    table = torch.randn(len(combined), da, generator=g)
    target = torch.randn(1, len(combined) * da, generator=g)
    return combined, thresholds, da, uih, actions, watch, table, target


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_action_encode_forward_equals_the_restatement(dtype):
    from generative_recommenders_amd.ops.preprocess import action_encode

    for ci, case in enumerate(ACTION_CASES):
        for bi, (lengths, targets) in enumerate(BATCHES):
            for idt in (torch.int32, torch.int64):
                combined, thresholds, da, uih, actions, watch, table, target = _action_inputs(case, lengths, targets, 10 * ci + bi)
                uo, to = R.offsets_of(uih), R.offsets_of(targets)
                out = action_encode(actions.to(DEV), watch.to(DEV), dev_i(uo, idt), dev_i(to, idt), table.to(DEV), target.to(DEV),
                                    combined[:len(case[0])] + [w for _, w in thresholds], thresholds, sum(uih), sum(targets), dtype)
                want = R.action_encode(actions.numpy(), watch.numpy(), uo, to, bits(table.to(dtype)), bits(target.to(dtype)),
                                       combined, thresholds)
                assert out.dtype == dtype and same_bits(out, want), f"case {ci} batch {bi} {idt}"


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_action_encode_backward_bound_and_determinism(dtype):
    from generative_recommenders_amd.ops import _launch

    for ci, case in enumerate(ACTION_CASES):
        for bi, (lengths, targets) in enumerate(BATCHES[:2]):
            combined, thresholds, da, uih, actions, watch, _, _ = _action_inputs(case, lengths, targets, 50 + 10 * ci + bi)
            uo, to = R.offsets_of(uih), R.offsets_of(targets)
            g = torch.Generator().manual_seed(ci)
            d_out = torch.randn(sum(lengths), len(combined) * da, generator=g).to(dtype)
            args = (d_out.to(DEV), actions.to(DEV), watch.to(DEV), dev_i(uo), dev_i(to), combined, thresholds, sum(uih),
                    sum(targets), da)
            d_table, d_target = _launch.action_encode_bwd(*args)
            again = _launch.action_encode_bwd(*args)
            assert torch.equal(d_table, again[0]) and torch.equal(d_target, again[1]), "two calls differ"
            ref = R.action_encode_bwd(d_out.double().numpy(), actions.numpy(), watch.numpy(), uo, to, combined, thresholds, da)
            for name, got in (("table", d_table), ("target", d_target)):
                err = np.abs(got.double().cpu().numpy().reshape(ref["d_" + name].shape) - ref["d_" + name])
                bound = ref["n_" + name] * 2.0**-24 * ref["abs_" + name]
                print(f"action bwd case {ci} batch {bi} {name}: max err {err.max():.3e}, max bound {bound.max():.3e}")
                assert (err <= bound).all(), f"case {ci} batch {bi} d_{name}: {float((err - bound).max()):.3e} over the bound"


def test_action_encode_gradients_reach_the_tables():
    from generative_recommenders_amd.ops.preprocess import action_encode

    combined, thresholds, da, uih, actions, watch, table, target = _action_inputs(ACTION_CASES[1], LENGTHS, TARGETS, 3)
    table, target = table.to(DEV).requires_grad_(), target.to(DEV).requires_grad_()
    out = action_encode(actions.to(DEV), watch.to(DEV), dev_i(R.offsets_of(uih)), dev_i(R.offsets_of(TARGETS)), table, target,
                        combined, thresholds, sum(uih), sum(TARGETS), torch.bfloat16)
    r = torch.randn(out.shape, device=DEV).bfloat16()
    (out * r).sum().backward()
    from generative_recommenders_amd.ops import _launch

    # autograd hands the tables exactly what the backward launcher returns for d_out = r
    d_table, d_target = _launch.action_encode_bwd(r, actions.to(DEV), watch.to(DEV), dev_i(R.offsets_of(uih)),
                                                  dev_i(R.offsets_of(TARGETS)), combined, thresholds, sum(uih), sum(TARGETS), da)
    assert table.grad.shape == table.shape and target.grad.shape == target.shape
    assert torch.equal(table.grad, d_table) and torch.equal(target.grad, d_target) and bool(table.grad.abs().sum() > 0)


# ------------------------------------------------------------------------------------------------------ combine
@pytest.mark.parametrize("mode", [R.SUM, R.INTERLEAVE_ALL, R.INTERLEAVE_UIH], ids=["sum", "interleave_all", "interleave_uih"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_combine_forward_and_backward_equal_the_restatement(dtype, mode):
    from generative_recommenders_amd.ops.preprocess import combine_embeddings

    n = 0
    for D in (24, 23, 512):
        for C in (0, 3):
            for has_action in ((True, False) if mode == R.SUM else (True,)):
                for bi, (lengths, targets) in enumerate(BATCHES):
                    idt = torch.int32 if (n := n + 1) % 2 else torch.int64
                    g = torch.Generator().manual_seed(n)
                    B, total = len(lengths), sum(lengths)
                    content = torch.randn(total, D, generator=g).to(dtype)
                    action = torch.randn(total, D, generator=g).to(dtype) if has_action else None
                    ctx = torch.randn(B, C, D, generator=g).to(dtype) if C else None
                    ts = torch.randint(1, 10**9, (total,), generator=g)
                    cd = content.to(DEV).requires_grad_()
                    ad = action.to(DEV).requires_grad_() if has_action else None
                    xd = ctx.to(DEV).requires_grad_() if C else None
                    sl = dev_i(lengths, idt)
                    out, out_ts, out_len, out_off = combine_embeddings(
                        cd, ad, xd, ts.to(DEV), sl, dev_i(R.offsets_of(lengths), idt), dev_i(targets, idt), total - sum(targets),
                        sum(targets), mode)
                    what = f"D {D} C {C} action {has_action} batch {bi} {idt}"
                    summed = bits(content + action) if (mode == R.SUM and has_action) else None
                    want, want_ts, want_len = R.combine(bits(content), bits(action) if has_action else None,
                                                        bits(ctx) if C else None, ts.numpy(), lengths, targets, mode, summed)
                    assert out.dtype == dtype and same_bits(out, want), what
                    assert out_ts.dtype == torch.int64 and np.array_equal(out_ts.cpu().numpy(), want_ts), what
                    assert np.array_equal(out_len.cpu().numpy(), want_len) and np.array_equal(out_off.cpu().numpy(), R.offsets_of(want_len)), what
                    d_out = torch.randn(out.shape, generator=g).to(dtype)
                    out.backward(d_out.to(DEV))
                    dc, da, dx = R.combine_bwd(bits(d_out), lengths, targets, C, mode, has_action)
                    assert same_bits(cd.grad, dc), what
                    if has_action:
                        assert same_bits(ad.grad, da), what
                    if C:
                        assert same_bits(xd.grad, dx), what


def test_combine_on_a_misaligned_base_takes_the_element_path():
    """rows of 16-byte multiples whose base pointer is not 16-byte aligned: same result as the aligned call"""
    from generative_recommenders_amd.ops import _launch

    lengths, targets = LENGTHS, TARGETS
    total, D = sum(lengths), 24
    g = torch.Generator().manual_seed(1)
    flat = torch.randn(total * D + 1, generator=g).bfloat16().to(DEV)
    content = flat[1:].view(total, D)
    assert content.data_ptr() % 16 != 0 and content.is_contiguous()
    action = torch.randn(total, D, generator=g).bfloat16().to(DEV)
    ts = torch.arange(total, device=DEV)
    so, nt = dev_i(R.offsets_of(lengths)), dev_i(targets)
    oo = dev_i(R.offsets_of(R.out_lengths(lengths, targets, 0, R.INTERLEAVE_UIH)))
    a = _launch.combine_embeddings_fwd(content, action, None, ts, so, nt, oo, R.INTERLEAVE_UIH, total - sum(targets), sum(targets))
    b = _launch.combine_embeddings_fwd(content.clone(), action, None, ts, so, nt, oo, R.INTERLEAVE_UIH, total - sum(targets),
                                       sum(targets))
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])


def test_error_paths_raise_runtime_error():
    from generative_recommenders_amd.ops.preprocess import COMBINE_INTERLEAVE_ALL, COMBINE_SUM, action_encode, combine_embeddings

    off, lens, nt = dev_i([0, 2, 5]), dev_i([2, 3]), dev_i([1, 1])
    x = torch.zeros(5, 8, device=DEV, dtype=torch.bfloat16)
    ts = torch.zeros(5, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="GPU"):
        combine_embeddings(x.cpu(), None, None, ts, lens, off, nt, 3, 2, COMBINE_SUM)
    with pytest.raises(RuntimeError, match="content_embeddings"):
        combine_embeddings(x, x.float(), None, ts, lens, off, nt, 3, 2, COMBINE_SUM)
    with pytest.raises(RuntimeError, match="int64"):
        combine_embeddings(x, x, None, ts.int(), lens, off, nt, 3, 2, COMBINE_SUM)
    with pytest.raises(RuntimeError, match="action_embeddings"):
        combine_embeddings(x, None, None, ts, lens, off, nt, 3, 2, COMBINE_INTERLEAVE_ALL)
    with pytest.raises(RuntimeError, match="do not fit"):
        combine_embeddings(x, x, None, ts, lens, off, nt, 3, 3, COMBINE_SUM)
    table, target = torch.zeros(2, 4, device=DEV), torch.zeros(1, 8, device=DEV)
    with pytest.raises(RuntimeError, match="GPU"):
        action_encode(torch.zeros(3, dtype=torch.int64), None, off, off, table, target, [1, 2], [], 3, 2)
    with pytest.raises(RuntimeError, match="int64"):
        action_encode(torch.zeros(3, dtype=torch.int32, device=DEV), None, off, off, table, target, [1, 2], [], 3, 2)
    with pytest.raises(RuntimeError, match="action types"):
        action_encode(torch.zeros(3, dtype=torch.int64, device=DEV), None, off, off, torch.zeros(65, 4, device=DEV),
                      torch.zeros(1, 260, device=DEV), list(range(1, 66)), [], 3, 2)


# ------------------------------------------------------------------------------------------------------ modules vs fixtures
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_NAME = {"f32": "float32", "bf16": "bfloat16"}
# the configuration of tests/golden/preprocessor/make_preprocessor_golden.py
D_IN, D_OUT, HIDDEN = 16, 24, 8
CONTEXTUAL, MIN_UIH = {"c0": 1, "c1": 2}, {"c1": 4}
ADDITIONAL, ENRICH = {"a0": 8}, {"t0": 8}
ACTION_WEIGHTS, ACTION_THRESHOLDS, ACTION_DIM = [1, 2, 4], [(30, 8)], 8


def _state_dict(c):
    return {str(k): torch.from_numpy(np.ascontiguousarray(R.widen(c["sd:" + str(k)]))) for k in c["sd_keys"]}


def _gate(name, tag, got, c, keys):
    bad = []
    for k in keys:
        truth = c["f64:" + k]
        e_hip = rel_fro(got[k].detach().double().cpu().numpy().reshape(truth.shape), truth)
        e_ref = rel_fro(R.widen(c[f"{tag}:{k}"]), truth)
        mult = gate_multiplier(DTYPE_NAME[tag], truth.size)
        print(f"{name} {tag} {k}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {e_hip / e_ref:.3f} (m = {mult})")
        if not e_hip <= mult * e_ref:
            bad.append((k, e_hip, e_ref, mult))
    assert not bad, f"(tensor, e_hip, e_ref, m) with e_hip > m * e_ref: {bad}"


@pytest.mark.parametrize("path", R.fixture_files("op"), ids=os.path.basename)
def test_action_encoder_module_against_the_reference_fixtures(path):
    from generative_recommenders_amd.modules.action_encoder import ActionEncoder

    c = R.load(path)
    thresholds = [(int(t), int(w)) for t, w in c["thresholds"]]
    for tag in ("f32", "bf16"):
        m = ActionEncoder(action_embedding_dim=int(c["embedding_dim"]), action_feature_name="actions",
                          action_weights=[int(w) for w in c["action_weights"]], watchtime_feature_name="watchtimes",
                          watchtime_to_action_thresholds_and_weights=thresholds)
        res = m.load_state_dict(_state_dict(c), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        m = m.to(DEV).to(TORCH_DTYPE[tag])
        total = int(c["uih_offsets"][-1] + c["target_offsets"][-1])
        out = m(max_uih_len=int(c["max_uih_len"]), max_targets=int(c["max_targets"]), uih_offsets=dev_i(c["uih_offsets"]),
                target_offsets=dev_i(c["target_offsets"]), seq_embeddings=torch.zeros(total, 4, device=DEV),
                seq_payloads={"actions": dev_i(c["actions"]), "watchtimes": dev_i(c["watchtimes"])})
        assert out.dtype == TORCH_DTYPE[tag]
        want = c[f"{tag}:out"]
        assert same_bits(out, want if want.dtype == np.uint16 else want.view(np.uint32)), f"{tag}: the output is not the reference's"
        (out * torch.from_numpy(c["r"]).to(DEV).to(out.dtype)).sum().backward()
        _gate(c["name"], tag, dict(g_table=m._action_embedding_table.grad, g_target=m._target_action_embedding_table.grad), c,
              ("g_table", "g_target"))


def _build_preprocessor(kind, interleaving, pmlp, is_inference, d_out=D_OUT):
    from generative_recommenders_amd.modules.action_encoder import ActionEncoder
    from generative_recommenders_amd.modules.content_encoder import ContentEncoder
    from generative_recommenders_amd.modules.contextual_interleave_preprocessor import ContextualInterleavePreprocessor
    from generative_recommenders_amd.modules.contextualize_mlps import ParameterizedContextualizedMLP, SimpleContextualizedMLP
    from generative_recommenders_amd.modules.preprocessors import ContextualPreprocessor

    if kind == "contextual":
        return ContextualPreprocessor(
            input_embedding_dim=D_IN, output_embedding_dim=d_out, contextual_feature_to_max_length=dict(CONTEXTUAL),
            contextual_feature_to_min_uih_length=dict(MIN_UIH), action_embedding_dim=ACTION_DIM, action_feature_name="actions",
            action_weights=list(ACTION_WEIGHTS), is_inference=is_inference)

    def mlp(in_dim, out_dim, contextual_dim, is_inf):
        if pmlp:
            return ParameterizedContextualizedMLP(contextual_embedding_dim=contextual_dim, sequential_input_dim=in_dim,
                                                  sequential_output_dim=out_dim, hidden_dim=HIDDEN, is_inference=is_inf)
        return SimpleContextualizedMLP(sequential_input_dim=in_dim, sequential_output_dim=out_dim, hidden_dim=HIDDEN,
                                       is_inference=is_inf)

    return ContextualInterleavePreprocessor(
        input_embedding_dim=D_IN, output_embedding_dim=d_out, contextual_feature_to_max_length=dict(CONTEXTUAL),
        contextual_feature_to_min_uih_length=dict(MIN_UIH),
        content_encoder=ContentEncoder(input_embedding_dim=D_IN, additional_content_features=dict(ADDITIONAL),
                                       target_enrich_features=dict(ENRICH), is_inference=is_inference),
        content_contextualize_mlp_fn=mlp,
        action_encoder=ActionEncoder(action_embedding_dim=ACTION_DIM, action_feature_name="actions",
                                     action_weights=list(ACTION_WEIGHTS), watchtime_feature_name="watchtimes",
                                     watchtime_to_action_thresholds_and_weights=list(ACTION_THRESHOLDS),
                                     is_inference=is_inference),
        action_contextualize_mlp_fn=mlp, pmlp_contextual_dropout_ratio=0.0, enable_interleaving=interleaving,
        is_inference=is_inference)


FLOAT_INPUTS = ("seq_embeddings", "c0", "c1", "a0", "t0")
INT_OUTPUTS = ("seq_lengths", "seq_offsets", "seq_timestamps", "num_targets")


def _module_inputs(c, dtype, grad):
    fl = {k: torch.from_numpy(R.widen(c["in:" + k])).to(DEV).to(dtype).requires_grad_(grad) for k in FLOAT_INPUTS}
    payloads = {k: v for k, v in fl.items() if k != "seq_embeddings"}
    payloads.update({k: dev_i(c["in:" + k]) for k in ("c0_offsets", "c1_offsets", "actions", "watchtimes")})
    kw = dict(max_uih_len=int(c["max_uih_len"]), max_targets=int(c["max_targets"]), total_uih_len=int(c["total_uih_len"]),
              total_targets=int(c["total_targets"]), seq_lengths=dev_i(c["in:seq_lengths"]),
              seq_timestamps=dev_i(c["in:seq_timestamps"]), seq_embeddings=fl["seq_embeddings"],
              num_targets=dev_i(c["in:num_targets"]), seq_payloads=payloads)
    return fl, kw


@pytest.mark.parametrize("path", R.fixture_files("module"), ids=os.path.basename)
def test_preprocessor_modules_against_the_reference_fixtures(path):
    c = R.load(path)
    kind, inference = str(c["kind"]), bool(int(c["is_inference"]))
    for tag in [t for t in R.tags_of(c) if t != "f64"]:
        dtype = TORCH_DTYPE[tag]
        m = _build_preprocessor(kind, bool(int(c["enable_interleaving"])), bool(int(c["parameterized"])), inference)
        res = m.load_state_dict(_state_dict(c), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert sorted(k for k, _ in m.named_parameters()) == sorted(str(k) for k in c["param_keys"])
        m = m.to(DEV).to(dtype)
        m.set_training_dtype(dtype)
        m.train(not inference)
        fl, kw = _module_inputs(c, dtype, not inference)
        out = m(**kw)
        assert len(out) == 9 and out[8] is kw["seq_payloads"]
        for name, got in zip(("max_seq_len", "total_uih_len", "total_targets"), out[:3]):
            assert isinstance(got, int) and got == int(c[f"{tag}:out:{name}"]), name
        for name, got in zip(INT_OUTPUTS, (out[3], out[4], out[5], out[7])):
            assert np.array_equal(got.cpu().numpy(), c[f"{tag}:out:{name}"]), name
        emb = out[6]
        assert emb.dtype == dtype and emb.shape == c[f"{tag}:out:seq_embeddings"].shape
        got = {"out:seq_embeddings": emb}
        if inference:            # forward only: the embeddings are gated like every other float output
            _gate(c["name"], tag, got, c, [str(k) for k in c["gated"]])
            continue
        (emb * torch.from_numpy(c["r"]).to(DEV).to(dtype)).sum().backward()
        for k, v in fl.items():
            got["g:" + k] = v.grad if v.grad is not None else torch.zeros_like(v)
        for k, p in m.named_parameters():
            got["gp:" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
        _gate(c["name"], tag, got, c, [str(k) for k in c["gated"]])


# ------------------------------------------------------------------------------------------------------ HSTUTransducer
def _transducer(inference, interleaving, return_full, D=32):
    from conftest import load_cases
    from generative_recommenders_amd.modules.hstu_transducer import HSTUTransducer
    from generative_recommenders_amd.modules.positional_encoder import HSTUPositionalEncoder
    from generative_recommenders_amd.modules.stu import STULayer, STULayerConfig, STUStack

    c = load_cases("stu.npz")[0]                 # the 2-layer stack of test_compute_gpu.py::test_stu_stack_golden_fwd_bwd
    assert int(c["D"]) == D
    layers = [STULayer(STULayerConfig(embedding_dim=D, num_heads=int(c["H"]), hidden_dim=int(c["Hd"]), attention_dim=int(c["A"]),
                                      output_dropout_ratio=0.0, causal=True, target_aware=True, max_attn_len=None,
                                      attn_alpha=None, use_group_norm=gn, recompute_normed_x=True, recompute_uvqk=True,
                                      recompute_y=True, sort_by_length=True, contextual_seq_len=0), is_inference=inference)
              for gn in (False, True)]
    pre = _build_preprocessor("interleave", interleaving, False, inference, d_out=D)
    t = HSTUTransducer(
        stu_module=STUStack(layers, is_inference=inference), input_preprocessor=pre,
        positional_encoder=HSTUPositionalEncoder(num_position_buckets=512, num_time_buckets=64, embedding_dim=D,
                                                 contextual_seq_len=3, is_inference=inference),
        input_dropout_ratio=0.0, is_inference=inference, return_full_embeddings=return_full).to(DEV)
    return t.train(not inference)


def _transducer_inputs(grad):
    g = torch.Generator().manual_seed(5)
    lengths, targets = [7, 1, 4, 3, 9], [2, 1, 0, 3, 1]
    total, n_uih, n_tgt = sum(lengths), sum(lengths) - sum(targets), sum(targets)
    c_len = {"c0": [1, 0, 1, 1, 1], "c1": [2, 1, 0, 2, 2]}
    payloads = {"a0": torch.randn(total, 8, generator=g).to(DEV), "t0": torch.randn(n_tgt, 8, generator=g).to(DEV),
                "actions": torch.randint(0, 16, (n_uih,), generator=g).to(DEV),
                "watchtimes": torch.randint(0, 60, (n_uih,), generator=g).to(DEV)}
    for k, lens in c_len.items():
        payloads[k] = torch.randn(sum(lens), D_IN, generator=g).to(DEV)
        payloads[k + "_offsets"] = dev_i(R.offsets_of(lens))
    kw = dict(max_uih_len=max(l - t for l, t in zip(lengths, targets)), max_targets=max(targets), total_uih_len=n_uih,
              total_targets=n_tgt, seq_lengths=dev_i(lengths),
              seq_embeddings=torch.randn(total, D_IN, generator=g).to(DEV).requires_grad_(grad),
              seq_timestamps=torch.randint(1, 10**6, (total,), generator=g).sort().values.to(DEV), num_targets=dev_i(targets),
              seq_payloads=payloads)
    return kw, lengths, targets


def _by_hand(t, kw):
    """the same sub-modules called one by one"""
    from generative_recommenders_amd.modules.hstu_transducer import hstu_postprocess

    pre_kw = {k: v for k, v in kw.items()}
    (max_seq_len, total_uih_len, total_targets, lengths, offsets, timestamps, emb, num_targets, payloads) = t._input_preprocessor(**pre_kw)
    emb = t._positional_encoder(max_seq_len=max_seq_len, seq_lengths=lengths, seq_offsets=offsets, seq_timestamps=timestamps,
                                seq_embeddings=emb, num_targets=num_targets)
    enc = t._stu_module(x=emb, x_lengths=lengths, x_offsets=offsets, max_seq_len=max_seq_len, num_targets=num_targets)
    full, cand = hstu_postprocess(t._output_postprocessor, max_seq_len=max_seq_len, total_uih_len=total_uih_len,
                                  total_targets=total_targets, seq_lengths=lengths, seq_timestamps=timestamps, seq_embeddings=enc,
                                  num_targets=num_targets, seq_payloads=payloads, return_full_embeddings=t._return_full_embeddings,
                                  interleave_targets=t._input_preprocessor.interleave_targets())
    return cand, full, lengths, num_targets


@pytest.mark.parametrize("return_full", [False, True], ids=["candidates", "full"])
@pytest.mark.parametrize("interleaving", [False, True], ids=["sum", "interleave"])
def test_transducer_in_training_equals_its_parts_called_one_by_one(interleaving, return_full):
    t = _transducer(False, interleaving, return_full)
    kw, lengths, targets = _transducer_inputs(True)
    cand, full = t(**kw)
    cand2, full2, out_len, out_nt = _by_hand(t, kw)
    assert cand.shape == (sum(targets), 32) and torch.equal(cand.view(torch.int32), cand2.view(torch.int32))
    assert (full is None) == (not return_full)
    if return_full:
        assert torch.equal(full.view(torch.int32), full2.view(torch.int32))
        # the candidate rows are the users' last (2 T | T) rows, every second one when the targets are interleaved
        want = R.candidates(bits(full), out_len.cpu().numpy(), out_nt.cpu().numpy(), interleaving)
        assert same_bits(cand, want)
        assert np.array_equal(out_nt.cpu().numpy(), np.asarray(targets) * (2 if interleaving else 1))
    r = torch.randn(cand.shape, device=DEV)
    (cand * r).sum().backward()
    for name, p in t.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), f"gradient of {name}"
    assert bool(torch.isfinite(kw["seq_embeddings"].grad).all())


def test_transducer_in_inference_with_interleaving_equals_its_parts():
    t = _transducer(True, True, False).eval()
    kw, lengths, targets = _transducer_inputs(False)
    with torch.no_grad():
        cand, full = t(**kw)
        cand2, _, out_len, out_nt = _by_hand(t, kw)
    assert full is None and cand.shape == (sum(targets), 32) and torch.equal(cand.view(torch.int32), cand2.view(torch.int32))
    assert np.array_equal(out_len.cpu().numpy(), R.out_lengths(lengths, targets, 3, R.INTERLEAVE_UIH))
    assert np.array_equal(out_nt.cpu().numpy(), targets) and bool(torch.isfinite(cand).all())
