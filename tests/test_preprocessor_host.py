"""CPU tests of the input preprocessors: the new C entry points are declared, exported and bound without an ABI bump, their
argument checks answer before any launch, and the numpy restatement (tests/preprocessor_ref.py) reproduces the fixtures
minted from the reference EXACTLY -- which pins the restatement the GPU tests compare against to the reference."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import preprocessor_ref as R
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hstu_hip.h")
SYMBOLS = ("hstu_action_encode_fwd", "hstu_action_encode_bwd", "hstu_action_encode_bwd_workspace_bytes",
           "hstu_combine_embeddings_fwd", "hstu_combine_embeddings_bwd")
EINVAL = -1
BF16, F16, F32 = 0, 1, 2
I32, I64 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbols_declared_exported_and_bound(lib):
    from generative_recommenders_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hstu_[a-z0-9_]+)\s*\(", src))
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/hstu_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert hasattr(lib, name), f"libhstu_hip.so does not export {name}"
    from generative_recommenders_amd.ops import _launch, preprocess

    for fn in ("action_encode_fwd", "action_encode_bwd", "combine_embeddings_fwd", "combine_embeddings_bwd"):
        assert callable(getattr(_launch, fn))
    assert callable(preprocess.action_encode) and callable(preprocess.combine_embeddings)


def test_abi_version_is_unchanged(lib):
    from generative_recommenders_amd import _lib

    assert lib.hstu_abi_version() == _lib.ABI_VERSION == 13
    assert re.search(r"#define\s+HSTU_ABI_VERSION\s+13\b", open(HEADER).read())


def _buf():
    raw = (C.c_char * 4096)()
    return raw, (C.addressof(raw) + 15) & ~15


def test_action_encode_argument_checks_without_gpu(lib):
    raw, a = _buf()
    w = (C.c_int64 * 65)(*range(1, 66))

    def fwd(actions=a, uo=a, to=a, table=a, ttable=a, weights=w, T=3, thr=None, tw=None, nthr=0, out=a, uih=4, tgt=2, B=2,
            da=8, dt=BF16, it=I64):
        return lib.hstu_action_encode_fwd(actions, None, uo, to, table, ttable, weights, T, thr, tw, nthr, out, uih, tgt, B, da, dt,
                                          it, None)

    def bwd(dout=a, uo=a, to=a, weights=w, T=3, d_table=a, d_target=a, ws=a, uih=4, tgt=2, B=2, da=8, dt=BF16, it=I64):
        return lib.hstu_action_encode_bwd(dout, a, None, uo, to, weights, T, None, None, 0, d_table, d_target, ws, uih, tgt, B, da,
                                          dt, it, None)

    assert fwd(T=65) == EINVAL and b"action types" in lib.hstu_last_error()
    assert bwd(T=65) == EINVAL and b"action types" in lib.hstu_last_error()
    assert fwd(T=0) == EINVAL
    assert fwd(uo=None) == EINVAL and b"offsets" in lib.hstu_last_error()
    assert fwd(to=None) == EINVAL and bwd(uo=None) == EINVAL and bwd(to=None) == EINVAL
    assert fwd(uih=-1) == EINVAL and fwd(tgt=-1) == EINVAL and fwd(B=-1) == EINVAL and fwd(da=0) == EINVAL
    assert bwd(uih=-1) == EINVAL and bwd(B=-1) == EINVAL
    assert fwd(dt=7) == EINVAL and b"dtype" in lib.hstu_last_error()
    assert bwd(dt=3) == EINVAL and fwd(it=5) == EINVAL
    assert fwd(uih=2**31, tgt=0) == EINVAL and b"2^31" in lib.hstu_last_error()
    assert fwd(nthr=1) == EINVAL                                   # thresholds announced, host arrays NULL
    assert fwd(weights=None) == EINVAL and fwd(table=None) == EINVAL and fwd(out=None) == EINVAL
    assert bwd(d_table=None) == EINVAL and bwd(ws=None) == EINVAL
    assert fwd(B=0) == 0 and fwd(uih=0, tgt=0) == 0                # nothing to do: no launch, no error
    assert lib.hstu_action_encode_bwd_workspace_bytes(1000, 256) > 0
    assert lib.hstu_action_encode_bwd_workspace_bytes(1000, 0) == 0
    del raw


def test_combine_argument_checks_without_gpu(lib):
    raw, a = _buf()

    def fwd(content=a, action=a, ctx=a, ts=a, so=a, nt=a, oo=a, out=a, out_ts=a, uih=4, tgt=2, B=2, Cn=1, D=8, mode=0, dt=BF16,
            it=I64):
        return lib.hstu_combine_embeddings_fwd(content, action, ctx, ts, so, nt, oo, out, out_ts, uih, tgt, B, Cn, D, mode, dt, it,
                                               None)

    def bwd(dout=a, so=a, nt=a, oo=a, dc=a, da=a, dctx=a, uih=4, tgt=2, B=2, Cn=1, D=8, mode=0, dt=BF16, it=I64):
        return lib.hstu_combine_embeddings_bwd(dout, so, nt, oo, dc, da, dctx, uih, tgt, B, Cn, D, mode, dt, it, None)

    assert fwd(mode=3) == EINVAL and b"unknown mode" in lib.hstu_last_error()
    assert bwd(mode=-1) == EINVAL and b"unknown mode" in lib.hstu_last_error()
    assert fwd(dt=3) == EINVAL and bwd(dt=9) == EINVAL and fwd(it=2) == EINVAL
    assert fwd(so=None) == EINVAL and b"offsets" in lib.hstu_last_error()
    assert fwd(oo=None) == EINVAL and bwd(so=None) == EINVAL and bwd(oo=None) == EINVAL
    assert fwd(uih=-1) == EINVAL and fwd(tgt=-3) == EINVAL and fwd(B=-1) == EINVAL and fwd(Cn=-1) == EINVAL and fwd(D=0) == EINVAL
    assert bwd(uih=-1) == EINVAL and bwd(Cn=-1) == EINVAL
    assert fwd(mode=2, nt=None) == EINVAL and b"num_targets" in lib.hstu_last_error()
    assert fwd(mode=1, action=None) == EINVAL and b"action" in lib.hstu_last_error()
    assert fwd(uih=2**30, tgt=0, mode=1) == EINVAL and b"2^31" in lib.hstu_last_error()      # 2 * 2^30 output rows
    assert fwd(content=None) == EINVAL and fwd(out_ts=None) == EINVAL and fwd(ctx=None) == EINVAL
    assert bwd(dout=None) == EINVAL and bwd(dc=None) == EINVAL
    assert fwd(B=0) == 0 and bwd(B=0) == 0 and fwd(uih=0, tgt=0, Cn=0) == 0
    del raw


def test_python_layer_refuses_cpu_tensors():
    from generative_recommenders_amd.ops.preprocess import COMBINE_SUM, action_encode, combine_embeddings

    off = torch.tensor([0, 2])
    with pytest.raises(RuntimeError, match="GPU"):
        action_encode(torch.zeros(2, dtype=torch.int64), None, off, torch.tensor([0, 1]), torch.zeros(2, 4), torch.zeros(1, 8),
                      [1, 2], [], 2, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        combine_embeddings(torch.zeros(2, 8), None, None, torch.zeros(2, dtype=torch.int64), torch.tensor([2]), off,
                           torch.tensor([1]), 1, 1, COMBINE_SUM)


# -------------------------------------------------------------------------------------- the restatement against the fixtures
@pytest.mark.parametrize("path", R.fixture_files("op"), ids=os.path.basename)
def test_action_encode_restatement_reproduces_the_fixture_bit_for_bit(path):
    c = R.load(path)
    weights = [int(w) for w in c["action_weights"]] + [int(w) for _, w in c["thresholds"]]
    thresholds = [(int(t), int(w)) for t, w in c["thresholds"]]
    da = int(c["embedding_dim"])
    table, target = c["sd:_action_embedding_table"], c["sd:_target_action_embedding_table"]       # bf16 bit patterns
    assert table.dtype == np.uint16 and [int(w) for w in c["sd:_combined_action_weights"]] == weights
    out_bits = R.action_encode(c["actions"], c["watchtimes"], c["uih_offsets"], c["target_offsets"], table, target, weights,
                               thresholds)
    assert np.array_equal(out_bits, c["bf16:out"])
    assert np.array_equal(R.widen(out_bits), c["f32:out"]) and np.array_equal(R.widen(out_bits).astype(np.float64), c["f64:out"])
    ref = R.action_encode_bwd(c["r"], c["actions"], c["watchtimes"], c["uih_offsets"], c["target_offsets"], weights, thresholds, da)
    np.testing.assert_allclose(ref["d_table"], c["f64:g_table"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["d_target"], c["f64:g_target"].reshape(-1), rtol=1e-12, atol=1e-12)
    for name, key in (("table", "f32:g_table"), ("target", "f32:g_target")):     # the reference's own fp32 sums obey the bound
        err = np.abs(c[key].reshape(ref["d_" + name].shape).astype(np.float64) - ref["d_" + name])
        assert (err <= ref["n_" + name] * 2.0**-24 * ref["abs_" + name] + 1e-300).all()


def _torch_add(a, b, tag):
    """content + action in the activation dtype, as the reference adds them"""
    if tag == "bf16":
        ta, tb = (torch.from_numpy(x.view(np.int16).copy()).view(torch.bfloat16) for x in (a, b))
        return (ta + tb).view(torch.int16).numpy().view(np.uint16)
    return (torch.from_numpy(a.copy()) + torch.from_numpy(b.copy())).numpy()


@pytest.mark.parametrize("path", [p for p in R.fixture_files("module") if "contextual" not in os.path.basename(p)],
                         ids=os.path.basename)
def test_combine_restatement_reproduces_the_module_fixture(path):
    c = R.load(path)
    mode = R.mode_of(c)
    lengths, targets = c["in:seq_lengths"], c["in:num_targets"]
    for tag in R.tags_of(c):
        content, action, ctx = c[f"{tag}:mlp:content"], c[f"{tag}:mlp:action"], c[f"{tag}:mlp:contextual"]
        summed = _torch_add(content, action, tag) if mode == R.SUM else None
        emb, ts, out_len = R.combine(content, action, ctx, c["in:seq_timestamps"], lengths, targets, mode, summed)
        assert np.array_equal(emb, c[f"{tag}:out:seq_embeddings"]), f"{tag}: embeddings"
        assert np.array_equal(ts, c[f"{tag}:out:seq_timestamps"]), f"{tag}: timestamps"
        assert np.array_equal(out_len, c[f"{tag}:out:seq_lengths"])
        assert np.array_equal(R.offsets_of(out_len), c[f"{tag}:out:seq_offsets"])
        C_len = ctx.shape[1]
        B, uih, tgt = len(lengths), int(c["total_uih_len"]), int(c["total_targets"])
        exp = {R.SUM: (uih, tgt, targets), R.INTERLEAVE_ALL: (2 * uih, 2 * tgt, 2 * targets),
               R.INTERLEAVE_UIH: (2 * uih, tgt, targets)}[mode]
        assert int(c[f"{tag}:out:total_uih_len"]) == exp[0] + B * C_len and int(c[f"{tag}:out:total_targets"]) == exp[1]
        assert np.array_equal(c[f"{tag}:out:num_targets"], exp[2])
        assert int(c[f"{tag}:out:max_seq_len"]) >= int(out_len.max())


def test_contextual_preprocessor_fixture_layout():
    c = R.load(os.path.join(R.FIXTURES, "module_contextual.npz"))
    lengths, targets = c["in:seq_lengths"], c["in:num_targets"]
    emb = c["f32:out:seq_embeddings"]
    out_len = R.out_lengths(lengths, targets, 3, R.SUM)
    assert np.array_equal(out_len, c["f32:out:seq_lengths"]) and emb.shape[0] == int(out_len.sum())
    oo = R.offsets_of(out_len)
    ctx = np.stack([emb[int(o):int(o) + 3] for o in oo[:-1]])
    seq = np.concatenate([emb[int(oo[b]) + 3:int(oo[b + 1])] for b in range(len(lengths))])
    again, ts, _ = R.combine(seq, None, ctx, c["in:seq_timestamps"], lengths, targets, R.SUM)
    assert np.array_equal(again, emb) and np.array_equal(ts, c["f32:out:seq_timestamps"])


def test_index_map_restatement_equals_the_per_row_loops():
    """the whole-array paths of preprocessor_ref.py (for the large batches of test_input_stage_classes_gpu.py) against its
    per-row loops, on the 17 users of test_preprocessor_gpu.py: moves bit for bit, the fp64 sums exactly (integer terms)"""
    lengths = np.array([7, 0, 4, 3, 9, 40, 12, 1, 5, 2, 31, 8, 16, 6, 23, 11, 3])
    targets = np.array([2, 0, 0, 3, 1, 7, 0, 0, 5, 1, 4, 8, 3, 2, 9, 1, 1])
    rng = np.random.default_rng(17)
    total, uih = int(lengths.sum()), lengths - targets
    uo, to = R.offsets_of(uih), R.offsets_of(targets)
    for weights, thresholds, da in (([2, 1, 4], [(10, 1), (50, 4)], 5), ([1 << 62, 3, (1 << 40) | 8, 16], [(30, 16)], 8)):
        T = len(weights)
        actions = rng.integers(0, 2**63 - 1, int(uih.sum())) if max(weights) > 2**32 else rng.integers(0, 16, int(uih.sum()))
        watch = rng.integers(0, 100, int(uih.sum()))
        table = rng.integers(0, 2**16, (T, da)).astype(np.uint16)
        target = rng.integers(0, 2**16, T * da).astype(np.uint16)
        args = (actions, watch, uo, to, table, target, weights, thresholds)
        assert np.array_equal(R.action_encode_mapped(*args), R.action_encode(*args))
        d_out = rng.integers(-8, 9, (total, T * da)).astype(np.float64)
        a, b = (f(d_out, actions, watch, uo, to, weights, thresholds, da) for f in (R.action_encode_bwd_mapped, R.action_encode_bwd))
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    content, action = (rng.integers(0, 2**16, (total, 6)).astype(np.uint16) for _ in range(2))
    summed = rng.integers(0, 2**16, (total, 6)).astype(np.uint16)
    ts = rng.integers(1, 10**9, total)
    for mode in (R.SUM, R.INTERLEAVE_ALL, R.INTERLEAVE_UIH):
        for C in (0, 3):
            ctx = rng.integers(0, 2**16, (len(lengths), C, 6)).astype(np.uint16) if C else None
            for has_action in ((True, False) if mode == R.SUM else (True,)):
                args = (content, action if has_action else None, ctx, ts, lengths, targets, mode, summed if has_action else None)
                got, want = R.combine_mapped(*args), R.combine(*args)
                assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want)), (mode, C, has_action)
                d_out = rng.integers(1, 2**16, want[0].shape).astype(np.uint16)
                got = R.combine_bwd_mapped(d_out, lengths, targets, C, mode, has_action)
                want = R.combine_bwd(d_out, lengths, targets, C, mode, has_action)
                assert all((g is None and w is None) or np.array_equal(g, w) for g, w in zip(got, want)), (mode, C, has_action)
    b, j, src, act = R.combine_row_map([], [], 3, R.INTERLEAVE_UIH)
    assert b.size == 0 and R.action_row_map([0], [0]).size == 0


def test_restatement_backward_is_the_inverse_of_the_forward():
    """combine_bwd(combine(x)) returns x for every row that the forward copied (and zeros for the dropped action targets)"""
    rng = np.random.default_rng(0)
    lengths, targets = np.array([5, 0, 3, 2, 4]), np.array([2, 0, 0, 2, 1])
    total = int(lengths.sum())
    content, action = rng.integers(1, 2**16, (total, 3)).astype(np.uint16), rng.integers(1, 2**16, (total, 3)).astype(np.uint16)
    ctx = rng.integers(1, 2**16, (5, 2, 3)).astype(np.uint16)
    for mode in (R.INTERLEAVE_ALL, R.INTERLEAVE_UIH):
        emb, _, _ = R.combine(content, action, ctx, np.arange(total), lengths, targets, mode)
        dc, da, dx = R.combine_bwd(emb, lengths, targets, 2, mode, True)
        assert np.array_equal(dc, content) and np.array_equal(dx, ctx)
        keep = np.ones(total, dtype=bool)
        if mode == R.INTERLEAVE_UIH:
            off = R.offsets_of(lengths)
            for b in range(5):
                keep[int(off[b + 1]) - int(targets[b]):int(off[b + 1])] = False
        assert np.array_equal(da[keep], action[keep]) and not da[~keep].any()
