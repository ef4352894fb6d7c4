"""CPU checks of the SASRec baseline: the ABI and the new symbols, argument validation of the C entry points (all before any
launch, so it runs without a GPU), the ``supported`` rule, the fp64 restatement against the fixtures, the power of the
fixtures to catch the obvious wrong kernels, the module's drop-in surface and the reproducibility of the fixtures."""

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import softmax_attn_ref as R
from conftest import ROOT

REFERENCE = "/root/reference/generative_recommenders"
CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")
SYMBOLS = ("hstu_softmax_attn_supported", "hstu_softmax_attn_fwd", "hstu_softmax_attn_bwd")
OP_CASES = R.op_case_names()
MODEL_CASES = R.model_case_names()


@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def op_cases():
    return {n: R.load_op_case(n) for n in OP_CASES}


# ------------------------------------------------------------------------------------------------------------ the C boundary
def test_abi_is_13_in_the_library_the_header_and_the_binding(lib):
    from generative_recommenders_amd import _lib

    header = open(os.path.join(ROOT, "include", "hstu_hip.h")).read()
    assert re.search(r"#define HSTU_ABI_VERSION (\d+)", header).group(1) == "13"
    assert _lib.ABI_VERSION == 13 == lib.hstu_abi_version()


def test_symbols_declared_exported_and_in_the_signature_table(lib):
    from generative_recommenders_amd import _lib
    from generative_recommenders_amd.ops import _launch

    header = open(os.path.join(ROOT, "include", "hstu_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        proto = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert proto, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == len(proto.group(1).split(",")), name      # one ctypes entry per C parameter
    consts = {k: int(v) for k, v in re.findall(r"#define HSTU_SOFTMAX_ATTN_(\w+) (\d+)", header)}
    assert consts == {"MAX_HEAD_DIM": _launch.SOFTMAX_ATTN_MAX_HEAD_DIM, "MAX_SEQ_LEN": _launch.SOFTMAX_ATTN_MAX_SEQ_LEN}
    assert "sasrec.py:209-214" in header                                                  # the reference lines it replaces
    assert "softmax_attn.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_entry_points_refuse_bad_arguments_with_a_message(lib):
    BF16, F32 = 0, 2
    buf = (C.c_char * 4096)()
    a = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.hstu_last_error()

    def fwd(q=a, k=a, v=a, out=a, lse=a, off=a, rs=64, hs=64, rows=4, batch=1, heads=1, d=64, n=70, scale=0.125, p=0.0, dt=BF16, it=1):
        return lib.hstu_softmax_attn_fwd(q, rs, hs, k, rs, hs, v, rs, hs, out, lse, off, rows, batch, heads, d, n, scale, p, 7, dt, it, None)

    def bwd(dout=a, q=a, k=a, v=a, out=a, lse=a, delta=a, dq=a, dk=a, dv=a, off=a, rs=64, hs=64, rows=4, batch=1, heads=1, d=64,
            n=70, scale=0.125, p=0.0, dt=BF16, it=1):
        return lib.hstu_softmax_attn_bwd(dout, q, rs, hs, k, rs, hs, v, rs, hs, out, lse, delta, dq, dk, dv, off, rows, batch, heads,
                                         d, n, scale, p, 7, dt, it, None)

    for call in (fwd, bwd):
        assert call(dt=7) == -1 and b"dtype" in err()
        assert call(it=5) == -1 and b"int32 or int64" in err()
        assert call(d=0) == -1 and b"head_dim must be positive" in err()
        assert call(d=72) == -2 and b"exceeds the limit of 64" in err()
        assert call(d=50) == -1 and b"multiple of 8" in err()
        assert call(d=6, dt=F32) == -1 and b"multiple of 4" in err()
        assert call(n=0) == -1 and b"max_seq_len must be at least 1" in err()
        assert call(n=513) == -2 and b"exceeds the limit of 512" in err()
        assert call(p=1.0) == -1 and b"dropout_p must be in [0, 1)" in err()
        assert call(p=-0.1) == -1 and b"dropout_p" in err()
        assert call(p=float("nan")) == -1 and b"dropout_p" in err()
        assert call(heads=0) == -1 and b"heads" in err()
        assert call(batch=-1) == -1 and b"batch" in err()
        for arg in ("q", "k", "v", "out", "lse", "off"):
            assert call(**{arg: None}) == -1 and b"non-NULL" in err(), arg
        assert call(rs=68) == -1 and b"16-byte aligned (stride 68" in err()
        assert call(hs=4) == -1 and b"16-byte aligned (stride 4" in err()
        assert call(q=a + 2) == -1 and b"base pointers" in err()
        assert call(lse=a + 2) == -1 and b"4-byte aligned" in err()
        # no rows / no users: nothing is read, nothing launched
        assert call(q=None, k=None, v=None, out=None, lse=None, rows=0) == 0
        assert call(q=None, off=None, batch=0) == 0
    for arg in ("dout", "delta", "dq", "dk", "dv"):
        assert bwd(**{arg: None}) == -1 and b"non-NULL" in err(), arg
    assert bwd(dq=a + 8) == -1 and b"base pointers" in err()


def test_supported_rule(lib):
    from generative_recommenders_amd.ops import _launch

    BF16, F16, F32, FP8 = 0, 1, 2, 3
    table = [(BF16, 1, 1, 1), (BF16, 16, 60, 1), (BF16, 50, 210, 1), (F16, 64, 510, 1), (F32, 64, 512, 1), (BF16, 64, 513, 0),
             (F16, 65, 210, 0), (F32, 80, 210, 0), (BF16, 0, 210, 0), (BF16, 64, 0, 0), (FP8, 64, 210, 0), (9, 64, 210, 0),
             (F32, 50, 600, 0)]
    torch_dt = {BF16: torch.bfloat16, F16: torch.float16, F32: torch.float32, FP8: torch.float8_e4m3fn, 9: torch.float64}
    for dt, d, n, want in table:
        assert lib.hstu_softmax_attn_supported(dt, d, n) == want, (dt, d, n)
        assert _launch.softmax_attn_supported(torch_dt[dt], d, n) == bool(want), (dt, d, n)


# --------------------------------------------------------------------------------------------------------------- the fixtures
def test_fixture_set_covers_the_cases_of_the_issue(op_cases):
    got = [(c["q"].shape[1], c["q"].shape[2], c["max_seq_len"], c["lengths"].tolist()) for c in op_cases.values()]
    assert got == [(2, 16, 70, [0, 1, 2, 31, 32, 33, 64, 65, 70]), (1, 50, 210, [210, 129, 128, 7]), (4, 64, 130, [130, 96, 1]),
                   (1, 64, 510, [510, 257, 3])]
    for c in op_cases.values():
        assert c["lengths"].max() >= 2 and c["q"].shape[0] == c["lengths"].sum()
        for tag in ("f32", "bf16"):          # a relative gate needs a reference that is off the truth
            for g in R.GRADS:
                assert R.rel_fro(c[f"{tag}:{g}"], c[f"f64:{g}"]) > 0.0, (c["name"], tag, g)
    assert len(MODEL_CASES) == 2


@pytest.mark.parametrize("name", OP_CASES)
def test_restatement_reproduces_the_f64_tensors(op_cases, name):
    c = op_cases[name]
    res = R.restate(c["q"], c["k"], c["v"], c["dout"], c["lengths"])
    for g in R.GRADS:
        assert R.rel_fro(res[g], c[f"f64:{g}"]) <= 1e-12, (name, g)
        assert np.abs(res[g] - c[f"f64:{g}"]).max() <= 1e-12 * max(1.0, np.abs(c[f"f64:{g}"]).max()), (name, g)


@pytest.mark.parametrize("name", OP_CASES)
def test_math_path_reproduces_the_low_precision_tensors(op_cases, name):
    """e_ref of the drawn batches comes from this function: on the fixtures' inputs it is what the fixtures store"""
    c = op_cases[name]
    for tag in ("f32", "bf16"):
        res = R.math_path(c["q"], c["k"], c["v"], c["dout"], c["lengths"], c["max_seq_len"], R.TORCH_DTYPE[tag])
        for g in R.GRADS:
            assert R.rel_fro(res[g], c[f"{tag}:{g}"]) <= (1e-6 if tag == "f32" else 1e-3), (name, tag, g)


def _caught(c, wrong_res, truth, tag):
    ref = {g: c[f"{tag}:{g}"] for g in R.GRADS}
    return R.gate(f"{c['name']} wrong", wrong_res, ref, truth, R.DTYPE_NAME[tag])


def test_fixtures_catch_the_obvious_wrong_kernels(op_cases):
    """each wrong kernel -- computed exactly, in fp64 -- fails the gate on at least one tensor of at least one case, for both tags"""
    truth = {n: {g: c[f"f64:{g}"] for g in R.GRADS} for n, c in op_cases.items()}
    for tag in ("f32", "bf16"):
        no_causal = [_caught(c, R.restate(c["q"], c["k"], c["v"], c["dout"], c["lengths"], wrong="no_causal"), truth[n], tag)
                     for n, c in op_cases.items()]
        assert any(no_causal), "no causal mask"
        neighbours = [_caught(c, R.restate(c["q"], c["k"], c["v"], c["dout"], c["lengths"], wrong="ignore_offsets"), truth[n], tag)
                      for n, c in op_cases.items()]
        assert any(neighbours), "offsets ignored"
        c = op_cases["op_2_h1_d50_n210"]          # head dim 50 is instantiated at 64
        assert _caught(c, R.restate(c["q"], c["k"], c["v"], c["dout"], c["lengths"], scale=64 ** -0.5), truth[c["name"]], tag), \
            "scale from the padded head dim"


def test_fixtures_catch_lse_taken_after_dropout(op_cases):
    c = op_cases["op_1_h2_d16_n70"]
    L, H, _ = c["q"].shape
    keep, ks = R.keep_mask(1234, L, H, c["max_seq_len"], 0.2)
    args = (c["q"], c["k"], c["v"], c["dout"], c["lengths"])
    truth = R.restate(*args, keep=keep, keep_scale=ks)
    ref = R.math_path(*args, c["max_seq_len"], torch.bfloat16, keep=keep, keep_scale=ks)
    assert not R.gate("dropout, exact", truth, ref, truth, "bfloat16")
    assert R.gate("lse after dropout", R.restate(*args, keep=keep, keep_scale=ks, wrong="lse_after_dropout"), ref, truth, "bfloat16")
    # delta = rowsum(dO o O) stays valid with the dropped O: the restatement's delta is rowsum(P dP)
    delta = (c["dout"] * truth["out"]).sum(axis=-1)
    assert np.isfinite(delta).all()


def test_lse_restatement_is_the_log_of_the_row_sum(op_cases):
    c = op_cases["op_1_h2_d16_n70"]
    lse = R.lse_of(c["q"], c["k"], c["lengths"])
    offs = R.offsets_of(c["lengths"])
    r = int(offs[3]) + 5                                                        # row 5 of the 31-row user, head 1
    s = (c["q"][r, 1] @ c["k"][int(offs[3]): r + 1, 1].T) * 16 ** -0.5
    assert abs(lse[r, 1] - np.log(np.exp(s).sum())) <= 1e-12


def test_fixture_files_are_small():
    files = [f for f in os.listdir(R.FIXTURES) if f.endswith(".npz")]
    assert len(files) >= 4 * 5 + 2 + 1
    for f in files:
        assert os.path.getsize(os.path.join(R.FIXTURES, f)) <= 1 << 20, f
    assert os.listdir(os.path.join(ROOT, "tests", "golden")).count("sasrec") == 1


# ----------------------------------------------------------------------------------------------------------------- the module
def _build(D, H, blocks, act, hidden, n, **kw):
    from sasrec_stubs import build_model

    return build_model(D, H, blocks, act, hidden, n, **kw)


@pytest.mark.parametrize("name", MODEL_CASES)
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    names = np.load(os.path.join(R.FIXTURES, "reference_names.npz"))
    c = R.load_model_case(name)
    D, H, blocks, hidden, n = (int(x) for x in c["config"])
    model, _ = _build(D, H, blocks, str(c["activation"]), hidden, n)
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in names["keys"]] == [str(k) for k in c["sd_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in names[f"{name}:shapes"]]
    for i in range(blocks):
        for k in (f"attention_layers.{i}.in_proj_weight", f"attention_layers.{i}.in_proj_bias", f"attention_layers.{i}.out_proj.weight",
                  f"attention_layers.{i}.out_proj.bias", f"forward_layers.{i}._conv1d.0.weight", f"forward_layers.{i}._conv1d.0.bias",
                  f"forward_layers.{i}._conv1d.3.weight", f"forward_layers.{i}._conv1d.3.bias"):
            assert k in sd, k
    assert "_attn_mask" in sd and sd["_attn_mask"].shape == (n, n) and sd["_attn_mask"].dtype == torch.bool
    res = model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(c["sd:" + k])).to(sd[k].dtype) for k in sd}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_model_multiplier_follows_the_references_own_relu_flips():
    a, b = (R.load_model_case(n) for n in MODEL_CASES)
    assert a["bf16:relu_flips"].tolist() == [0, 0] and str(a["activation"]) == "gelu"
    flips = b["bf16:relu_flips"]
    assert str(b["activation"]) == "relu" and flips.shape == (2,) and 0 < flips.min() and flips.sum() < 100
    mm = lambda t, fl=flips, dt="bfloat16": R.model_multiplier(dt, t, 2500, fl)
    assert mm("out") == 1.5 and mm("g:forward_layers.1._conv1d.3.weight") == 1.5 and mm("g:emb", dt="float32") == 8.0
    assert mm("g:emb", fl=a["bf16:relu_flips"]) == 1.5
    assert mm("g:forward_layers.1._conv1d.0.weight") == mm("g:attention_layers.1.in_proj_bias") == mm("g:forward_layers.0._conv1d.3.bias")
    assert 1.5 <= mm("g:emb") == mm("g:forward_layers.0._conv1d.0.bias") <= mm("g:forward_layers.1._conv1d.0.weight") < 2.5
    assert abs(R.model_multiplier("bfloat16", "g:emb", 2500, np.array([18])) - 1.76) < 0.01      # sqrt(F_0.99(18, 18))


def test_module_constructs_on_the_cpu_with_the_reference_surface():
    from generative_recommenders_amd.research.modeling.sequential.sasrec import SASRec, StandardAttentionFF

    model, _ = _build(48, 3, 2, "gelu", 40, 40, ffn_dropout_rate=0.2, activation_checkpoint=True)
    assert isinstance(model, SASRec) and isinstance(model.forward_layers[0], StandardAttentionFF)
    assert isinstance(model.attention_layers[0], torch.nn.MultiheadAttention) and model.attention_layers[0].dropout == 0.2
    assert model.debug_str() == "SASRec-d48-b2-h3-stub_pre-stub_post-ffn40-gelu-d0.2-ac"
    assert model._max_sequence_length == 40 and model._attn_mask[0, 1] and not model._attn_mask[1, 0]
    for i in range(2):      # reset_state: xavier on the matrices, the 1-D parameters as constructed (attention biases zero)
        assert float(model.attention_layers[i].in_proj_bias.detach().abs().max()) == 0.0
        assert float(model.attention_layers[i].out_proj.bias.detach().abs().max()) == 0.0
        w = model.attention_layers[i].in_proj_weight
        assert abs(float(w.detach().std()) - (2.0 / (48 + 144)) ** 0.5) < 0.02
    assert not hasattr(model, "predict")
    with pytest.raises(AssertionError, match="Invalid activation_fn"):
        StandardAttentionFF(8, 8, "silu", 0.0)
    ff = StandardAttentionFF(8, 6, "relu", 0.0)
    x = torch.randn(5, 8)
    assert torch.allclose(ff.jagged_forward(x), ff(x.unsqueeze(0))[0], atol=1e-6)       # the jagged form of the same module


def test_cpu_tensors_are_refused_by_the_op():
    from generative_recommenders_amd.ops.softmax_attention import (jagged_causal_softmax_attention,
                                                                   jagged_causal_softmax_attention_composed)

    q = torch.zeros(4, 2, 16)
    off = torch.tensor([0, 4])
    for f in (jagged_causal_softmax_attention, jagged_causal_softmax_attention_composed):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(4, q, q, q, off)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree (build container only)")
def test_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    maker = os.path.join(R.FIXTURES, "make_sasrec_golden.py")
    res = subprocess.run([sys.executable, "-W", "ignore", maker, "--out", str(tmp_path)], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    committed = sorted(f for f in os.listdir(R.FIXTURES) if f.endswith(".npz"))
    fresh = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert committed == fresh and committed
    for f in committed:
        a, b = np.load(os.path.join(R.FIXTURES, f)), np.load(os.path.join(tmp_path, f))
        assert sorted(a.files) == sorted(b.files), f
        for key in a.files:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, f"{f}:{key} dtype / shape"
            assert np.array_equal(a[key], b[key]), f"{f}:{key} is not reproduced bit for bit"
