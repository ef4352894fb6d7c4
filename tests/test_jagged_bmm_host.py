"""CPU-side checks of jagged_dense_bmm_broadcast_add and the contextualized MLPs: the C ABI exports and validates the new
entry points, the Python layers import, the fixtures under tests/golden/jagged_bmm/ regenerate bit for bit, and the fp64
helper the GPU tests gate against agrees with the reference outputs stored in the fp32 fixtures."""

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from jagged_bmm_ref import FIXTURES, OP_TENSORS, bmm_fp64, load_op_case, op_case_files, rel_fro

REFERENCE = "/root/reference/generative_recommenders"
NEW = ("hstu_jagged_dense_bmm_workspace_bytes", "hstu_jagged_dense_bmm_fwd", "hstu_jagged_dense_bmm_wgrad")


@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_entry_points_declared_exported_and_bound(lib):
    from generative_recommenders_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hstu_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/hstu_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"libhstu_hip.so does not export {name}"
    assert lib.hstu_abi_version() == 13        # purely additive
    assert lib.hstu_jagged_dense_bmm_workspace_bytes(7) >= 8 * 4


def test_python_layers_import():
    import inspect

    from generative_recommenders_amd.modules import contextualize_mlps as M
    from generative_recommenders_amd.ops.jagged_tensors import jagged_dense_bmm_broadcast_add

    assert list(inspect.signature(jagged_dense_bmm_broadcast_add).parameters) == [
        "max_seq_len", "seq_offsets", "jagged", "dense", "bias", "kernel"]
    m = M.ParameterizedContextualizedMLP(contextual_embedding_dim=48, sequential_input_dim=24, sequential_output_dim=40,
                                         hidden_dim=32)
    assert sorted(m.state_dict()) == sorted(
        [f"{p}.{w}" for p in ("_dense_features_compress", "_attn_raw_weights.0", "_attn_weights_norm", "_res_weights.0",
                              "_res_weights.1", "_res_weights.2") for w in ("weight", "bias")])
    s = M.SimpleContextualizedMLP(sequential_input_dim=24, sequential_output_dim=40, hidden_dim=32)
    assert sorted(s.state_dict()) == sorted([f"_mlp.{i}.{w}" for i in range(4) for w in ("weight", "bias")])
    assert issubclass(M.ParameterizedContextualizedMLP, M.ContextualizedMLP)


def test_shape_asserts_and_cpu_tensors_raise():
    import torch

    from generative_recommenders_amd.ops.jagged_tensors import jagged_dense_bmm_broadcast_add as f

    off = torch.tensor([0, 3, 5])
    j, d, b = torch.zeros(5, 8), torch.zeros(2, 8, 16), torch.zeros(2, 16)
    for args, msg in (((off, j, torch.zeros(2, 9, 16), b), r"wrong dense shape\[1\]"),
                      ((off[:2], j, d, b), r"wrong seq_offsets shape\[0\]"),
                      ((off, j, d, torch.zeros(3, 16)), r"wrong bias shape\[0\]"),
                      ((off, j, d, torch.zeros(2, 8)), r"wrong bias shape\[1\]")):
        with pytest.raises(Exception, match=msg):
            f(5, *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(5, off, j, d, b)


# ---- C ABI validation: every refusal happens before anything touches a device ------------------------------------------------
def _fwd_args(**kw):
    a = dict(jagged=64, jrs=8, dense=128, dbs=128, dks=16, dns=1, bias=None, bbs=16, out=256, ors=16, off=512, total=5,
             batch=2, k=8, n=16, ws=1024, dtype=0, idt=1)
    a.update(kw)
    return [a["jagged"], a["jrs"], a["dense"], a["dbs"], a["dks"], a["dns"], a["bias"], a["bbs"], a["out"], a["ors"], a["off"],
            a["total"], a["batch"], a["k"], a["n"], a["ws"], a["dtype"], a["idt"], None]


def _wgrad_args(**kw):
    a = dict(jagged=64, jrs=8, g=128, grs=16, dd=256, ddbs=128, ddks=16, db=None, dbbs=16, off=512, total=5, batch=2, k=8,
             n=16, dtype=0, idt=1)
    a.update(kw)
    return [a["jagged"], a["jrs"], a["g"], a["grs"], a["dd"], a["ddbs"], a["ddks"], a["db"], a["dbbs"], a["off"], a["total"],
            a["batch"], a["k"], a["n"], a["dtype"], a["idt"], None]


@pytest.mark.parametrize("bad, text", [
    (dict(jagged=None), "non-NULL"), (dict(dense=None), "non-NULL"), (dict(out=None), "non-NULL"), (dict(off=None), "non-NULL"),
    (dict(ws=None), "non-NULL"), (dict(k=0), "positive"), (dict(n=-4), "positive"), (dict(dtype=3), "dtype"),
    (dict(dtype=-1), "dtype"), (dict(idt=2), "int32 or int64"), (dict(k=12), "multiples of 8"), (dict(dtype=2, n=6), "multiples of 4"),
    (dict(jrs=12), "16-byte aligned"), (dict(jagged=66), "16-byte aligned"), (dict(dks=3, dns=5), "unit stride"),
    (dict(batch=-1), "negative"),
])
def test_fwd_refuses_bad_arguments(lib, bad, text):
    from generative_recommenders_amd import _lib

    assert lib.hstu_jagged_dense_bmm_fwd(*_fwd_args(**bad)) == -1      # HSTU_EINVAL
    assert text in lib.hstu_last_error().decode()
    with pytest.raises(RuntimeError, match="libhstu_hip error -1"):
        _lib.check(-1)


@pytest.mark.parametrize("bad, text", [
    (dict(jagged=None), "non-NULL"), (dict(g=None), "non-NULL"), (dict(dd=None), "non-NULL"), (dict(off=None), "non-NULL"),
    (dict(k=0), "positive"), (dict(n=0), "positive"), (dict(dtype=3), "dtype"), (dict(idt=-1), "int32 or int64"),
    (dict(n=20), "multiples of 8"), (dict(grs=18), "16-byte aligned"), (dict(ddks=8), "smaller than a row"),
])
def test_wgrad_refuses_bad_arguments(lib, bad, text):
    assert lib.hstu_jagged_dense_bmm_wgrad(*_wgrad_args(**bad)) == -1
    assert text in lib.hstu_last_error().decode()


def test_empty_batch_returns_ok_without_a_launch(lib):
    # no device exists in this test: a launch would fail, HSTU_OK means none was attempted
    assert lib.hstu_jagged_dense_bmm_fwd(*_fwd_args(batch=0, total=0)) == 0
    assert lib.hstu_jagged_dense_bmm_fwd(*_fwd_args(total=0)) == 0
    assert lib.hstu_jagged_dense_bmm_wgrad(*_wgrad_args(batch=0, total=0)) == 0


# ---- fixtures --------------------------------------------------------------------------------------------------------------
def test_fixture_set_covers_the_required_cases():
    cases = [load_op_case(p) for p in op_case_files()]
    assert len(cases) == 15
    for dt in ("float32", "bfloat16", "float16"):
        mine = [c for c in cases if c["dtype"] == dt]
        shapes = {c["dense"].shape[1:] for c in mine}
        assert {(37, 23), (200, 200), (64, 512)} <= shapes
        lens = [np.diff(c["seq_offsets"]) for c in mine]
        assert any((l == 0).any() for l in lens) and any((l == 1).any() for l in lens)
        assert any((l == c["max_seq_len"]).any() for l, c in zip(lens, mine))
        assert {c["seq_offsets"].dtype for c in mine} == {np.dtype(np.int32), np.dtype(np.int64)}
        assert any(int(c["dense_transposed"]) for c in mine)
    for f in os.listdir(FIXTURES):
        assert os.path.getsize(os.path.join(FIXTURES, f)) < 1 << 20


def test_fp64_helper_matches_reference_outputs_fp32():
    """the helper restates the op: against the reference's own fp32 results it may differ by fp32 rounding only"""
    n = 0
    for path in op_case_files():
        c = load_op_case(path)
        if c["dtype"] != "float32":
            continue
        ref = bmm_fp64(c["seq_offsets"], c["jagged"], c["dense"], c["bias"], c["d_out"])
        for name in OP_TENSORS:
            assert ref[name].shape == c[name].shape
            e = rel_fro(c[name], ref[name])
            assert e < 2e-6, f"{c['name']}: {name} rel_fro {e:.3e}"
        empty = np.flatnonzero(np.diff(c["seq_offsets"]) == 0)
        assert not ref["d_dense"][empty].any() and not ref["d_bias"][empty].any()
        n += 1
    assert n == 5


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree (build container only)")
def test_jagged_bmm_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    res = subprocess.run([sys.executable, os.path.join(FIXTURES, "make_jagged_bmm_golden.py"), "--out", str(tmp_path)], cwd=ROOT,
                         env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    committed = sorted(f for f in os.listdir(FIXTURES) if f.endswith(".npz"))
    fresh = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert committed == fresh, f"fixture sets differ: committed {committed}, regenerated {fresh}"
    for f in committed:
        a, b = np.load(os.path.join(FIXTURES, f)), np.load(os.path.join(tmp_path, f))
        assert sorted(a.files) == sorted(b.files), f"{f}: array names differ"
        for key in a.files:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, f"{f}:{key} dtype / shape"
            assert np.array_equal(a[key], b[key]), f"{f}:{key} is not reproduced bit for bit"
