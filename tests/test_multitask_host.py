"""CPU checks of the multitask prediction head: the fp64 restatement against the reference-minted fixtures, the module's
drop-in surface (names, enum, state_dict), the C entry points' declarations and argument validation (all before any
launch), and the reproducibility of the fixtures."""

import ctypes as C
import dataclasses
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import multitask_ref as R
from conftest import ROOT

REFERENCE = "/root/reference/generative_recommenders"
SYMBOLS = ("hstu_multitask_head_fwd", "hstu_multitask_head_bwd", "hstu_multitask_head_workspace_bytes")


def _prediction_fn(in_dim, num_tasks):
    from generative_recommenders_amd.ops.layer_norm import SwishLayerNorm

    return torch.nn.Sequential(torch.nn.Linear(in_dim, 512), SwishLayerNorm(512), torch.nn.Linear(512, num_tasks))


def _module(case, is_inference=False, prediction_fn=_prediction_fn):
    from generative_recommenders_amd.modules.multitask_module import DefaultMultitaskModule, MultitaskTaskType, TaskConfig

    configs = [TaskConfig(task_name=n, task_weight=1, task_type=MultitaskTaskType(t))
               for n, t in zip(case["task_names"], case["task_types"])]
    return DefaultMultitaskModule(task_configs=configs, embedding_dim=case["u"].shape[1], prediction_fn=prediction_fn,
                                  causal_multitask_weights=case["cmw"], is_inference=is_inference)


def test_fixture_set_covers_the_cases_of_the_issue():
    cases = [R.load_case(p) for p in R.case_files()]
    assert len(cases) == 7
    assert {c["u"].shape[0] for c in cases} == {1, 37, 200} and all(c["u"].shape[1] == 64 and c["cmw"] == 0.3 for c in cases)
    assert sorted((c["num_binary"], len(c["task_names"]) - c["num_binary"]) for c in cases) == \
        [(0, 1), (0, 1), (0, 2), (1, 0), (3, 0), (3, 2), (3, 2)]
    sums = [float(c["weight:" + n].sum()) for c in cases for n in c["weighted_tasks"]]
    assert any(s == 0.0 for s in sums) and any(0.0 < s < 1.0 for s in sums) and any(s > 1.0 for s in sums)
    assert any(len(c["weighted_tasks"]) < len(c["task_names"]) for c in cases)
    assert max(float(c["label:" + n].max()) for c in cases for n, t in zip(c["task_names"], c["task_types"]) if t == 0) > 1.0
    for c in cases:     # a relative gate needs a reference that is off the truth
        for tag in ("f32", "bf16"):
            for k in R.result_names():
                assert R.rel_fro(c[f"{tag}:{k}"], c["f64:" + k]) > 0.0, (c["name"], tag, k)


@pytest.mark.parametrize("path", R.case_files(), ids=lambda p: os.path.basename(p)[5:-4])
def test_restatement_equals_the_fp64_truth(path):
    """the fp64 restatement and the reference module run in fp64 differ by summation order only: fp64 unit round-off
    (1.1e-16) times a few hundred terms stays below 1e-12"""
    c = R.load_case(path)
    got = R.module_fp64(c["u"], c["i"], c["params"], c["labels_tl"], c["weights_tl"], c["num_binary"], c["cmw"], c["r"])
    for k in R.result_names():
        assert got[k].shape == c["f64:" + k].shape, k
        assert R.rel_fro(got[k], c["f64:" + k]) <= 1e-12, (k, R.rel_fro(got[k], c["f64:" + k]))


def test_head_restatement_is_the_tail_of_the_module_restatement():
    c = R.load_case(R.case_files()[5])
    p = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in c["params"].items()}
    h = (torch.from_numpy(c["u"].astype(np.float64)) * torch.from_numpy(c["i"].astype(np.float64))) @ p[R.PARAMS[0]].t() + p[R.PARAMS[1]]
    head = R.head_fp64(h, p[R.PARAMS[2]], p[R.PARAMS[3]], 1e-5, p[R.PARAMS[4]], p[R.PARAMS[5]], c["labels_tl"], c["weights_tl"],
                       c["num_binary"], c["cmw"], r=c["r"])
    for k, hk in (("preds", "preds"), ("losses", "losses"), ("gp:" + R.PARAMS[2], "dg"), ("gp:" + R.PARAMS[4], "dw"), ("gp:" + R.PARAMS[5], "dc")):
        assert R.rel_fro(head[hk], c["f64:" + k]) <= 1e-12, k


def test_module_surface_matches_the_reference_names():
    from generative_recommenders_amd.common import HammerModule
    from generative_recommenders_amd.modules import multitask_module as M

    names = R.load_names()
    assert [f"{e.name}={int(e)}" for e in M.MultitaskTaskType] == names["task_types"]
    assert [f.name for f in dataclasses.fields(M.TaskConfig)] == names["task_config_fields"]
    assert list(inspect.signature(M.DefaultMultitaskModule.__init__).parameters) == names["init_args"]
    assert list(inspect.signature(M.DefaultMultitaskModule.forward).parameters) == names["forward_args"]
    assert list(inspect.signature(M.MultitaskModule.forward).parameters) == names["base_forward_args"]
    assert issubclass(M.DefaultMultitaskModule, M.MultitaskModule) and issubclass(M.MultitaskModule, HammerModule)
    c = R.load_case(R.case_files()[0])
    assert [k.replace(".0.", ".X.").replace(".1.", ".Y.").replace(".2.", ".Z.") for k in _module(c).state_dict()] == \
        [k.replace(".0.", ".X.").replace(".1.", ".Y.").replace(".2.", ".Z.") for k in names["state_dict_keys"]]
    assert list(_module(c).state_dict()) == names["state_dict_keys"] == list(R.PARAMS)


def test_constructor_asserts_as_the_reference():
    from generative_recommenders_amd.modules.multitask_module import DefaultMultitaskModule, MultitaskTaskType, TaskConfig

    reg = TaskConfig("vvp", 2, MultitaskTaskType.REGRESSION)
    click = TaskConfig("is_click", 1, MultitaskTaskType.BINARY_CLASSIFICATION)
    with pytest.raises(AssertionError, match="sorted by task_type"):
        DefaultMultitaskModule([reg, click], 8, _prediction_fn, 1.0, False)
    with pytest.raises(AssertionError, match="non-empty"):
        DefaultMultitaskModule([], 8, _prediction_fn, 1.0, False)
    m = DefaultMultitaskModule([click, click, reg], 8, _prediction_fn, 0.3, False)
    assert m._task_offsets == [0, 2, 3] and m._has_multiple_task_types and m._prediction_module[2].out_features == 3
    assert not DefaultMultitaskModule([reg], 8, _prediction_fn, 0.3, True)._has_multiple_task_types


@pytest.mark.parametrize("path", R.case_files(), ids=lambda p: os.path.basename(p)[5:-4])
def test_strict_load_of_the_fixture_parameters(path):
    c = R.load_case(path)
    m = _module(c)
    res = m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c["params"].items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m._prediction_module[2].weight.detach(), torch.from_numpy(np.ascontiguousarray(c["params"][R.PARAMS[4]])))


def test_cpu_tensors_are_refused_by_the_op():
    from generative_recommenders_amd.ops.multitask import multitask_head

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        multitask_head(torch.zeros(4, 64), torch.ones(64), torch.zeros(64), 1e-5, torch.zeros(2, 64), torch.zeros(2), None, None, 1, 1.0)


# ------------------------------------------------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbols_declared_exported_and_in_the_signature_table(lib):
    from generative_recommenders_amd import _lib
    from generative_recommenders_amd.ops import _launch

    header = open(os.path.join(ROOT, "include", "hstu_hip.h")).read()
    internal = open(os.path.join(ROOT, "generative_recommenders_amd", "csrc", "capi_internal.h")).read()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert name.replace("hstu_", "") in internal, name
    assert "multitask_module.py:" in header and "dlrm_hstu.py:139-149" in header       # the reference lines it replaces
    consts = {k: int(v) for k, v in re.findall(r"#define HSTU_MULTITASK_(\w+) (\d+)", header)}
    assert consts == {"MAX_TASKS": _launch.MULTITASK_MAX_TASKS, "MAX_BLOCKS": _launch.MULTITASK_MAX_BLOCKS,
                      "ROWS_PER_BLOCK": _launch.MULTITASK_ROWS_PER_BLOCK}
    assert _lib.ABI_VERSION == 13 == lib.hstu_abi_version()


def test_workspace_bytes_do_not_depend_on_rows(lib):
    from generative_recommenders_amd.ops import _launch

    ws = lib.hstu_multitask_head_workspace_bytes
    assert len(inspect.signature(lambda dim, num_tasks: None).parameters) == len(ws.argtypes) == 2    # (dim, num_tasks): no rows
    per_block = lambda dim, t: ((t + 2) * dim + _launch.MULTITASK_MAX_TASKS) * 4
    for dim, t in ((64, 1), (512, 5), (520, 8), (4096, 8)):
        assert ws(dim, t) == _launch.MULTITASK_MAX_BLOCKS * per_block(dim, t)
    assert ws(512, 8) > ws(512, 1) and ws(0, 1) == 0


def test_entry_points_refuse_bad_arguments_with_a_message(lib):
    BF16, F32 = 0, 2
    buf = (C.c_char * 65536)()
    a = (C.addressof(buf) + 15) & ~15

    def fwd(x=a, x_rs=None, tasks=5, nbin=3, dim=512, dt=BF16, rows=4, labels=a, preds=a, ws=a, w=a):
        return lib.hstu_multitask_head_fwd(x, max(dim, 1) if x_rs is None else x_rs, a, a, 1e-5, w, a, labels, None, a, preds, a, a, a, a, ws, rows, dim, tasks, nbin,
                                           0.3, dt, None)

    def bwd(x=a, x_rs=None, tasks=5, nbin=3, dim=512, dt=BF16, rows=4, dx=a, dx_rs=None, dw=a, gl=a):
        return lib.hstu_multitask_head_bwd(gl, a, x, max(dim, 1) if x_rs is None else x_rs, a, a, a, a, None, a, a, a, a, dx,
                                           max(dim, 1) if dx_rs is None else dx_rs, dw, a, a, a, a, rows, dim, tasks,
                                           nbin, 0.3, dt, None)

    err = lambda: lib.hstu_last_error()
    for call in (fwd, bwd):
        assert call(tasks=0) == -1 and b"num_tasks must be in [1, 8]" in err()
        assert call(tasks=9) == -1 and b"num_tasks must be in [1, 8]" in err()
        assert call(tasks=3, nbin=4) == -1 and b"num_binary" in err()
        assert call(nbin=-1) == -1 and b"num_binary" in err()
        assert call(x=a + 1) == -1 and b"aligned" in err()                     # not even element aligned
        assert call(dt=7) == -1 and b"dtype" in err()
        assert call(dim=0) == -1 and b"dim must be positive" in err()
        assert call(dim=4104) == -1 and b"exceeds the 4096" in err()           # rows of 16-byte pieces
        assert call(dim=2049) == -1 and b"exceeds the 2048" in err()           # an odd dim: element by element
        assert call(x=a + 2, dim=2056) == -1 and b"exceeds the 2048" in err()  # ... or a row that starts off a 16-byte boundary
        assert call(dim=1024, x_rs=512, dt=F32) == -1 and b"row stride" in err()
    assert fwd(ws=a + 4) == -1 and b"workspace must be 16-byte aligned" in err()
    assert fwd(w=a + 2) == -1 and b"4-byte aligned" in err()
    assert fwd(preds=None) == -1 and b"non-NULL" in err()
    assert fwd(x_rs=100) == -1 and b"row stride" in err()
    assert bwd(dx_rs=8) == -1 and b"row stride" in err()
    assert bwd(dw=None) == -1 and b"required" in err()
    assert bwd(dx=None) == -1 and b"non-NULL" in err()
    # the inference form without rows needs nothing at all
    assert lib.hstu_multitask_head_fwd(None, 512, None, None, 1e-5, None, None, None, None, None, None, None, None, None, None,
                                       None, 0, 512, 5, 3, 0.3, BF16, None) == 0


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree (build container only)")
def test_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    res = subprocess.run([sys.executable, "-W", "ignore", os.path.join(R.FIXTURES, "make_multitask_golden.py"), "--out", str(tmp_path)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    committed = sorted(f for f in os.listdir(R.FIXTURES) if f.endswith(".npz"))
    fresh = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert committed == fresh and len(committed) == 8
    for f in committed:
        assert os.path.getsize(os.path.join(R.FIXTURES, f)) <= 1 << 20, f
        a, b = np.load(os.path.join(R.FIXTURES, f)), np.load(os.path.join(tmp_path, f))
        assert sorted(a.files) == sorted(b.files), f
        for key in a.files:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, f"{f}:{key} dtype / shape"
            assert np.array_equal(a[key], b[key]), f"{f}:{key} is not reproduced bit for bit"
