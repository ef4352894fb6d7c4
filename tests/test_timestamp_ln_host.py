"""CPU checks of the timestamp postprocessor's row pass: the ABI and its new symbols, argument validation of the C entry
points (all before any launch, so it runs without a GPU), the workspace query, the fp32 numpy restatement of the time
features against the reference-minted fixtures, the new norm_dispatch class functions compiled alone, the module's drop-in
surface and the reproducibility of the fixtures."""

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import timestamp_ln_ref as R
from conftest import ROOT

REFERENCE = "/root/reference/generative_recommenders"
CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")
SYMBOLS = ("hstu_time_features", "hstu_time_ln_workspace_bytes", "hstu_time_ln_fwd", "hstu_time_ln_bwd")
CASES = R.case_files()


@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


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
    assert "postprocessors.py:105-176" in header and "dlrm_hstu.py:182-191" in header       # the reference lines it replaces
    consts = {k: int(v) for k, v in re.findall(r"#define HSTU_TIME_LN_(\w+) (\d+)", header)}
    assert consts == {"MAX_PERIODS": _launch.TIME_LN_MAX_PERIODS, "MAX_BLOCKS": 1024}
    assert "#define HSTU_TIME_FEATURES_MAX_PERIODS 1024" in header
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "time_ln_ops.hip" in makefile


def test_workspace_query_is_monotone_in_dim_and_periods(lib):
    ws = lib.hstu_time_ln_workspace_bytes
    assert len(ws.argtypes) == 2                                            # (dim, num_periods): independent of rows
    for f in (1, 2, 3, 4):
        sizes = [ws(d, f) for d in (1, 37, 40, 512, 1536, 4096)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes) and sizes[0] > 0
    for d in (37, 512, 4096):
        sizes = [ws(d, f) for f in (1, 2, 3, 4)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert ws(512, 2) == 1024 * (3 + 4) * 512 * 4                           # one partial row per workgroup, 3 + 2F column sums
    assert ws(0, 2) == 0 and ws(512, 0) == 0 and ws(512, 5) == 0


def test_entry_points_refuse_bad_arguments_with_a_message(lib):
    BF16, F32 = 0, 2
    buf = (C.c_char * 65536)()
    a = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.hstu_last_error()

    def feats(t=a, pu=a, upp=a, f=2, out=a, rows=4):
        return lib.hstu_time_features(t, pu, upp, f, out, rows, None)

    def fwd(z0=a, t=a, pu=a, f=2, b=a, wt=a, g=a, h=a, y=a, rows=4, dim=512, dt=BF16):
        return lib.hstu_time_ln_fwd(z0, t, pu, a, f, b, wt, g, h, 1e-5, y, a, a, rows, dim, dt, None)

    def bwd(dy=a, z0=a, t=a, pu=a, f=2, b=a, wt=a, g=a, mean=a, dz=a, dg=a, dwt=a, ws=a, rows=4, dim=512, dt=BF16):
        return lib.hstu_time_ln_bwd(dy, z0, t, pu, a, f, b, wt, g, mean, a, dz, dg, a, a, dwt, ws, rows, dim, dt, None)

    assert feats(f=0) == -1 and b"num_periods must be in [1, 1024]" in err()    # alone, the feature kernel takes any F
    for call in (fwd, bwd):
        assert call(f=0) == -1 and b"num_periods must be in [1, 4]" in err()
        assert call(f=5) == -1 and b"num_periods must be in [1, 4]" in err()
    for call in (feats, fwd, bwd):
        assert call(rows=-1) == -1 and b"negative rows" in err()
        assert call(pu=None) == -1 and b"non-NULL" in err()
        assert call(t=None) == -1 and b"non-NULL" in err()
        assert call(t=a + 4) == -1 and b"aligned" in err()
    for call in (fwd, bwd):
        assert call(dt=7) == -1 and b"dtype" in err()
        assert call(dim=0) == -1 and b"dim must be positive" in err()
        assert call(dim=4104) == -2 and b"exceeds the 4096" in err()           # rows of 16-byte pieces
        assert call(dim=2049) == -2 and b"exceeds the 2048" in err()           # an odd dim: element by element
        assert call(z0=a + 2, dim=2056) == -2 and b"exceeds the 2048" in err()  # ... or rows that start off a 16-byte boundary
        assert call(wt=a + 4, dim=2056) == -2 and b"exceeds the 2048" in err()  # ... or parameters that do
        assert call(dim=4100, dt=F32) == -2 and b"exceeds the 4096" in err()
        assert call(z0=a + 1) == -1 and b"aligned" in err()                     # not even element aligned
        assert call(b=None) == -1 and b"non-NULL" in err()
        assert call(wt=None) == -1 and b"non-NULL" in err()
        assert call(g=None) == -1 and b"non-NULL" in err()
        assert call(z0=None) == -1 and b"non-NULL" in err()
    assert feats(out=None) == -1 and b"non-NULL" in err()
    assert fwd(h=None) == -1 and b"non-NULL" in err()
    assert fwd(y=None) == -1 and b"non-NULL" in err()
    assert bwd(dy=None) == -1 and b"non-NULL" in err()
    assert bwd(dz=None) == -1 and b"non-NULL" in err()
    assert bwd(mean=None) == -1 and b"non-NULL" in err()
    assert bwd(ws=None) == -1 and b"non-NULL" in err()
    assert bwd(ws=a + 4) == -1 and b"aligned" in err()
    assert bwd(dg=None) == -1 and b"required" in err()
    assert bwd(dwt=None) == -1 and b"required" in err()
    # no rows: nothing is read, nothing launched
    assert feats(t=None, out=None, rows=0) == 0
    assert fwd(z0=None, t=None, y=None, rows=0) == 0


# ------------------------------------------------------------------------------------------------------------ time features
def test_fixture_set_covers_the_cases_of_the_issue():
    cases = [R.load_case(p) for p in CASES]
    assert [(c["x"].shape, len(c["periods"])) for c in cases] == \
        [((23, 40), 2), ((11, 37), 1), ((70, 512), 2), ((9, 1536), 3), ((5, 64), 4), ((1, 40), 2)]
    assert cases[4]["periods"] == [(3600, 24), (86400, 7), (86400, 365), (60, 60)]
    assert [c["tags"] for c in cases] == [["f32", "bf16", "f64"], ["f32", "bf16", "f64"], ["bf16", "f64"], ["bf16", "f64"],
                                          ["f32", "f64"], ["f32", "bf16", "f64"]]
    full = set(cases[0]["timestamps"].tolist()) | set(cases[2]["timestamps"].tolist())
    assert {0, 1, 3599, 3600} <= full and max(full) > 2**33
    k = 472000
    assert {k * 3600 - 1, k * 3600, k * 3600 + 1, k * 3600 - 64, k * 3600 + 64} <= full
    assert sum(1_600_000_000 <= t < 1_760_000_000 for t in cases[2]["timestamps"].tolist()) >= 48
    for c in cases:
        assert c["time_features"].dtype == np.float32 and c["time_features"].shape == (c["x"].shape[0], 2 * len(c["periods"]))
        for tag in c["tags"][:-1]:     # a relative gate needs a reference that is off the truth
            for name in R.result_names():
                exact = c["x"].shape[0] == 1 and tag == "f32" and name == "gp:_layer_norm.bias"      # one row: r itself
                assert (R.rel_fro(c[f"{tag}:{name}"], c["f64:" + name]) > 0.0) != exact, (c["name"], tag, name)


@pytest.mark.parametrize("path", CASES, ids=R.case_id)
def test_fp32_restatement_reproduces_buckets_and_angles_bit_for_bit(path):
    c = R.load_case(path)
    units, angles = R.time_buckets_and_angles(c["timestamps"], c["periods"])
    assert units.dtype == np.float32 and np.array_equal(units.view(np.uint32), c["units"].view(np.uint32))
    assert angles.dtype == np.float32 and np.array_equal(angles.view(np.uint32), c["angles"].view(np.uint32))
    # cos / sin: numpy's against torch.polar's -- libm noise (1e-7), two orders under the smallest bucket step (2 * 3.14 / 365)
    assert np.abs(R.time_features(c["timestamps"], c["periods"]) - c["time_features"]).max() <= 1e-6


@pytest.mark.parametrize("path", CASES, ids=R.case_id)
def test_fixtures_catch_the_two_obvious_kernels(path):
    """plain floorf(a / b) and exact integer arithmetic each move at least one timestamp of every case into another hour"""
    c = R.load_case(path)
    hour = [i for i, (p, _) in enumerate(c["periods"]) if p == 3600]
    assert hour, "every case has the hour-of-day period"
    t = c["timestamps"]
    ref = c["units"][:, hour[0]]
    plain = np.floor(t.astype(np.float32) / np.float32(3600))
    assert (plain != ref).any() and ((t // 3600).astype(np.float64) != ref).any()


# ------------------------------------------------------------------------------------------------------------ the dispatch
PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "norm_dispatch.h"
using namespace hstu::norm_dispatch;
int main() {
  char op[8];
  int eb, dim;
  unsigned long long a[6];
  while (scanf("%7s %d %d %llu %llu %llu %llu %llu %llu", op, &eb, &dim, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 9) {
    const void* p[6];
    for (int i = 0; i < 6; ++i) p[i] = (const void*)(uintptr_t)a[i];
    const RowClass k = !strcmp(op, "fwd") ? time_ln_fwd_class(dim, eb, p[0], p[1], p[2], p[3], p[4], p[5])
                                          : time_ln_bwd_class(dim, eb, p[0], p[1], p[2], p[3], p[4], p[5]);
    printf("%d %d %d %d %d\n", k.vec, (int)k.wide, (int)k.one_chunk, k.limit, (int)refused(k, dim));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("time_ln_dispatch")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROGRAM)
    # -Wall -Werror, no HIP include path: the header must stand alone as plain C++
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(op, eb, dim, spoil=None, by=0):
        addrs = [((i + 1) << 20) + (by if i == spoil else 0) for i in range(6)]
        out = subprocess.run([str(exe)], input=f"{op} {eb} {dim} " + " ".join(map(str, addrs)) + "\n", capture_output=True,
                             text=True, check=True).stdout
        return tuple(int(x) for x in out.split())

    return run


@pytest.mark.parametrize("op", ["fwd", "bwd"])
def test_time_ln_classes(ask, op):
    # (vec, wide, one_chunk, limit, refused)
    assert ask(op, 2, 37) == (1, 0, 0, 2048, 0)              # scalar
    assert ask(op, 2, 40) == (8, 0, 1, 4096, 0)              # vector pieces, one chunk
    assert ask(op, 2, 512) == (8, 0, 1, 4096, 0)             # vector and narrow: the DLRM row, one chunk
    assert ask(op, 2, 1024) == (8, 0, 0, 4096, 0)            # narrow, two chunks
    assert ask(op, 2, 1536) == (8, 1, 0, 4096, 0)            # wide
    assert ask(op, 2, 4104) == (8, 1, 0, 4096, 1)            # refused
    assert ask(op, 4, 64) == (4, 0, 1, 4096, 0) and ask(op, 4, 1028) == (4, 1, 0, 4096, 0)
    assert ask(op, 2, 600, spoil=None) == (8, 0, 0, 4096, 0)
    for role in range(6):       # every pointer the kernels read in pieces is a fact of the class
        assert ask(op, 2, 600, spoil=role, by=4) == (1, 1, 0, 2048, 0), role
        assert ask(op, 2, 2056, spoil=role, by=4)[4] == 1, role


# ------------------------------------------------------------------------------------------------------------ the module
def test_module_surface_matches_the_reference():
    from generative_recommenders_amd.modules.postprocessors import OutputPostprocessor, TimestampLayerNormPostprocessor

    m = TimestampLayerNormPostprocessor(embedding_dim=40, time_duration_features=[(3600, 24), (86400, 7)], eps=1e-5)
    assert isinstance(m, OutputPostprocessor) and not m._is_inference
    c = R.load_case(CASES[0])
    assert list(m.state_dict()) == [str(k) for k in c["sd_keys"]]
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in c["param_keys"]] == list(R.PARAMS)
    assert m._period_units.tolist() == [[3600.0, 86400.0]] and m._units_per_period.tolist() == [[24.0, 7.0]]
    assert m._period_units.dtype == torch.float32 and m._time_feature_combiner.weight.shape == (40, 44)
    assert float(m._time_feature_combiner.bias.detach().abs().max()) == 0.0          # init_mlp_weights_optional_bias
    bound = (6.0 / (40 + 44)) ** 0.5
    assert float(m._time_feature_combiner.weight.detach().abs().max()) <= bound       # Xavier-uniform
    res = m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(c["sd:" + k])) for k in m.state_dict()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    import generative_recommenders_amd.modules.postprocessors as P
    assert "is not mirrored" not in P.__doc__


def test_cpu_tensors_are_refused_by_the_op():
    from generative_recommenders_amd.ops.timestamp_layer_norm import timestamp_layer_norm

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        timestamp_layer_norm(torch.zeros(4, 40), torch.zeros(4, dtype=torch.int64), torch.zeros(40, 44), torch.zeros(40),
                             torch.ones(40), torch.zeros(40), torch.tensor([[3600.0, 86400.0]]), torch.tensor([[24.0, 7.0]]))


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree (build container only)")
def test_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    maker = os.path.join(ROOT, "tests", "golden", "dlrm_hstu", "make_dlrm_hstu_golden.py")
    res = subprocess.run([sys.executable, "-W", "ignore", maker, "--out", str(tmp_path / "model"), "--op-out", str(tmp_path / "op")],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    for committed_dir, fresh_dir in ((R.FIXTURES, tmp_path / "op"), (os.path.join(ROOT, "tests", "golden", "dlrm_hstu"), tmp_path / "model")):
        committed = sorted(f for f in os.listdir(committed_dir) if f.endswith(".npz"))
        fresh = sorted(f for f in os.listdir(fresh_dir) if f.endswith(".npz"))
        assert committed == fresh and committed
        for f in committed:
            assert os.path.getsize(os.path.join(committed_dir, f)) <= 1 << 20, f
            a, b = np.load(os.path.join(committed_dir, f)), np.load(os.path.join(fresh_dir, f))
            assert sorted(a.files) == sorted(b.files), f
            for key in a.files:
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, f"{f}:{key} dtype / shape"
                assert np.array_equal(a[key], b[key]), f"{f}:{key} is not reproduced bit for bit"
