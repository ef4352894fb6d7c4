"""CPU tests of RMS norm: the class table of tests/rms_norm_cases.py against the compiled csrc/norm_dispatch.h (every row lands
in its labelled class; the labels cover all five classes, forward and backward, in both dtype groups), the two C symbols and
their argument checks (which run before any launch), and the module's parameters."""

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import rms_norm_cases as T
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hstu_hip.h")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "norm_dispatch.h"
using namespace hstu::norm_dispatch;
int main() {
  char op[16];
  int eb, dim;
  unsigned long long a[4];
  while (scanf("%15s %d %d %llu %llu %llu %llu", op, &eb, &dim, &a[0], &a[1], &a[2], &a[3]) == 7) {
    const void* p[4];
    for (int i = 0; i < 4; ++i) p[i] = (const void*)(uintptr_t)a[i];
    RowClass k{0, false, false, false, 0};
    if (!strcmp(op, "rms_fwd")) k = rms_fwd_class(dim, eb, p[0], p[1], p[2]);
    else if (!strcmp(op, "rms_bwd")) k = rms_bwd_class(dim, eb, p[0], p[1], p[2], p[3]);
    else return 2;
    printf("%d %d %d %d %d %d\n", k.vec, (int)k.wide, (int)k.one_chunk, (int)k.gn_fast, k.limit, (int)refused(k, dim));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("rms_dispatch")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROGRAM)
    # -Wall -Werror, no HIP include path: the header must stand alone as plain C++
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(queries):
        out = subprocess.run([str(exe)], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout
        rows = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
        assert len(rows) == len(queries)
        return rows

    return run


def _addr(i, elems, eb):
    """role i of a call: its own 256-byte-aligned allocation, `elems` elements in"""
    return ((i + 1) << 20) + elems * eb


def _queries(c):
    eb = 2 if c["dt"] == "16" else 4
    res = []
    for d in ("fwd", "bwd"):
        roles = T.ROLES[f"rms_{d}"]
        addrs = [_addr(i, T.offset(c, r), eb) for i, r in enumerate(roles)] + [0] * (4 - len(roles))
        res.append((d, f"rms_{d} {eb} {c['dim']} " + " ".join(str(a) for a in addrs)))
    return res


def _label(out):
    vec, wide, one, fast, limit, refused = out
    assert not fast
    if refused:
        return T.REF
    return ("wide/" if wide else "narrow/") + ("scalar" if vec == 1 else ("vec-one" if one else "vec-max"))


def test_every_table_row_lands_in_its_labelled_class(ask):
    plan = [(c, d, q) for c in T.RMS_CASES for d, q in _queries(c)]
    got = ask([q for _, _, q in plan])
    for (c, d, _), out in zip(plan, got):
        assert _label(out) == c[d], f"{T.case_id(c)} {d}: labelled {c[d]}, dispatched to {_label(out)} {out}"
        V = T.VEC[c["dt"]]
        assert out[4] == (4096 if out[0] == V else 2048)


def test_the_table_covers_every_class():
    for dt in ("16", "32"):
        cases = [c for c in T.RMS_CASES if c["dt"] == dt]
        for d in ("fwd", "bwd"):
            seen = {c[d] for c in cases}
            assert T.REQUIRED <= seen, f"{dt}-bit {d}: no row for {sorted(T.REQUIRED - seen)}"
            assert T.REF in seen, f"{dt}-bit {d}: no refused row"
        assert {r for c in cases for r in c["mis"]} == {"x", "w", "y", "dy", "dx"}, f"{dt}-bit: a role is never misaligned"
        assert {1, 3, T.MANY_ROWS} <= {c["rows"] for c in cases}
        assert any(c["null_rstd"] for c in cases)
        dims = {c["dim"] for c in cases}
        assert {37, 513, 2047, 4096, 2049} <= dims and ({512, 520, 1024, 1032, 4104} if dt == "16" else {256, 260, 1024, 1028, 4100}) <= dims
    ids = [T.case_id(c) for c in T.RMS_CASES]
    assert len(ids) == len(set(ids))
    assert all(c["dim"] <= 64 for c in T.RMS_CASES if c["rows"] == T.MANY_ROWS) and all(c["rows"] <= 33 for c in T.RMS_CASES if c["rows"] != T.MANY_ROWS)


# ------------------------------------------------------------------------------------------------------ ABI and bindings
@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbols_exported_declared_and_bound(lib):
    from generative_recommenders_amd import _lib as L

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in (("hstu_rms_norm_fwd", 9), ("hstu_rms_norm_bwd", 11)):
        assert hasattr(lib, name), f"libhstu_hip.so does not export {name}"
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/hstu_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(L.SIGNATURES[name][1])
        assert L.SIGNATURES[name][0] is C.c_int
    assert lib.hstu_abi_version() == L.ABI_VERSION == 13


def test_argument_checks_fire_before_any_launch(lib):
    BF16, F32 = 0, 2
    buf = (C.c_char * 4096)()
    a = (C.addressof(buf) + 15) & ~15          # host memory: a kernel launched on it would fault, a check never reads it
    fwd = lambda x=a, w=a, y=a, rows=4, dim=64, dt=BF16: lib.hstu_rms_norm_fwd(x, w, y, None, rows, dim, 1e-5, dt, None)
    bwd = lambda dy=a, x=a, w=a, rstd=a, dx=a, dw=a, ws=a, rows=4, dim=64, dt=BF16: lib.hstu_rms_norm_bwd(
        dy, x, w, rstd, dx, dw, ws, rows, dim, dt, None)
    err = lambda: lib.hstu_last_error()
    assert fwd(rows=0) == 0                                     # nothing to do: no launch, no error
    for role in ("x", "w", "y"):
        assert fwd(**{role: None}) == -1 and b"NULL" in err(), role
    for role in ("dy", "x", "w", "rstd", "dx", "ws"):
        assert bwd(**{role: None}) == -1 and b"NULL" in err(), role
    assert bwd(dw=None) == -1 and b"dweight" in err()
    assert bwd(dw=None, rows=0) == -1 and b"dweight" in err()   # required even when there is nothing to sum
    assert fwd(dim=0) == -1 and b"positive" in err() and bwd(dim=-3) == -1 and b"positive" in err()
    # past the wide limit of each width: 16-byte pieces 4096, elements 2048 (odd dim, or one misaligned pointer)
    for call in (fwd, bwd):
        assert call(dim=4104) != 0 and b"exceeds the 4096" in err()
        assert call(dim=2049) != 0 and b"exceeds the 2048" in err()
        assert call(dim=2056, x=a + 2) != 0 and b"exceeds the 2048" in err()
        assert call(dim=4100, dt=F32) != 0 and b"exceeds the 4096" in err()
        assert call(dim=2052, dt=F32, x=a + 4) != 0 and b"exceeds the 2048" in err()


def test_module_owns_one_weight_of_ones():
    from generative_recommenders_amd.ops.layer_norm import RMSNorm, rms_norm

    m = RMSNorm(8)
    sd = m.state_dict()
    assert list(sd) == ["weight"] and sd["weight"].shape == (8,) and bool((sd["weight"] == 1).all())
    assert m._eps == 1e-5 and RMSNorm(4, eps=1e-6, is_inference=True).is_inference
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rms_norm(torch.zeros(4, 8), torch.ones(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 8))


# ------------------------------------------------------------------------------------------------------ the fixture
REFERENCE = "/root/reference/generative_recommenders"


def test_fixture_shapes_and_formulas():
    """tests/golden/rms_norm/rms_norm.npz without a GPU: two cases of the shapes the GPU test expects, a weight that is not
    all ones, and y / dx / dw that satisfy the op's formulas in fp64 (the fixture is fp32: 1e-5 relative)"""
    z = np.load(os.path.join(GOLDEN, "rms_norm", "rms_norm.npz"), allow_pickle=False)
    assert int(z["n_cases"]) == 2
    for i, shape in enumerate([(7, 37), (33, 520)]):
        x, w, g = (z[f"c{i}:{k}"].astype(np.float64) for k in ("x", "w", "g"))
        eps = float(z[f"c{i}:eps"])
        assert x.shape == shape and w.shape == shape[1:] and eps == np.float32(1e-5) and np.abs(w - 1).max() > 0.05
        rstd = 1.0 / np.sqrt((x * x).mean(axis=1, keepdims=True) + eps)
        xhat, wdy = x * rstd, w * g
        np.testing.assert_allclose(z[f"c{i}:y"], xhat * w, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(z[f"c{i}:dx"], (wdy - xhat * (xhat * wdy).mean(axis=1, keepdims=True)) * rstd, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(z[f"c{i}:dw"], (g * xhat).sum(axis=0), rtol=1e-5, atol=1e-5)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference tree (build container only)")
def test_fixture_regenerates_bit_identically(tmp_path):
    """as tests/test_golden_regen.py does for make_golden.py's fixtures"""
    res = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_rms_norm_golden.py"), "--out", str(tmp_path)], cwd=ROOT,
                         env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    a, b = np.load(os.path.join(GOLDEN, "rms_norm", "rms_norm.npz")), np.load(os.path.join(tmp_path, "rms_norm.npz"))
    assert sorted(a.files) == sorted(b.files)
    for key in a.files:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key
