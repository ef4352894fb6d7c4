"""CPU tests of csrc/norm_dispatch.h, the one place that decides which instantiation of a row-norm kernel a call runs:
piece width from ALL the facts the kernels depend on, then narrow / wide from dim at that width, refusal only past the
wide limit.  A few-line program is compiled against the header alone (it is plain C++) and answers queries:
  * an exhaustive sweep of dim 1 .. 4200 x element size x "one fact spoils the vector width" patterns,
  * the parent commit's rule restated -- every call it accepted keeps its class; what it refused and is accepted now are
    exactly the scalar rows of 513 .. 1024 elements that the wide instance holds,
  * the class table of tests/norm_class_cases.py: every row lands in its labelled class, and the labels cover every launch
    line of ln_fwd, ln_bwd, nm_fwd, nm_bwd, l2_launch and silu_launch."""

import os
import subprocess

import pytest

import norm_class_cases as T
from conftest import ROOT

CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "norm_dispatch.h"
using namespace hstu::norm_dispatch;
int main() {
  char op[16];
  int eb, dim, heads, hd, gn;
  long long sa, sb, sc;
  unsigned long long a[7];
  while (scanf("%15s %d %d %d %d %d %lld %lld %lld %llu %llu %llu %llu %llu %llu %llu", op, &eb, &dim, &heads, &hd, &gn, &sa, &sb, &sc,
               &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]) == 16) {
    const void* p[7];
    for (int i = 0; i < 7; ++i) p[i] = (const void*)(uintptr_t)a[i];
    RowClass k{0, false, false, false, 0};
    if (!strcmp(op, "ln_fwd")) k = ln_fwd_class(dim, eb, p[0], p[1], p[2], p[3]);
    else if (!strcmp(op, "ln_bwd")) k = ln_bwd_class(dim, eb, p[0], p[1], p[2], p[3], p[4], p[5]);
    else if (!strcmp(op, "nm_fwd")) k = nm_fwd_class(heads, hd, eb, gn != 0, p[0], p[1], sa, p[2], p[3], p[4]);
    else if (!strcmp(op, "nm_bwd")) k = nm_bwd_class(heads, hd, eb, gn != 0, p[0], p[1], p[2], sa, p[3], p[4], p[5], p[6], sb);
    else if (!strcmp(op, "l2_fwd") || !strcmp(op, "l2_bwd")) k = l2_class(dim, eb, p[0], p[1], p[2]);
    else if (!strcmp(op, "silu_fwd") || !strcmp(op, "silu_bwd")) k.vec = silu_vector(eb, dim, p[0], p[1], p[2], sa, sb, sc) ? 16 / eb : 1;
    else return 2;
    const bool row_op = strncmp(op, "silu", 4) != 0;
    printf("%d %d %d %d %d %d\n", k.vec, (int)k.wide, (int)k.one_chunk, (int)k.gn_fast, k.limit, (int)(row_op && refused(k, dim)));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("norm_dispatch")
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


def _query(op, eb, dim, heads, hd, gn, strides, addrs):
    s = list(strides) + [0] * (3 - len(strides))
    a = list(addrs) + [0] * (7 - len(addrs))
    return f"{op} {eb} {dim} {heads} {hd} {int(gn)} {s[0]} {s[1]} {s[2]} " + " ".join(str(x) for x in a)


# ------------------------------------------------------------------------------------------------------ the sweep
# which roles each launcher's kernels touch in 16-byte pieces (group norm reads weight / bias as scalars per head), and
# the pointers the PARENT commit's norm_wide() looked at before the launcher computed the width from all of them
ROLES = {"ln_fwd": ("x", "w", "b", "y"), "ln_bwd": ("dy", "x", "w", "b", "dres", "dx"), "nm_fwd": ("attn", "u", "w", "b", "y"),
         "nm_bwd": ("dy", "attn", "u", "w", "b", "dattn", "du"), "l2_fwd": ("x", "g", "y"), "l2_bwd": ("x", "dy", "dx")}
PARENT_SAW = {"ln_fwd": [("x", "y", "w")], "ln_bwd": [("dy", "x", "dx")], "nm_fwd": [("attn", "u", "y")],
              "nm_bwd": [("attn", "u", "dy"), ("dattn", "du")], "l2_fwd": [("x", "y")], "l2_bwd": [("x", "dy", "dx")]}


def _capacity(vec, wide):
    return (4 if wide else 1) * (512 if vec == 1 else 1024)


def _parent_rule(op, dim, V, vec, spoiled_role):
    """the parent commit: wide iff dim > (1024 if dim % V == 0 and the pointers norm_wide() saw are aligned else 512),
    for nm_bwd the OR over its two calls; then the instance's check_dim refuses dim > its capacity at the launcher's width"""
    wide = any(dim > (1024 if dim % V == 0 and spoiled_role not in seen else 512) for seen in PARENT_SAW[op])
    return wide, dim > _capacity(vec, wide)


def _sweep_patterns():
    """(op, gn heads or 0, kind, which): kind 'none' | 'ptr' (role `which` one element off) | 'ustride' | 'dustride'"""
    pats = []
    for op, roles in ROLES.items():
        for heads in ((0,) if not op.startswith("nm") else (0, 2, 8)):     # 0: layer norm
            pats.append((op, heads, "none", None))
            pats += [(op, heads, "ptr", r) for r in roles if not (op == "l2_fwd" and r == "g")]
            if op.startswith("nm"):
                pats.append((op, heads, "ustride", None))
            if op == "nm_bwd":
                pats.append((op, heads, "dustride", None))
    return pats


@pytest.mark.parametrize("eb", [2, 4])
def test_exhaustive_sweep(ask, eb):
    V = 16 // eb
    queries, expect = [], []
    for op, gheads, kind, which in _sweep_patterns():
        roles = ROLES[op]
        for dim in range(1, 4201):
            heads = gheads or 1
            if dim % heads:
                continue
            hd = dim // heads
            gn = gheads > 0
            addrs = [_addr(i, 64 + (1 if (kind == "ptr" and r == which) else 0), eb) for i, r in enumerate(roles)]
            if op == "l2_fwd":
                addrs[1] = 0
            us = dim + (1 if kind == "ustride" else 0)
            ds = dim + (1 if kind == "dustride" else 0)
            queries.append(_query(op, eb, dim, heads, hd, gn, (us, ds), addrs))
            spoils = kind in ("ustride", "dustride") or (kind == "ptr" and not (gn and which in ("w", "b")))
            vector = dim % V == 0 and not spoils and not (gn and hd % V)
            expect.append((op, dim, hd, gn, vector, which if kind == "ptr" else None))
    got = ask(queries)
    newly_accepted = set()
    for (op, dim, hd, gn, vector, spoiled), (vec, wide, one, fast, limit, refused) in zip(expect, got):
        what = (op, dim, hd, gn, spoiled)
        assert vec == (V if vector else 1), what
        assert limit == (4096 if vector else 2048), what
        assert bool(refused) == (dim > limit), what                                # (a)
        assert bool(wide) == (dim > (1024 if vector else 512)), what               # (b)
        assert bool(one) == (vector and dim <= 64 * V), what
        lph = hd // V
        assert bool(fast) == (gn and vector and lph <= 64 and lph & (lph - 1) == 0), what
        old_wide, old_refused = _parent_rule(op, dim, V, vec, spoiled)             # (c)
        if not old_refused:
            assert not refused and bool(wide) == old_wide, what                    # every accepted call keeps its class
        elif not refused:
            assert vec == 1 and 512 < dim <= 1024 and wide, what                   # the hole: a row the wide instance holds
            newly_accepted.add(op)
    # the hole was in every launcher whose width depends on a fact norm_wide() did not see (l2 norm: it saw them all)
    assert newly_accepted == {"ln_fwd", "ln_bwd", "nm_fwd", "nm_bwd"}


def test_fully_aligned_inputs_keep_the_parent_class(ask):
    """(c) in its plain form: 16-byte-aligned tensors, dense strides, layer norm -- dim alone decides, as it always did"""
    for eb in (2, 4):
        V = 16 // eb
        dims = range(1, 4201)
        for op, roles in ROLES.items():
            addrs = [0 if (op == "l2_fwd" and r == "g") else _addr(i, 64, eb) for i, r in enumerate(roles)]
            got = ask([_query(op, eb, d, 1, d, False, (d, d), addrs) for d in dims])
            for d, (vec, wide, one, fast, limit, refused) in zip(dims, got):
                old_vec = V if d % V == 0 else 1
                old_wide = d > (1024 if d % V == 0 else 512)
                assert (vec, bool(wide), bool(refused)) == (old_vec, old_wide, d > _capacity(old_vec, old_wide)), (op, eb, d)


# ------------------------------------------------------------------------------------------------------ the class table
def _label(c, op, out):
    vec, wide, one, fast, limit, refused = out
    if op.startswith("silu"):
        return "scalar" if vec == 1 else "vec"
    if refused:
        return T.REF
    inst = "wide/" if wide else "narrow/"
    if op.startswith("l2"):
        return inst + ("scalar" if vec == 1 else "vec")
    if op.startswith("ln"):
        return inst + ("scalar" if vec == 1 else ("vec-one" if one else "vec-max"))
    norm = "gn" if c["gn"] else "ln"       # the order of the launch lines in nm_fwd / nm_bwd
    kernel = ("gn-fast-one" if fast and one else "gn-fast-max" if fast else f"{norm}-scalar" if vec == 1 else f"{norm}-vec")
    return inst + kernel + ("/silu" if c["silu"] else "/plain")


def _case_queries(c):
    """the forward and the backward call of a table row as the GPU test lays them out"""
    eb = 2 if c["dt"] == "16" else 4
    swish = c["op"] == "swish"
    fam = {"ln": "ln", "swish": "ln"}.get(c["op"], c["op"])
    res = []
    for d in ("fwd", "bwd"):
        op = f"{fam}_{d}"
        roles = T.ROLES[op]
        absent = {"ln_bwd": {"b"} - ({"b"} if swish else set()) | (set() if c["res"] else {"dres"}), "l2_fwd": {"g"},
                  "silu_fwd": {"dout"}}.get(op, set())
        addrs = [0 if r in absent else _addr(i, T.offset(c, r), eb) for i, r in enumerate(roles)]
        if fam == "silu":
            strides = (c["dim"] if d == "bwd" else 0, c["ustride"], c["dustride"])
        else:
            strides = (c["ustride"], c["dustride"])
        res.append((d, op, _query(op, eb, c["dim"], c["heads"], c["hd"], c["gn"], strides, addrs)))
    return res


def test_every_table_row_lands_in_its_labelled_class(ask):
    plan = [(c, d, op, q) for c in T.CASES for d, op, q in _case_queries(c)]
    got = ask([q for _, _, _, q in plan])
    for (c, d, op, _), out in zip(plan, got):
        assert _label(c, op, out) == c[d], f"{T.case_id(c)} {d}: labelled {c[d]}, dispatched to {_label(c, op, out)} {out}"


def test_the_table_covers_every_launch_line():
    for dt in ("16", "32"):
        seen = {}
        for c in T.CASES:
            if c["dt"] != dt:
                continue
            for d in ("fwd", "bwd"):
                seen.setdefault((c["op"], d), set()).add(c[d])
                if c["op"] == "ln" and c["res"] and d == "bwd":
                    seen.setdefault(("ln+res", d), set()).add(c[d])
        for key, lines in T.REQUIRED.items():
            assert lines <= seen.get(key, set()), f"{dt}-bit {key}: no row for {sorted(lines - seen.get(key, set()))}"
            assert T.REF in seen[key] or key[0] == "silu", f"{dt}-bit {key}: no refused row"
    ids = [T.case_id(c) for c in T.CASES]
    assert len(ids) == len(set(ids))
    # every scalar cause at least once per op: each role of each launcher, the two strides, group norm's head_dim
    for fam, ops in (("ln", ("ln_fwd", "ln_bwd")), ("swish", ("ln_fwd", "ln_bwd")), ("nm", ("nm_fwd", "nm_bwd")), ("l2", ("l2_fwd", "l2_bwd")),
                     ("silu", ("silu_fwd", "silu_bwd"))):
        want = {r for op in ops for r in T.ROLES[op]} - {"g"} - ({"dres"} if fam == "swish" else set())
        have = {r for c in T.CASES if c["op"] == fam for r in c["mis"]}
        assert want <= have, f"{fam}: no row misaligns {sorted(want - have)}"
    nmc = [c for c in T.CASES if c["op"] == "nm"]
    assert any(c["ustride"] % 8 and c["dim"] % 8 == 0 for c in nmc) and any(c["dustride"] % 8 and c["dim"] % 8 == 0 for c in nmc)
    assert any(c["gn"] and c["dim"] % 8 == 0 and c["hd"] % 8 for c in nmc if c["dt"] == "16")
    assert any(c["gn"] and c["dim"] % 4 == 0 and c["hd"] % 4 for c in nmc if c["dt"] == "32")
    assert {1, 3, T.MANY_ROWS} <= {c["rows"] for c in T.CASES} and all(c["dim"] <= 64 for c in T.CASES if c["rows"] == T.MANY_ROWS)
    assert all(c["rows"] <= 33 for c in T.CASES if c["rows"] != T.MANY_ROWS)


# ------------------------------------------------------------------------------------------------------ the regressions
REGRESSIONS = [
    # name of the table row, direction, class it must reach; the parent commit refused each with
    # "dim 800 exceeds the 512 supported with this alignment" (dim 816 for 8 x 102)
    ("nm_fwd_gn_8x100", "fwd", "wide/gn-scalar/plain"), ("nm_fwd_gn_8x100", "bwd", "wide/gn-scalar/plain"),
    ("nm_fwd_gn_8x102_fp32", "fwd", "wide/gn-scalar/plain"), ("nm_fwd_gn_8x102_fp32", "bwd", "wide/gn-scalar/plain"),
    ("ln_fwd_dim800_bias_misaligned", "fwd", "wide/scalar"), ("ln_fwd_dim800_bias_misaligned_fp32", "fwd", "wide/scalar"),
    ("ln_bwd_dim800_weight_misaligned", "bwd", "wide/scalar"), ("ln_bwd_dim800_dresidual_misaligned", "bwd", "wide/scalar"),
    ("nm_fwd_ln_dim800_u_stride_804", "fwd", "wide/ln-scalar/silu"), ("nm_fwd_ln_dim800_u_stride_804", "bwd", "wide/ln-scalar/silu"),
    ("nm_bwd_ln_dim800_du_stride_804", "bwd", "wide/ln-scalar/silu"),
    ("nm_fwd_ln_dim800_u_stride_802_fp32", "fwd", "wide/ln-scalar/silu"), ("nm_bwd_ln_dim800_du_stride_801_fp32", "bwd", "wide/ln-scalar/plain"),
]


@pytest.mark.parametrize("name,direction,want", REGRESSIONS, ids=[f"{n}-{d}" for n, d, _ in REGRESSIONS])
def test_rows_the_parent_refused_reach_the_wide_scalar_kernels(ask, name, direction, want):
    c = next(c for c in T.CASES if c["name"] == name)
    d, op, q = next(x for x in _case_queries(c) if x[0] == direction)
    out = ask([q])[0]
    vec, wide, one, fast, limit, refused = out
    assert (vec, bool(wide), limit, bool(refused)) == (1, True, 2048, False) and _label(c, op, out) == want
    # the parent commit: none of the pointers its norm_wide() saw is misaligned and dim % V == 0, so it chose the narrow
    # instance -- whose scalar capacity is 512
    V = 8 if c["dt"] == "16" else 4
    assert c["dim"] % V == 0 and 512 < c["dim"] <= 1024
    assert all(r not in seen for seen in PARENT_SAW[op] for r in c["mis"])
    assert c["dim"] > _capacity(1, False)
