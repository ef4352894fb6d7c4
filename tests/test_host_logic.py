"""Host-side logic that needs no GPU."""

import os
import re

import pytest
import torch


def test_length_order_sorts_by_tile_count_and_keeps_batch_order_inside_a_tile_count():
    """sort_by_length's launch order (ops/_launch.py::length_order; reference: triton_hstu_attention.py:1968-1973 sorts by
    length): heavy users first at the granularity of the kernels' work -- 32-row tiles -- ties in batch order."""
    from generative_recommenders_amd.ops._launch import length_order

    lengths = torch.tensor([190, 200, 181, 193, 32, 33, 0, 199, 64, 1])
    off = torch.zeros(lengths.numel() + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(lengths, 0)
    order = length_order(off).tolist()
    tiles = ((lengths + 31) // 32).tolist()
    assert sorted(order) == list(range(lengths.numel()))
    assert [tiles[i] for i in order] == sorted(tiles, reverse=True)
    for a, b in zip(order, order[1:]):
        assert tiles[a] > tiles[b] or a < b            # same tile count: batch order
    assert length_order(off) is length_order(off)      # cached per offsets tensor object


def test_addmm_residual_is_refused_for_what_the_one_launch_path_cannot_take():
    """ops/_launch.py::addmm_residual_supported (hstu_addmm_residual, ABI v13): CPU tensors, fp32, a 1-D bias, mismatched shapes and rows that
    are not 16-byte multiples all stay with torch.addmm -- decided on the host, before anything is launched."""
    from generative_recommenders_amd.ops import _launch

    x = torch.zeros(8, 16, dtype=torch.bfloat16)
    y = torch.zeros(8, 32, dtype=torch.bfloat16)
    w = torch.zeros(32, 16, dtype=torch.bfloat16)
    assert not _launch.addmm_residual_supported(x, y, w)                          # CPU
    assert not _launch.addmm_residual_supported(x.float(), y.float(), w.float())  # fp32
    assert not _launch.addmm_residual_supported(x[0], y, w)                       # 1-D input (a bias)
    assert not _launch.addmm_residual_supported(x[:, :8], y, w)                   # shape mismatch


# ---------------------------------------------------------------------------------------------------------------------
# sampled-softmax loss: what hstu_sampled_softmax_fwd / _bwd refuse, decided on the host.  The addresses are aligned but
# fake: a refused call (and one of no rows) dereferences nothing and launches nothing.
_FAKE = 0x7F0000001000          # 4096-aligned, never dereferenced
HSTU_OK, HSTU_EINVAL, HSTU_EUNSUPPORTED = 0, -1, -2


def _loss_call(lib, bwd, dtype, dim, q=_FAKE, q_stride=None, num_neg=4, temperature=0.05, n_rows=5, dq_stride=None):
    s = dim if q_stride is None else q_stride
    common = (q, s, _FAKE, dim, _FAKE, _FAKE, _FAKE, _FAKE, dim, 10, n_rows, num_neg, dim, temperature, 1, 1, 1e-6)
    if bwd:
        return lib.hstu_sampled_softmax_bwd(*common, _FAKE, _FAKE, _FAKE, dim if dq_stride is None else dq_stride, _FAKE, dim, _FAKE, dtype, None)
    return lib.hstu_sampled_softmax_fwd(*common, _FAKE, _FAKE, dtype, None)


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_sampled_softmax_refusals(bwd):
    from generative_recommenders_amd import _lib as L

    lib = L.lib()
    BF16, F16, F32 = L.HSTU_DTYPE_BF16, L.HSTU_DTYPE_F16, L.HSTU_DTYPE_F32
    msg = lambda: lib.hstu_last_error().decode()
    # more than 64 16-byte units per embedding: no instantiation
    for dtype, dim in ((F32, 260), (BF16, 520), (F16, 520)):
        assert _loss_call(lib, bwd, dtype, dim) == HSTU_EUNSUPPORTED and "above 64 x 16 bytes" in msg()
    # the last dims that fit would launch: not called here (that needs a device) -- the GPU lane table runs them
    assert _loss_call(lib, bwd, F32, 6) == HSTU_EINVAL and "multiple of 4" in msg()
    assert _loss_call(lib, bwd, BF16, 12) == HSTU_EINVAL and "multiple of 8" in msg()
    assert _loss_call(lib, bwd, F32, 8, q_stride=10) == HSTU_EINVAL and "row strides" in msg()
    assert _loss_call(lib, bwd, F16, 8, q_stride=12) == HSTU_EINVAL and "row strides" in msg()
    assert _loss_call(lib, bwd, F32, 8, q=_FAKE + 4) == HSTU_EINVAL and "base pointers" in msg()
    assert _loss_call(lib, bwd, BF16, 8, q=_FAKE + 8) == HSTU_EINVAL and "base pointers" in msg()
    assert _loss_call(lib, bwd, F32, 8, num_neg=0) == HSTU_EINVAL and "num_negatives" in msg()
    assert _loss_call(lib, bwd, F32, 8, temperature=0.0) == HSTU_EINVAL and "temperature" in msg()
    if bwd:
        assert _loss_call(lib, bwd, F32, 8, dq_stride=10) == HSTU_EINVAL and "gradient rows" in msg()
    # no rows: nothing to do, whatever else is passed
    assert _loss_call(lib, bwd, F32, 8, n_rows=0) == HSTU_OK
    assert _loss_call(lib, bwd, F32, 260, n_rows=0) == HSTU_OK


def _source(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "generative_recommenders_amd", "csrc", name)) as f:
        return f.read()


def test_jagged_class_table_reaches_every_launch_line():
    """tests/jagged_class_cases.py: every row lands on its label by the restated rule (256-byte aligned allocations, as
    the GPU test asserts), every kernel has every row the matrix asks for, and the widths of the table are the launch
    lines of the three switch (v) blocks of csrc/jagged_ops.hip -- an added width fails here until the table has rows for it."""
    import jagged_class_cases as T

    base = 0x7F0000000000
    for k in T.CASES:
        assert set(k["mis"]) <= set(T.ROLES[k["kind"]]), T.case_id(k)
        ptrs = [base + T.offset(k, role) for role in T.ROLES[k["kind"]]]
        assert T.width_rule(k["row_bytes"], *ptrs) == k["v"], T.case_id(k)
        if k["why"] == "tiny":
            assert k["row_bytes"] == k["v"] and not k["mis"]
        elif k["why"] == "long":
            assert k["row_bytes"] > T.K_COPY_THREADS * k["v"] and not k["mis"]
        elif k["why"] == "size":
            assert k["row_bytes"] > k["v"] and not k["mis"]
        else:
            assert k["row_bytes"] % 16 == 0 and list(k["mis"]) == [k["why"][4:]]
    for kind in T.ROLES:
        have = {(k["why"], k["v"]) for k in T.CASES if k["kind"] == kind}
        assert have == T.required(kind), f"{kind}: missing {T.required(kind) - have}, not asked for {have - T.required(kind)}"
        rows = [k for k in T.CASES if k["kind"] == kind]
        assert {k["idx"] for k in rows} == {32, 64}
        if kind in ("concat", "split"):
            assert {k["n_prefix"] for k in rows} == {0, 1, 3}
            assert {k["shape"] for k in rows} == ({"jj", "dl", "dr", "dd"} if kind == "concat" else {"jj", "dl", "dr"})
            # n_prefix above a right length, with and without a dense side
            assert any(k["n_prefix"] == 3 and k["shape"] == "jj" for k in rows) and any(k["n_prefix"] == 3 and k["shape"] == "dl" for k in rows)
        if kind == "write_tail":
            assert {k["tail"] for k in rows} == {1, 16, 17}
    src = _source("jagged_ops.hip")
    assert f"kRowsPerBlock = {T.K_ROWS_PER_BLOCK};" in src and f"kCopyThreads = {T.K_COPY_THREADS};" in src
    # every launcher hands pick_vec (jagged_dispatch.h, tested below) all the tensors its kernel touches
    assert sorted(re.findall(r"pick_vec\(row_bytes, ([^)]*)\)", src)) == ["dense, values, nullptr", "left, right, comb", "values, dense, nullptr"]
    switches = src.split("switch (")[1:]
    assert len(switches) == 3
    for body in switches:
        body = body[:body.index("#undef LAUNCH")]
        lines = re.findall(r"^\s*(?:case (\d+)|default): LAUNCH\((\d+)\); break;$", body, flags=re.M)
        assert len(lines) == len(T.WIDTHS) and {int(v) for _, v in lines} == set(T.WIDTHS), lines
        assert all(not c or c == v for c, v in lines)
    # 3 switches: concat + split share one (the SPLIT template), so do the padded pair; 5 kernels x directions in the table
    assert src.count("LAUNCH(") - src.count("#define LAUNCH(") == 3 * len(T.WIDTHS)


_PICK_VEC_PROGRAM = r"""
#include <cstdio>
#include "jagged_dispatch.h"
int main() {
  int row_bytes;
  unsigned long long a, b, c;
  while (scanf("%d %llu %llu %llu", &row_bytes, &a, &b, &c) == 4)
    printf("%d\n", hstu::jagged_dispatch::pick_vec(row_bytes, (const void*)(uintptr_t)a, (const void*)(uintptr_t)b, (const void*)(uintptr_t)c));
  return 0;
}
"""


def test_jagged_pick_vec_follows_the_rule(tmp_path):
    """csrc/jagged_dispatch.h, compiled alone: the width it picks is the restated rule's for every row of the class table
    (pointers in the order each launcher hands them over) and for a sweep of row sizes x one, two or three misaligned
    pointers.  The GPU cannot show a width picked too wide -- it serves misaligned vector accesses -- so this is where a
    pick_vec that forgets a pointer fails."""
    import subprocess

    import jagged_class_cases as T

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "pick_vec.cpp", tmp_path / "pick_vec"
    src.write_text(_PICK_VEC_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "generative_recommenders_amd", "csrc"),
                           str(src), "-o", str(exe)])
    queries, want = [], []
    for k in T.CASES:
        ptrs = [((i + 1) << 20) + T.offset(k, role) for i, role in enumerate(T.ROLES[k["kind"]])] + [0]     # two-role kernels pass NULL last
        queries.append((k["row_bytes"], *ptrs[:3]))
        want.append(k["v"])
    offs = (0, 1, 2, 4, 8, 16, 24)
    for rb in list(range(1, 65)) + [96, 770, 1001, 1540, 3080, 6144]:
        for oa in offs:
            for ob in offs:
                for oc in offs:
                    q = (rb, (1 << 20) + oa, (2 << 20) + ob, (3 << 20) + oc)
                    queries.append(q)
                    want.append(T.width_rule(*q))
    out = subprocess.run([str(exe)], input="".join("%d %d %d %d\n" % q for q in queries), capture_output=True, text=True, check=True).stdout
    got = [int(x) for x in out.split()]
    assert len(got) == len(want)
    bad = [(q, g, w) for q, g, w in zip(queries, got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(want)} picks differ from the rule, the first (row_bytes, pointers), got, want: {bad[:3]}"
    assert set(got) == set(T.WIDTHS)


def test_loss_lane_table_reaches_every_instantiation():
    """tests/test_sampled_softmax_gpu.py::LANE_CASES: every row's LPE label is what the restated rule gives, and per I/O
    dtype the labels are exactly the LPE_CASE lines of csrc/loss_ops.hip (7 x 3 dtypes x forward / backward: every row runs
    both directions) -- an added instantiation fails here until the table has a row for it."""
    import test_sampled_softmax_gpu as S

    src = _source("loss_ops.hip")
    line = next(l for l in src.splitlines() if l.lstrip().startswith("LPE_CASE("))
    lpes = [int(x) for x in re.findall(r"LPE_CASE\((\d+)\)", line)]
    assert src.count("LPE_CASE(") == len(lpes) + 1 and len(lpes) == 7        # + the #define
    assert set(S.LANE_SHAPES) == set(lpes)
    elt = {"32": 4, "16": 2}
    for grp, D, lpe, pl2, tl2, T, strided in S.LANE_CASES:
        assert S.lane_rule(D, elt[grp]) == lpe, (grp, D)
        assert D % (16 // elt[grp]) == 0
    for grp, dtypes in S.LANE_DTYPES.items():
        rows = [c for c in S.LANE_CASES if c[0] == grp]
        assert {c[2] for c in rows} == set(lpes), grp
        assert {(c[3], c[4]) for c in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {c[5] for c in rows} == {0.05, 1.0}
        # masked lanes (D not a power of two) at LPE 4 and 64; strided rows at a masked-lane D and at LPE 64
        masked = {c[2] for c in rows if c[1] & (c[1] - 1)}
        assert {4, 64} <= masked
        strided = [c for c in rows if c[6]]
        assert any(c[1] & (c[1] - 1) for c in strided) and any(c[2] == 64 for c in strided)
    assert sorted(c[1] for c in S.LANE_CASES if c[0] == "32" and not c[6]) == [4, 8, 12, 16, 32, 36, 64, 128, 132, 256]
    assert sorted(c[1] for c in S.LANE_CASES if c[0] == "16" and not c[6]) == [8, 16, 24, 32, 64, 128, 256, 264, 512]
    # the three dtypes of loss_launch<T>
    assert sorted(len(re.findall(rf"loss_launch<{t}>\(", src)) for t in ("bf16_t", "f16_t", "float")) == [2, 2, 2]
    assert sum(len(v) for v in S.LANE_DTYPES.values()) == 3
    for lpe, (Rs, n, V) in S.LANE_SHAPES.items():
        G = 64 // lpe
        assert len(Rs) == 2 and 1 <= Rs[0] and (Rs[0] < G or G == 1) and Rs[1] == 4 * G + 1
    assert min(Rs[0] for Rs, _, _ in S.LANE_SHAPES.values()) == 1


def test_research_attention_orders_large_batches_only():
    from generative_recommenders_amd.research.modeling.sequential import hstu as R

    assert R._ORDER_MIN_USERS == 512
