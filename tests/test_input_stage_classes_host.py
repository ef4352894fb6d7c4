"""The case table of the input-stage kernels (tests/input_stage_class_cases.py) without a GPU: every row lands on its label
under the restated host geometry at 256, 64 and 304 CUs, every label is used, the restatement answers what the compiled host
header (csrc/input_stage_dispatch.h) answers, and the restated slab counts agree with hstu_input_preprocess_bwd_workspace_bytes."""

import os
import re

import numpy as np
import pytest

import input_stage_class_cases as K
from conftest import ROOT

CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")

# Every query is one line "name integers..."; every answer one line of integers.  A pointer is given as its byte offset from
# a base of its own (-1: NULL).
_HEADER_PROGRAM = r"""
#include "input_stage_dispatch.h"

#include <cstdio>
#include <cstring>
using namespace hstu;
using namespace hstu::input_stage;
static long long v[16];
static const void* ptr(int slot, long long off) { return off < 0 ? nullptr : (const void*)(uintptr_t)(((slot + 1ll) << 20) + off); }
static Dims dims(int i) {
  Dims d;
  d.B = (int)v[i]; d.N = (int)v[i + 1]; d.Nout = (int)v[i + 2]; d.Di = (int)v[i + 3]; d.Dr = (int)v[i + 4]; d.Do = (int)v[i + 5];
  d.R = (int)v[i + 6]; d.P = (int)v[i + 7]; d.layout = (int)v[i + 8];
  return d;
}
int main() {
  static_assert(threads_per_row(0, 256) == 1 && rows_in_flight(24, 256) == 8, "constexpr: host and device share the rule");
  char name[32], line[512];
  while (fgets(line, sizeof line, stdin)) {
    int used = 0, n = 0;
    if (sscanf(line, "%31s%n", name, &used) != 1) continue;
    for (int k; n < 16 && sscanf(line + used, "%lld%n", &v[n], &k) == 1; used += k) ++n;
    auto is = [&](const char* q) { return !strcmp(name, q); };
    if (is("tpr")) printf("%d %d\n", threads_per_row((int)v[0], (int)v[1]), rows_in_flight((int)v[0], (int)v[1]));
    else if (is("resident")) printf("%d\n", resident_blocks(v[0], (int)v[1], (int)v[2]));
    else if (is("abwd_groups")) printf("%d\n", action_bwd_groups(v[0], (int)v[1], (int)v[2]));
    else if (is("abwd_y")) printf("%d\n", action_bwd_grid_y((int)v[0]));
    else if (is("abwd_finish")) printf("%d\n", action_bwd_finish_blocks((int)v[0]));
    else if (is("abwd_bytes")) printf("%zu\n", action_bwd_workspace_bytes((int32_t)v[0]));
    else if (is("action_fwd")) printf("%d\n", action_fwd_piece((int)v[0], (int)v[1], ptr(0, v[2]), ptr(1, v[3]), ptr(2, v[4])));
    else if (is("action_bwd")) printf("%d\n", action_bwd_piece((int)v[0], (int)v[1], ptr(0, v[2]), ptr(1, v[3])));
    else if (is("combine_fwd")) printf("%d\n", combine_fwd_piece((int)v[0], (int)v[1], ptr(0, v[2]), ptr(1, v[3]), ptr(2, v[4]), ptr(3, v[5])));
    else if (is("combine_bwd")) printf("%d\n", combine_bwd_piece((int)v[0], (int)v[1], ptr(0, v[2]), ptr(1, v[3]), ptr(2, v[4]), ptr(3, v[5])));
    else if (is("out_rows")) printf("%lld\n", (long long)combine_out_rows((int)v[0], v[1], v[2], (int)v[3], (int)v[4]));
    else if (is("bwd_rows")) printf("%lld\n", (long long)combine_bwd_rows(v[0], (int)v[1], (int)v[2], v[3] != 0));
    else if (is("unit_blocks")) printf("%d\n", unit_blocks(dims(0), (int)v[9]));
    else if (is("fwd_groups")) printf("%d\n", fwd_user_groups(dims(0), (int)v[9]));
    else if (is("bwd_groups")) printf("%d\n", bwd_groups(dims(0)));
    else if (is("slab_count")) { int upg = -1; const int slabs = slab_count((int)v[0], (int)v[1], &upg); printf("%d %d\n", slabs, upg); }
    else if (is("rating_groups")) printf("%d\n", rating_groups(dims(0)));
    else if (is("rating_z")) printf("%d\n", rating_grid_z(dims(0), (int)v[9]));
    else if (is("pos_finish")) printf("%d\n", pos_finish_blocks(v[0]));
    else if (is("rating_finish")) printf("%d\n", rating_finish_blocks((int)v[0]));
    else if (is("partials")) printf("%zu %zu\n", pos_partial_bytes(dims(0)), rating_partial_bytes(dims(0)));
    else if (is("pick_vec")) printf("%d\n", pick_vec(dims(0), (size_t)v[9], (size_t)v[10], {ptr(0, v[11])}, {ptr(1, v[12]), ptr(2, v[13]), ptr(3, v[14])}));
    else { fprintf(stderr, "unknown query %s\n", name); return 2; }
  }
  return 0;
}
"""


def _dims(layout, B, N, di, dr, R, extra_pos=0):
    n_out = K.n_out_of(layout, N)
    return (B, N, n_out, di, dr, K.d_out_of(layout, di, dr), R, n_out + extra_pos, layout)


def _pow2_neighbours(lo, hi):
    """lo .. hi by powers of two, each with its two neighbours"""
    out, p = set(), lo
    while p <= hi:
        out |= {p - 1, p, p + 1}
        p <<= 1
    return sorted(x for x in out if x >= 0)


def test_header_agrees_with_the_restatement(tmp_path):
    """csrc/input_stage_dispatch.h (with csrc/row_slots.h), compiled alone by g++ -- so it is host-only -- answers exactly what
    the restatement of input_stage_class_cases.py answers: for every P row at 256, 64 and 304 CUs (rows in flight, grid, action
    backward groups and grid.y, the piece width under the row's misalignments, the combine row counts), for every R row (unit
    blocks at every admitted V, forward user groups, d_pos groups, both outputs of slab_count, rating groups and grid.z,
    pick_vec of both directions under the row's pointer offsets, both partial sizes), and for a sweep in which every constant
    and every clamp sits on a boundary.  Which query pins what:

      tpr            the slot rule: units 0 .. 3, every power of two +-1 up to 4096, at 64 and 256 threads (the cap)
      resident       kPreBlocksPerCu and both clamps: rows = cap * rows_par -1 / +0 / +1 at each CU count and rows_par, rows 0 / 1
      abwd_groups    kActionBwdRowsPerSlot: rows = 8 rows_par g +0 / +1 for small g; kActionBwdWgsPerCu: g around 2 CUs at 64 and
                     256 CUs; kActionBwdGroupsMax: g around 512 at 304 CUs (2 CUs = 608 does not bind there); rows 0 -> 1;
                     kPreThreads through rows_par at 1 .. 257 units
      abwd_y         kPreThreads: units 255 .. 257, 511 .. 513;  abwd_finish: the 2 tables x 256 threads;  abwd_bytes:
                     kActionBwdGroupsMax x 2 x 4 bytes, width <= 0
      action_fwd ..  the 16-byte rule of each launcher: row elements that N does and does not divide, offsets {0, 2, 4, 8, 16}
      combine_bwd    and NULL on every pointer the launcher names, in every combination
      out_rows       the three modes;  bwd_rows: with and without the contextual rows
      unit_blocks    kThreads: 255 .. 257 pieces; kMaxUnitBlocks: 1024 x 256 pieces -1 / +0 / +1; no pieces -> 1
      fwd_groups     kFwdBlocks: gx 1, 2, 3, 2047, 2048, 2049 with more users than groups; the user limit with few
      bwd_groups     the 8 x kThreads elements per unit block and kBwdBlocks: Nout Do = 63 x 2048 +0 / +1 (33 -> 32 groups), unit
                     blocks 64 (2048 = 32 x 64: + 1 would show) and 89 (2047 = 23 x 89: - 1 would show); kMaxUnitBlocks: 2048 and
                     more unit blocks (2 groups, not 1); kBwdUsersPerGroupMin: B = 16, 17 and every B below; kBwdGroupsMax:
                     B = 504, 512, 513, 520 with few elements; B = 0 -> 1
      slab_count     every B <= 40 x every group count <= 12
      rating_groups  kRatingRowsPerGroup: B N = 64, 65, 127 .. 129; kRatingGroupsMax: 64 x 255 and 64 x 256 rows -1 / +0 / +1; 0 -> 1
      rating_z       kThreads through the slot rule: Dr / V = 1 .. 3, 255 .. 257, 511 .. 513
      pos_finish     kThreads: 255 .. 257 elements; kFwdBlocks: 2048 x 256 -1 / +0 / +1;  rating_finish: 255 .. 257, 512, 513
      partials       align256 (sizes just below, at and above a multiple of 256 bytes come with the R rows and the sweep's B)
      pick_vec       every (embedding, output) dtype pair x row widths that 8, 4, 2 and nothing divide, in the three layouts, x
                     offsets {0, 2, 4, 8, 16} on each of the four pointer roles in every combination, and NULL roles; Do, Di
                     and Dr each the only width that 8 (or 4) does not divide
    """
    import subprocess

    src, exe = tmp_path / "input_stage.cpp", tmp_path / "input_stage"
    src.write_text(_HEADER_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    queries = []                                         # (name, arguments, what the restatement answers)

    def ask(name, args, want):
        queries.append((name, tuple(int(a) for a in args), tuple(int(w) for w in (want if isinstance(want, tuple) else (want,)))))

    # ---- the P rows
    offs = (0, 2, 4, 8, 16)
    roles = {"action_fwd": ("table", "target_table", "out"), "action_bwd": ("d_out", "partial"),
             "combine_fwd": ("content", "action", "contextual", "out"), "combine_bwd": ("d_out", "d_content", "d_action", "d_contextual")}
    for c in K.P_CASES:
        assert set(c["mis"]) <= set(roles[c["kind"]]), K.p_id(c)
        eb = K.ELEM_BYTES[c["dtype"]]
        ask(c["kind"], (K.p_row_elems(c)[1], eb, *(c["mis"].get(r, 0) for r in roles[c["kind"]])), K.p_vec(c))
        for cus in K.CU_COUNTS:
            f = K.p_class_facts(c, cus)
            ask("tpr", (f["units"], K.K_PRE_THREADS), (f["tpr"], f["rows_par"]))
            if c["kind"] == "action_bwd":
                ask("abwd_groups", (f["rows"], f["units"], cus), f["groups"])
                ask("abwd_y", (f["units"],), f["grid_y"])
            else:
                ask("resident", (f["rows"], f["rows_par"], cus), f["grid"])
            if c["kind"].startswith("combine"):
                lengths, targets = K.batch_of(c, cus)
                total, t = int(lengths.sum()), int(targets.sum())
                ask("out_rows", (c["mode"], total - t, t, len(lengths), c["C"]), K.combine_out_rows(lengths, targets, c["C"], c["mode"]))
                if c["kind"] == "combine_bwd":
                    ask("bwd_rows", (total, len(lengths), c["C"], c["d_ctx"] and c["C"] > 0), f["rows"])
    # ---- the R rows
    for c in K.R_CASES:
        d = _dims(c["layout"], c["B"], c["N"], c["di"], c["dr"], c["R"], c["extra_pos"])
        f = K.r_class_facts(c)
        for v in K.admitted_vs(c["emb"], c["out"]):
            gx = K.unit_blocks(f["n_out"], f["do"], v)
            ask("unit_blocks", (*d, v), gx)
            ask("fwd_groups", (*d, gx), K.fwd_user_groups(c["B"], gx))
            ask("slab_count", (c["B"], K.fwd_user_groups(c["B"], gx)), K.slab_count(c["B"], K.fwd_user_groups(c["B"], gx)))
        ask("bwd_groups", d, f["groups"])
        ask("slab_count", (c["B"], f["groups"]), (f["slabs"], f["users_per_slab"]))
        ask("partials", d, K.research_workspace_bytes(c["layout"], c["B"], c["N"], c["di"], c["dr"], c["R"]))
        if c["layout"] != K.PLAIN:
            ask("rating_groups", d, f["rating_groups"])
            ask("rating_z", (*d, f["v_bwd"]), f["rating_grid_z"])
        es, osz, m = K.ELEM_BYTES[c["emb"]], K.ELEM_BYTES[c["out"]], c["mis"]
        ask("pick_vec", (*d, es, osz, *(m.get(k, 0) for k in K.FWD_EMB_ROLES + K.FWD_OUT_ROLES)), f["v_fwd"])
        ask("pick_vec", (*d, es, osz, *(m.get(k, 0) for k in K.BWD_EMB_ROLES + K.BWD_OUT_ROLES), 0, -1), f["v_bwd"])   # workspace, NULL
    # ---- the sweep: row_slots.h
    for threads in (64, 256):
        for units in _pow2_neighbours(1, 4096):
            ask("tpr", (units, threads), (K.threads_per_row(units, threads), K.rows_in_flight(units, threads)))
    # ---- the sweep: preprocess_ops.hip
    rows_pars = (1, 2, 8, 64, 256)
    for cus in K.CU_COUNTS:
        for rp in rows_pars:
            cap = cus * K.K_PRE_BLOCKS_PER_CU
            for rows in (0, 1, rp - 1, rp, rp + 1, cap * rp - 1, cap * rp, cap * rp + 1, (cap - 1) * rp, (cap - 1) * rp + 1, 3 * cap * rp):
                ask("resident", (rows, rp, cus), K.resident_blocks(rows, rp, cus))
        for units in (1, 3, 8, 24, 129, 256, 257):
            slot = K.ACTION_BWD_ROWS_PER_SLOT * K.host_rows_par(units)
            marks = {1, 2, 3, 5, cus * K.ACTION_BWD_WGS_PER_CU - 1, cus * K.ACTION_BWD_WGS_PER_CU, K.K_ACTION_BWD_GROUPS_MAX - 1,
                     K.K_ACTION_BWD_GROUPS_MAX, K.K_ACTION_BWD_GROUPS_MAX + 100}
            for rows in [0, 1] + [slot * g + e for g in marks for e in (-1, 0, 1)]:
                ask("abwd_groups", (rows, units, cus), K.action_bwd_groups(rows, units, cus))
    for units in (0, 1, 255, 256, 257, 511, 512, 513):
        ask("abwd_y", (units,), K.action_bwd_grid_y(units))
    for width in (-1, 0, 1, 127, 128, 129, 255, 256, 257, 2560):
        ask("abwd_bytes", (width,), K.action_bwd_workspace_bytes(width))
        if width > 0:
            ask("abwd_finish", (width,), K.action_bwd_finish_blocks(width))
    import itertools

    for kind, names in roles.items():
        for dtype in (K.BF16, K.F32):
            for elems in (4, 8, 9, 12, 24, 27):
                for at in itertools.product(offs + (-1,), repeat=len(names)):
                    ask(kind, (elems, K.ELEM_BYTES[dtype], *at), K.pre_pick_vec(elems, dtype, any(o > 0 and o % 16 for o in at)))
    one = lambda total, t, batch: (np.asarray([total] + [0] * (batch - 1)), np.asarray([t] + [0] * (batch - 1)))
    for mode in (K.SUM, K.INTERLEAVE_ALL, K.INTERLEAVE_UIH):
        for total, t, batch, C in ((0, 0, 1, 0), (10, 3, 1, 0), (10, 3, 4, 3), (1000, 1000, 7, 2), (5, 0, 2, 1)):
            ask("out_rows", (mode, total - t, t, batch, C), K.combine_out_rows(*one(total, t, batch), C, mode))
    for total, batch, C, ctx in ((10, 4, 3, 1), (10, 4, 3, 0), (0, 5, 2, 1), (7, 3, 0, 1)):
        ask("bwd_rows", (total, batch, C, ctx), total + (batch * C if ctx else 0))
    # ---- the sweep: research_preprocess.hip
    plain = lambda B, N, D: _dims(K.PLAIN, B, N, D, 0, 0)
    for n_out, do in ((0, 64), (1, 1), (1, 255), (1, 256), (1, 257), (51, 5), (16, 16), (512, 512), (481, 545), (513, 511), (1029, 257)):
        for v in (1, 2, 4, 8):
            ask("unit_blocks", (*plain(3, n_out, do), v), K.unit_blocks(n_out, do, v))
    for gx in (1, 2, 3, 1023, 1024, K.K_FWD_BLOCKS - 1, K.K_FWD_BLOCKS, K.K_FWD_BLOCKS + 1):
        for B in (1, 2, 5, 2047, 2048, 2049, 5000):
            ask("fwd_groups", (*plain(B, 9, 64), gx), K.fwd_user_groups(B, gx))
    many = 8 * 64 * 4                                    # users: neither the user limit nor the clamp binds below 64 groups
    for n_out, do in ((63, 2048), (129025, 1), (64, 2048), (131073, 1), (89, 2048), (88 * 2048 + 1, 1), (2048, 2048), (2049, 2048),
                      (1024, 2048), (1023, 2048), (1025, 2048), (36, 2048), (0, 64), (1, 2048), (2049, 1)):
        ask("bwd_groups", plain(many, n_out, do), K.bwd_groups(many, n_out, do))
    for B in list(range(0, 34)) + [503, 504, 505, 511, 512, 513, 519, 520, 521, 5000]:
        ask("bwd_groups", plain(B, 9, 64), K.bwd_groups(B, 9, 64))
        ask("partials", _dims(K.CONCAT, B, 9, 5, 3, 7), K.research_workspace_bytes(K.CONCAT, B, 9, 5, 3, 7))
        ask("partials", plain(B, 9, 5), K.research_workspace_bytes(K.PLAIN, B, 9, 5, 0, 0))
        ask("partials", _dims(K.PLAIN, B, 9, 5, 3, 7), K.research_workspace_bytes(K.PLAIN, B, 9, 5, 3, 7))   # PLAIN: no rating partials
    for B in range(1, 41):
        for groups in range(1, 13):
            ask("slab_count", (B, groups), K.slab_count(B, groups))
    g64 = K.RATING_ROWS_PER_GROUP
    for rows in (0, 1, g64 - 1, g64, g64 + 1, 2 * g64 - 1, 2 * g64, 2 * g64 + 1, g64 * 255 - 1, g64 * 255, g64 * 255 + 1, g64 * 256 - 1,
                 g64 * 256, g64 * 256 + 1, g64 * 1000):
        ask("rating_groups", _dims(K.CONCAT, 1, rows, 5, 3, 7), K.rating_groups(1, rows))
        ask("rating_groups", _dims(K.CONCAT, rows, 1, 5, 3, 7), K.rating_groups(rows, 1))
    for units in (1, 2, 3, 255, 256, 257, 511, 512, 513):
        for v in (1, 2, 8):
            ask("rating_z", (*_dims(K.CONCAT, 4, 9, 8, units * v, 7), v), K.rating_grid_z(units * v, v))
    T, F = K.K_THREADS, K.K_FWD_BLOCKS
    for total in (0, 1, T - 1, T, T + 1, F * T - 1, F * T, F * T + 1, (F - 1) * T, (F - 1) * T + 1, 10 * F * T):
        ask("pos_finish", (total,), K.pos_finish_blocks(total))
    for width in (1, T - 1, T, T + 1, 2 * T, 2 * T + 1):
        ask("rating_finish", (width,), K.rating_finish_blocks(width))
    shapes = ((K.PLAIN, 64, 0), (K.PLAIN, 68, 0), (K.PLAIN, 66, 0), (K.PLAIN, 67, 0), (K.CONCAT, 56, 8), (K.CONCAT, 60, 4),
              (K.CONCAT, 50, 14), (K.CONCAT, 64, 7), (K.CONCAT, 4, 60), (K.INTERLEAVE, 64, 64), (K.INTERLEAVE, 66, 66))
    for emb, out in K.R_PAIRS:
        es, osz = K.ELEM_BYTES[emb], K.ELEM_BYTES[out]
        for layout, di, dr in shapes:
            d = _dims(layout, 4, 9, di, dr, 0 if layout == K.PLAIN else 6)
            for at in itertools.product(offs, repeat=4):
                ask("pick_vec", (*d, es, osz, *at), K.research_pick_vec(layout, di, dr, emb, out, at[:1], at[1:]))
            for at in ((-1, 0, 0, 0), (8, -1, -1, 0), (0, 4, -1, -1), (-1, -1, -1, -1), (0, -1, 2, -1)):
                want = K.research_pick_vec(layout, di, dr, emb, out, [o for o in at[:1] if o >= 0], [o for o in at[1:] if o >= 0])
                ask("pick_vec", (*d, es, osz, *at), want)

        # widths no call has (Do follows from Di and Dr): each of the three divisibility checks decides alone
        for layout, di, dr, do in ((K.PLAIN, 64, 0, 60), (K.PLAIN, 60, 0, 64), (K.CONCAT, 64, 4, 64), (K.CONCAT, 64, 2, 64)):
            d = _dims(layout, 4, 9, di, dr, 0 if layout == K.PLAIN else 6)
            ask("pick_vec", (*d[:5], do, *d[6:], es, osz, 0, 0, 0, 0), K.research_pick_vec(layout, di, dr, emb, out, [0], [0], do=do))

    text = "".join("%s %s\n" % (name, " ".join(map(str, args))) for name, args, _ in queries)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
    got = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    assert len(got) == len(queries)
    bad = [(name, args, g, want) for (name, args, want), g in zip(queries, got) if g != want]
    by_name = sorted({b[0] for b in bad})
    assert not bad, f"{len(bad)} of {len(queries)} answers differ ({by_name}); the first (query, arguments, header, restatement): {bad[:3]}"
    # what the sweep is there for: every clamp was reached and every piece width picked
    answers = lambda name: {g for (n, _, _), g in zip(queries, got) if n == name}
    assert {(1,), (K.K_ACTION_BWD_GROUPS_MAX,), (2 * 64,), (2 * 256,)} <= answers("abwd_groups")
    assert {(1,), (K.K_MAX_UNIT_BLOCKS,)} <= answers("unit_blocks") and {(1,), (K.K_BWD_GROUPS_MAX,), (2,), (32,), (33,)} <= answers("bwd_groups")
    assert {(1,), (K.K_RATING_GROUPS_MAX,)} <= answers("rating_groups") and {(K.K_FWD_BLOCKS,)} <= answers("pos_finish")
    assert answers("pick_vec") == {(8,), (4,), (2,), (1,)} and answers("action_fwd") == {(8,), (4,), (1,)}
    # without a device the units' cu_count() answers HOST_CUS: the CU count the host tests of the table assume
    m = re.search(r"inline int cu_count\(\) \{.*?int n = (\d+);", open(os.path.join(CSRC, "capi_internal.h")).read(), flags=re.S)
    assert m and int(m.group(1)) == K.HOST_CUS


@pytest.mark.parametrize("cus", K.CU_COUNTS)
@pytest.mark.parametrize("case", K.P_CASES, ids=K.p_id)
def test_preprocess_rows_land_on_their_labels(case, cus):
    assert K.p_lands_on_its_label(case, cus), K.p_class_facts(case, cus)


@pytest.mark.parametrize("case", K.R_CASES, ids=K.r_id)
def test_research_rows_land_on_their_labels(case):
    """(nothing in research_preprocess.hip's geometry depends on the CU count)"""
    assert K.r_lands_on_its_label(case), K.r_class_facts(case)


def test_ids_are_unique_and_every_label_is_used():
    for cases, ident, labels in ((K.P_CASES, K.p_id, K.P_LABELS), (K.R_CASES, K.r_id, K.R_LABELS)):
        ids = [ident(c) for c in cases]
        assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
        assert {c["label"] for c in cases} == set(labels)


def test_preprocess_table_holds_what_the_classes_need():
    P = K.P_CASES
    walk = [c for c in P if c["label"] == K.WALK]
    rp = lambda c: K.host_rows_par(K.p_units(c))
    for kind in ("action_fwd", "combine_fwd", "combine_bwd"):
        got = {rp(c) for c in walk if c["kind"] == kind}
        assert {1, 64} <= got and any(1 < r < 64 for r in got), (kind, got)
    assert {(c["mode"], c["C"]) for c in walk if c["kind"] == "combine_fwd"} == {(m, C) for m in (0, 1, 2) for C in (0, 3)}
    bwd = [c for c in walk if c["kind"] == "combine_bwd"]
    assert {c["mode"] for c in bwd} == {0, 1, 2}
    assert {c["d_action"] for c in bwd} == {True, False} and {bool(c["d_ctx"] and c["C"]) for c in bwd} == {True, False}
    assert any(K.p_class_facts(c, K.HOST_CUS)["straddles"] for c in bwd)
    assert {c["idx"] for c in P} == {32, 64}
    wide = [c for c in P if c["label"] == K.WIDE]
    assert {(c["kind"], K.p_vec(c) > 1) for c in wide} >= {("combine_fwd", False), ("combine_fwd", True), ("combine_bwd", False),
                                                           ("combine_bwd", True), ("action_fwd", False), ("action_fwd", True)}
    assert any(c["T"] == 64 and c["dtype"] == K.BF16 for c in wide)
    w = K.wide_weights()
    assert len(w) == 64 and max(w) < 2**63 and sum(bin(x).count("1") == 1 for x in w) == 60 and (1 << 62) in w
    assert {K.p_vec(c) > 1 for c in P if c["label"] == K.BWD_Y} == {True, False}
    assert sorted(c["groups"] for c in P if c["label"] == K.BWD_GROUPS) == [4, 5, 6, 7]
    clamp = [c for c in P if c["label"] == K.BWD_CLAMP]
    assert len(clamp) == 1 and 4100 <= K.p_class_facts(clamp[0], 256)["rows"] <= 4200
    mis = [c for c in P if c["label"] == K.MISALIGNED]
    assert {(c["kind"], role) for c in mis for role in c["mis"]} == {("action_fwd", "table"), ("action_fwd", "target_table"),
                                                                    ("action_fwd", "out"), ("action_bwd", "d_out")}
    assert {v for c in mis for v in c["mis"].values()} == {2, 4}
    # every batch holds empty users, users without targets, users of targets only
    for c in P:
        lengths, targets = K.batch_of(c, K.HOST_CUS)
        assert (lengths == 0).any() and ((lengths > 0) & (targets == 0)).any() and ((lengths > 0) & (targets == lengths)).any()


def test_research_table_holds_what_the_classes_need():
    matrix = [c for c in K.R_CASES if c["label"] == K.MATRIX]
    for emb, out in K.R_PAIRS:
        got = {c["v"] for c in matrix if (c["emb"], c["out"]) == (emb, out)}
        assert got == set(K.admitted_vs(emb, out)), (emb, out, got)
        assert len({c["layout"] for c in matrix if (c["emb"], c["out"]) == (emb, out)}) == 3
    assert {c["layout"] for c in matrix} == {K.PLAIN, K.CONCAT, K.INTERLEAVE}
    assert {b for c in K.R_CASES if c["label"] == K.LOWERED for b in c["mis"].values()} == {4, 8}
    stride = [c for c in K.R_CASES if c["label"] == K.STRIDE]
    assert any(c["p"] == 0.2 for c in stride) and {c["layout"] for c in stride} == {K.PLAIN, K.INTERLEAVE}
    assert any(c["layout"] == K.INTERLEAVE and c["B"] >= 100 for c in K.R_CASES), "INTERLEAVE with many users"
    assert any(c["extra_pos"] for c in K.R_CASES if c["label"].startswith("R-pos"))
    assert all(c["unused_rating"] is not None for c in K.R_CASES if c["layout"] != K.PLAIN)
    z = {K.r_class_facts(c).get("rating_grid_z") for c in K.R_CASES if c["label"] == K.RATING}
    assert z == {1, 2}
    # the heaviest case is the smallest the restatement admits: over every unit-block count ub, more than (ub - 1) * 2048
    # elements per user and more than 8 * ceil(2048 / ub) users
    heavy = [c for c in K.R_CASES if c["label"] == K.POS_BLOCKS]
    assert len(heavy) == 1
    least = min((8 * K.ceil_div(K.K_BWD_BLOCKS, ub) + 1) * ((ub - 1) * 8 * K.K_THREADS + 1)
                for ub in range(2, K.K_MAX_UNIT_BLOCKS + 1) if K.ceil_div(K.K_BWD_BLOCKS, ub) < K.K_BWD_GROUPS_MAX)
    c = heavy[0]
    assert least <= c["B"] * c["N"] * c["di"] <= 1.001 * least, (least, c["B"] * c["N"] * c["di"])


@pytest.mark.parametrize("case", K.R_CASES, ids=K.r_id)
def test_restated_slab_counts_agree_with_the_workspace_helper(case):
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    c = case
    got = _lib.lib().hstu_input_preprocess_bwd_workspace_bytes(c["B"], c["N"], c["di"], c["dr"], c["R"], c["layout"])
    pos, rat = K.research_workspace_bytes(c["layout"], c["B"], c["N"], c["di"], c["dr"], c["R"])
    assert got == pos + rat
    # ... and the two counts can be told apart in that sum: one more group of either changes it
    f = K.r_class_facts(c)
    assert pos == -(-f["groups"] * f["n_out"] * f["do"] * 4 // 256) * 256
    if c["layout"] != K.PLAIN:
        assert rat == -(-f["rating_groups"] * c["R"] * c["dr"] * 4 // 256) * 256
