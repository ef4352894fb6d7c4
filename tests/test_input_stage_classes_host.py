"""The case table of the input-stage kernels (tests/input_stage_class_cases.py) without a GPU: every row lands on its label
under the restated host geometry at 256, 64 and 304 CUs, every label is used, the restated constants are the ones in the .hip
sources, and the restated slab counts agree with hstu_input_preprocess_bwd_workspace_bytes."""

import os
import re

import pytest

import input_stage_class_cases as K
from conftest import ROOT

CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")
PRE_SRC = open(os.path.join(CSRC, "preprocess_ops.hip")).read()
RES_SRC = open(os.path.join(CSRC, "research_preprocess.hip")).read()


def _constexpr(src, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert m, f"{name} is not a constexpr int of the source"
    return int(m.group(1))


def test_restated_constants_are_the_sources():
    for name, value in (("kPreThreads", K.K_PRE_THREADS), ("kPreBlocksPerCu", K.K_PRE_BLOCKS_PER_CU),
                        ("kActionBwdGroupsMax", K.K_ACTION_BWD_GROUPS_MAX)):
        assert _constexpr(PRE_SRC, name) == value, name
    for name, value in (("kThreads", K.K_THREADS), ("kMaxUnitBlocks", K.K_MAX_UNIT_BLOCKS), ("kFwdBlocks", K.K_FWD_BLOCKS),
                        ("kBwdBlocks", K.K_BWD_BLOCKS), ("kBwdGroupsMax", K.K_BWD_GROUPS_MAX),
                        ("kBwdUsersPerGroupMin", K.K_BWD_USERS_PER_GROUP_MIN), ("kRatingGroupsMax", K.K_RATING_GROUPS_MAX)):
        assert _constexpr(RES_SRC, name) == value, name
    # the literals inside the host rules
    body = PRE_SRC[PRE_SRC.index("static int action_bwd_groups("):PRE_SRC.index("static bool aligned16(")]
    m = re.search(r"\(rows \+ (\d+) \* host_rows_par\(units\) - 1\) / \((\d+) \* host_rows_par\(units\)\)", body)
    assert m and int(m.group(1)) == int(m.group(2)) == K.ACTION_BWD_ROWS_PER_SLOT
    m = re.search(r"cap = \(int64_t\)cu_count\(\) \* (\d+);", body)
    assert m and int(m.group(1)) == K.ACTION_BWD_WGS_PER_CU
    assert re.search(r"cap = \(int64_t\)cu_count\(\) \* kPreBlocksPerCu;", PRE_SRC)
    assert re.search(r"dim3 grid\(groups, \(units \+ kPreThreads - 1\) / kPreThreads\);", PRE_SRC)
    body = RES_SRC[RES_SRC.index("int rating_groups("):RES_SRC.index("size_t pos_partial_bytes(")]
    m = re.search(r"\(\(int64_t\)d\.B \* d\.N \+ (\d+)\) / (\d+);", body)
    assert m and int(m.group(2)) == int(m.group(1)) + 1 == K.RATING_ROWS_PER_GROUP
    m = re.search(r"\(\(int64_t\)d\.Nout \* d\.Do \+ (\d+) \* kThreads - 1\) / \((\d+) \* kThreads\)", RES_SRC)
    assert m and m.group(1) == m.group(2) == "8"
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
