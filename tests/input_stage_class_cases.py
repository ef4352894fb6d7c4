"""The class matrix of the input-stage kernels (csrc/preprocess_ops.hip, csrc/research_preprocess.hip): one literal table
of calls, each labelled with the class it is MEANT to reach -- the lines of those kernels that only run once a workgroup
walks many rows (the slab loop, the user advance, the wrapped lane loop, the second grid dimension, the clamps of the slab
counts, the grid stride).  tests/test_input_stage_classes_gpu.py runs every row on the GPU through the C ABI, with outputs
and workspaces it owns; tests/test_input_stage_classes_host.py checks without a GPU that every row lands on its label under
the restatement of the host geometry below (at 256, 64 and 304 CUs), that every label is used, and that the restatement
answers what csrc/input_stage_dispatch.h and csrc/row_slots.h -- the host geometry of the two units, compiled alone --
answer, for every row and for a sweep around every constant.

Layout shared by both: every output and workspace lives alone in a sentinel-filled byte allocation (256-byte aligned),
GUARD bytes from its start plus the bytes ``mis`` lists for its role; GUARD more bytes follow it.

Row counts that depend on the CU count are given as a rule ("slots" / "groups" / "clamp", see ``rows_of``), not as literals.
"""

import numpy as np

GUARD = 256                       # bytes in front of and behind every output and workspace
HOST_CUS = 256                    # what cu_count() answers without a device
CU_COUNTS = (256, 64, 304)

BF16, F16, F32 = "bfloat16", "float16", "float32"
ELEM_BYTES = {BF16: 2, F16: 2, F32: 4}
SUM, INTERLEAVE_ALL, INTERLEAVE_UIH = 0, 1, 2          # HSTU_COMBINE_*
PLAIN, CONCAT, INTERLEAVE = 0, 1, 2                    # HSTU_PREPROCESS_*

# ------------------------------------------------------------------------------------------------ row_slots.h
def threads_per_row(units, threads):
    tpr = 1
    while tpr < units and tpr < threads:
        tpr <<= 1
    return tpr


def rows_in_flight(units, threads):
    return threads // threads_per_row(units, threads)


# ------------------------------------------------------------------------------------------------ preprocess_ops.hip
K_PRE_THREADS = 256               # kPreThreads
K_PRE_BLOCKS_PER_CU = 8           # kPreBlocksPerCu
K_ACTION_BWD_GROUPS_MAX = 512     # kActionBwdGroupsMax
ACTION_BWD_ROWS_PER_SLOT = 8      # the "8 *" of action_bwd_groups: slabs of at least 8 rows per row slot
ACTION_BWD_WGS_PER_CU = 2         # the "* 2" of action_bwd_groups


def ceil_div(a, b):
    return -(-a // b)


def host_tpr(units):
    return threads_per_row(units, K_PRE_THREADS)


def host_rows_par(units):
    return K_PRE_THREADS // host_tpr(units)


def resident_blocks(rows, rows_par, cus):
    b = min(ceil_div(rows, rows_par), cus * K_PRE_BLOCKS_PER_CU)
    return max(b, 1)


def action_bwd_groups_unclamped(rows, units):
    return ceil_div(rows, ACTION_BWD_ROWS_PER_SLOT * host_rows_par(units))


def action_bwd_cap(cus):
    return min(cus * ACTION_BWD_WGS_PER_CU, K_ACTION_BWD_GROUPS_MAX)


def action_bwd_groups(rows, units, cus):
    return max(min(action_bwd_groups_unclamped(rows, units), action_bwd_cap(cus)), 1)


def action_bwd_grid_y(units):
    return ceil_div(units, K_PRE_THREADS)


def action_bwd_finish_blocks(width):
    return ceil_div(2 * width, 256)


def action_bwd_workspace_bytes(width):
    return K_ACTION_BWD_GROUPS_MAX * 2 * width * 4 if width > 0 else 0


def pre_pick_vec(row_elems, dtype, any_misaligned):
    """the `vec` of the four launchers of preprocess_ops.hip: 16-byte pieces (N elements) when N divides the row -- Da for
    the action ops, D for combine -- and every base pointer the launcher looks at is 16-byte aligned; elements otherwise"""
    n = 16 // ELEM_BYTES[dtype]
    return n if (row_elems % n == 0 and not any_misaligned) else 1


def slab_rows(rows, grid):
    """slab_of: rows per workgroup"""
    return ceil_div(rows, grid)


# ------------------------------------------------------------------------------------------------ research_preprocess.hip
K_THREADS = 256                   # kThreads
K_MAX_UNIT_BLOCKS = 1024          # kMaxUnitBlocks
K_FWD_BLOCKS = 2048               # kFwdBlocks
K_BWD_BLOCKS = 2048               # kBwdBlocks
K_BWD_GROUPS_MAX = 64             # kBwdGroupsMax
K_BWD_USERS_PER_GROUP_MIN = 8     # kBwdUsersPerGroupMin
K_RATING_GROUPS_MAX = 256         # kRatingGroupsMax
RATING_ROWS_PER_GROUP = 64        # the 64 of rating_groups


def n_out_of(layout, n):
    return 2 * n if layout == INTERLEAVE else n


def d_out_of(layout, di, dr):
    return di + dr if layout == CONCAT else di


def unit_blocks(n_out, do, v):
    b = ceil_div(n_out * (do // v), K_THREADS)
    return min(max(b, 1), K_MAX_UNIT_BLOCKS)


def fwd_user_groups(batch, gx):
    return min(ceil_div(K_FWD_BLOCKS, gx), batch)


def bwd_groups_by_blocks(n_out, do):
    ub = min(max(ceil_div(n_out * do, 8 * K_THREADS), 1), K_MAX_UNIT_BLOCKS)
    return ceil_div(K_BWD_BLOCKS, ub)


def bwd_groups_by_users(batch):
    return ceil_div(batch, K_BWD_USERS_PER_GROUP_MIN)


def bwd_groups(batch, n_out, do):
    return max(min(bwd_groups_by_blocks(n_out, do), bwd_groups_by_users(batch), K_BWD_GROUPS_MAX), 1)


def slab_count(batch, groups):
    """(number of slabs, users per slab)"""
    upg = ceil_div(batch, groups)
    return ceil_div(batch, upg), upg


def rating_groups(batch, n):
    return max(min(ceil_div(batch * n, RATING_ROWS_PER_GROUP), K_RATING_GROUPS_MAX), 1)


def rating_tpr(dr, v):
    return threads_per_row(dr // v, K_THREADS)


def rating_grid_z(dr, v):
    return ceil_div(dr // v, rating_tpr(dr, v))


def pos_finish_blocks(total):
    return min(ceil_div(total, K_THREADS), K_FWD_BLOCKS)


def rating_finish_blocks(width):
    return ceil_div(width, K_THREADS)


def research_pick_vec(layout, di, dr, emb_dtype, out_dtype, emb_offsets, out_offsets, do=None):
    """pick_vec of research_preprocess.hip: the widest of 8 / 4 / 2 / 1 elements (at most 16 bytes of the output dtype) that
    divides Do, Di (and Dr in the rated layouts) and that every base pointer is aligned to -- the embedding-typed ones to
    V * sizeof(emb), the others to V * sizeof(out).  ``*_offsets``: byte offsets of the pointers from 256-byte alignment.
    ``do``: an output width other than the layout's (no call has one; it tells the three divisibility checks apart)"""
    do = d_out_of(layout, di, dr) if do is None else do
    es, osz = ELEM_BYTES[emb_dtype], ELEM_BYTES[out_dtype]
    v = 16 // osz
    while v > 1:
        ok = do % v == 0 and di % v == 0 and (layout == PLAIN or dr % v == 0)
        ok = ok and all(o % (v * es) == 0 for o in emb_offsets) and all(o % (v * osz) == 0 for o in out_offsets)
        if ok:
            return v
        v >>= 1
    return 1


def research_workspace_bytes(layout, batch, n, di, dr, r):
    """hstu_input_preprocess_bwd_workspace_bytes restated: (bytes of the d_pos partials, bytes of the d_rating partials)"""
    a256 = lambda x: (x + 255) // 256 * 256
    n_out, do = n_out_of(layout, n), d_out_of(layout, di, dr)
    pos = a256(bwd_groups(batch, n_out, do) * n_out * do * 4)
    rat = 0 if layout == PLAIN else a256(rating_groups(batch, n) * r * dr * 4)
    return pos, rat


# ------------------------------------------------------------------------------------------------ batches of jagged users
def make_batch(rows, seed):
    """(lengths, num_targets) of exactly `rows` source rows.  A fixed texture repeats: an empty user, a user without
    targets, a user of targets only, a run of nine users of 0 .. 3 rows (empty ones among them: one step of a row slot
    passes several users), two empty users in a row, a long user -- so every slab of a few dozen rows sees all of them"""
    rng = np.random.RandomState(seed)
    lengths, targets, left = [], [], rows

    def add(l, t):
        nonlocal left
        l = min(l, left)
        lengths.append(l)
        targets.append(min(t, l))
        left -= l

    while left > 0:
        add(0, 0)
        add(int(rng.randint(1, 50)), 0)
        k = int(rng.randint(1, 5))
        add(k, k)
        for l in rng.randint(0, 4, 9):
            add(int(l), int(rng.randint(0, 3)))
        add(0, 0)
        add(0, 0)
        add(int(rng.randint(30, 200)), int(rng.randint(0, 9)))
    add(0, 0)                                             # the batch ends with an empty user
    assert sum(lengths) == rows
    return np.asarray(lengths, dtype=np.int64), np.asarray(targets, dtype=np.int64)


def combine_out_rows(lengths, targets, c_len, mode):
    total, t = int(np.sum(lengths)), int(np.sum(targets))
    return len(lengths) * c_len + (total if mode == SUM else 2 * total if mode == INTERLEAVE_ALL else 2 * total - t)


SMALL_LENGTHS = [7, 0, 4, 3, 9, 40, 12, 1, 5, 2, 31, 8, 16, 6, 23, 11, 3]      # the 17 users of tests/test_preprocessor_gpu.py
SMALL_TARGETS = [2, 0, 0, 3, 1, 7, 0, 0, 5, 1, 4, 8, 3, 2, 9, 1, 1]


def rows_of(rule, units, cus):
    """the row count a case asks for: a literal, or
    ("slots", k, rem)   8 CUs x rows_par x k + rem: every workgroup of the capped grid, every row slot walks k rows (+ rem)
    ("groups", g, rem)  8 rows_par x (g - 1) + rem: g slabs of the action backward
    ("clamp", rem)      8 rows_par x (min(2 CUs, 512) + 4) + rem: more slabs than the clamp admits"""
    rp = host_rows_par(units)
    if isinstance(rule, int):
        return rule
    if rule[0] == "slots":
        return K_PRE_BLOCKS_PER_CU * cus * rp * rule[1] + rule[2]
    if rule[0] == "groups":
        return ACTION_BWD_ROWS_PER_SLOT * rp * (rule[1] - 1) + rule[2]
    assert rule[0] == "clamp"
    return ACTION_BWD_ROWS_PER_SLOT * rp * (action_bwd_cap(cus) + 4) + rule[1]


_BATCHES = {}


def batch_of(case, cus):
    """(lengths, num_targets) of a P case: `rows` counts what the kernel's grid is sized from -- source rows for the action
    ops, output rows for the combine forward, source + contextual rows for the combine backward (at least the count asked
    for, and at most a user's worth more: an interleaved output has no odd row count)"""
    key = (p_id(case), cus)
    if key not in _BATCHES:
        _BATCHES[key] = _batch_of(case, cus)
    return _BATCHES[key]


def _batch_of(case, cus):
    if case["rows"] == "small":
        return np.asarray(SMALL_LENGTHS, dtype=np.int64), np.asarray(SMALL_TARGETS, dtype=np.int64)
    want = rows_of(case["rows"], p_units(case), cus)
    if case["kind"] in ("action_fwd", "action_bwd"):
        return make_batch(want, case["seed"])
    src = want                                            # combine: settle the source rows that give `want`
    for _ in range(3):
        lengths, targets = make_batch(src, case["seed"])
        got = p_grid_rows(case, lengths, targets)
        src = max(1, src + int((want - got) * src / max(got, 1)))
    lengths, targets = make_batch(src, case["seed"])
    def short():
        rows = p_grid_rows(case, lengths, targets)
        if rows < want:
            return True
        # the combine backward: the source rows end inside a slab, which then goes on into the contextual rows
        ctx = case["kind"] == "combine_bwd" and case["d_ctx"] and case["C"] > 0
        rp = host_rows_par(p_units(case))
        return ctx and src % slab_rows(rows, resident_blocks(rows, rp, cus)) == 0

    while short():
        src += 1
        lengths, targets = make_batch(src, case["seed"])
    return lengths, targets


# ------------------------------------------------------------------------------------------------ P: preprocess_ops.hip
def _p(kind, label, dtype, rows, idx=64, seed=1, **kw):
    d = dict(kind=kind, label=label, dtype=dtype, rows=rows, idx=idx, seed=seed, mis={}, T=None, da=None, thresholds=(),
             weights=None, D=None, mode=None, C=0, action=True, d_action=True, d_ctx=True)
    d.update(kw)
    return d


def act(kind, label, dtype, T, da, rows, **kw):
    return _p(kind, label, dtype, rows, T=T, da=da, **kw)


def comb(kind, label, dtype, D, mode, C, rows, **kw):
    return _p(kind, label, dtype, rows, D=D, mode=mode, C=C, **kw)


def wide_weights():
    """64 action types: 60 single bits 2^3 .. 2^62 and four combined weights of several bits"""
    return [1 << (t + 3) for t in range(60)] + [0b111, (1 << 62) | 1, (1 << 40) | (1 << 20) | 2, (1 << 62) | (1 << 61)]


WALK, WIDE, BWD_Y, BWD_GROUPS, BWD_CLAMP, MISALIGNED = "P-walk", "P-wide", "P-bwd-y", "P-bwd-groups", "P-bwd-clamp", "P-misaligned"
W3 = ("slots", 3, 7)              # three rows per row slot plus a remainder: trailing workgroups have an empty slab

P_CASES = [
    # ---- P-walk: rows_par 1 (129 .. 256 units), a middle value, 64 (D 24 bf16: 3 pieces of 16 bytes)
    act("action_fwd", WALK, F32, 8, 17, W3, idx=32, thresholds=((30, 4),)),                   # 136 elements: rows_par 1
    act("action_fwd", WALK, BF16, 3, 9, W3, seed=2),                                          # 27 elements: rows_par 8
    act("action_fwd", WALK, BF16, 3, 8, W3, idx=32, seed=3, thresholds=((10, 1), (50, 4))),   # 3 pieces: rows_par 64
    comb("combine_fwd", WALK, F32, 150, SUM, 0, W3, idx=32, seed=4),                          # 150 elements: rows_par 1
    comb("combine_fwd", WALK, BF16, 24, SUM, 3, W3, seed=5),                                  # rows_par 64
    comb("combine_fwd", WALK, F16, 27, SUM, 3, W3, idx=32, seed=6, action=False),             # rows_par 8
    comb("combine_fwd", WALK, BF16, 24, INTERLEAVE_ALL, 0, W3, idx=32, seed=7),
    comb("combine_fwd", WALK, F32, 150, INTERLEAVE_ALL, 3, W3, seed=8),
    comb("combine_fwd", WALK, BF16, 27, INTERLEAVE_UIH, 0, W3, seed=9),
    comb("combine_fwd", WALK, BF16, 24, INTERLEAVE_UIH, 3, W3, idx=32, seed=10),
    comb("combine_fwd", WALK, F32, 150, INTERLEAVE_UIH, 3, W3, seed=11),
    comb("combine_bwd", WALK, F32, 150, SUM, 3, W3, seed=12),
    comb("combine_bwd", WALK, BF16, 27, INTERLEAVE_ALL, 3, W3, idx=32, seed=13),
    comb("combine_bwd", WALK, F16, 27, INTERLEAVE_UIH, 3, W3, seed=14),
    comb("combine_bwd", WALK, BF16, 24, SUM, 0, W3, idx=32, seed=15, d_action=False),
    comb("combine_bwd", WALK, F32, 150, INTERLEAVE_ALL, 3, W3, seed=16, d_ctx=False),
    comb("combine_bwd", WALK, F32, 150, SUM, 3, W3, idx=32, seed=17, d_action=False),
    comb("combine_bwd", WALK, BF16, 24, SUM, 3, W3, seed=18),                                 # (the interleaved d_out would be twice as large)
    comb("combine_bwd", WALK, F32, 150, INTERLEAVE_UIH, 3, W3, idx=32, seed=27),
    # ---- P-wide: more than 256 units per row, the lane loop wraps
    comb("combine_fwd", WIDE, F32, 301, INTERLEAVE_UIH, 3, "small", idx=32),
    comb("combine_fwd", WIDE, BF16, 2056, SUM, 3, "small"),
    comb("combine_fwd", WIDE, BF16, 2056, INTERLEAVE_ALL, 0, "small", idx=32),
    comb("combine_bwd", WIDE, F32, 301, INTERLEAVE_ALL, 3, "small"),
    comb("combine_bwd", WIDE, BF16, 2056, INTERLEAVE_UIH, 3, "small", idx=32),
    act("action_fwd", WIDE, F32, 8, 33, "small", thresholds=((30, 16),)),                     # T Da = 264 elements
    act("action_fwd", WIDE, BF16, 64, 40, 700, idx=32, seed=19, weights="wide"),              # 320 pieces, mask bits up to 63
    # ---- P-bwd-y: the action backward with gridDim.y == 2
    act("action_bwd", BWD_Y, F32, 8, 33, 700, seed=20, thresholds=((30, 16),)),               # 264 elements
    act("action_bwd", BWD_Y, BF16, 64, 40, 700, idx=32, seed=21, weights="wide"),             # 320 pieces
    # ---- P-bwd-groups: 4, 5, 6, 7 slabs -- the finish kernel's unrolled loop with each remainder -- and the clamp
    act("action_bwd", BWD_GROUPS, F32, 4, 8, ("groups", 4, 5), seed=22, groups=4),            # 8 pieces: rows_par 32
    act("action_bwd", BWD_GROUPS, BF16, 4, 8, ("groups", 5, 1), idx=32, seed=23, groups=5, thresholds=((30, 2),)),
    act("action_bwd", BWD_GROUPS, F16, 3, 5, ("groups", 6, 9), seed=24, groups=6),            # 15 elements: rows_par 16
    act("action_bwd", BWD_GROUPS, F32, 4, 8, ("groups", 7, 255), idx=32, seed=25, groups=7),
    act("action_bwd", BWD_CLAMP, F32, 8, 17, ("clamp", 5), seed=26, thresholds=((30, 4),)),   # 136 elements: rows_par 1
    # ---- P-misaligned: Da a 16-byte multiple, one pointer 2 or 4 bytes off: the element path, the aligned call's bits
    act("action_fwd", MISALIGNED, BF16, 4, 8, "small", mis={"table": 4}),
    act("action_fwd", MISALIGNED, BF16, 4, 8, "small", idx=32, mis={"target_table": 4}),
    act("action_fwd", MISALIGNED, BF16, 4, 8, "small", mis={"out": 2}),
    act("action_fwd", MISALIGNED, F32, 4, 8, "small", idx=32, mis={"out": 4}),
    act("action_bwd", MISALIGNED, BF16, 4, 8, "small", idx=32, mis={"d_out": 2}),
    act("action_bwd", MISALIGNED, F32, 4, 8, "small", mis={"d_out": 4}),
]
P_LABELS = (WALK, WIDE, BWD_Y, BWD_GROUPS, BWD_CLAMP, MISALIGNED)


def p_id(c):
    bits = [c["label"], c["kind"], c["dtype"]]
    bits.append(f"T{c['T']}x{c['da']}" if c["T"] else f"D{c['D']}-m{c['mode']}-C{c['C']}")
    bits.append(f"i{c['idx']}")
    if c["kind"] == "combine_fwd" and not c["action"]:
        bits.append("noaction")
    if c["kind"] == "combine_bwd":
        bits += [f for f, on in (("nodaction", not c["d_action"]), ("nodctx", not c["d_ctx"])) if on]
    if c["mis"]:
        bits += [f"{k}+{v}" for k, v in c["mis"].items()]
    if c.get("groups"):
        bits.append(f"g{c['groups']}")
    return "-".join(bits)


def p_row_elems(c):
    """(elements of a row, the count that must be a multiple of the 16-byte piece)"""
    return (c["T"] * c["da"], c["da"]) if c["T"] else (c["D"], c["D"])


def p_vec(c, aligned=False):
    n = pre_pick_vec(p_row_elems(c)[1], c["dtype"], bool(c["mis"]) and not aligned)
    return n


def p_units(c, aligned=False):
    return p_row_elems(c)[0] // p_vec(c, aligned)


def p_grid_rows(c, lengths, targets):
    """the row count the kernel's grid is sized from"""
    total = int(np.sum(lengths))
    if c["kind"] == "combine_fwd":
        return combine_out_rows(lengths, targets, c["C"], c["mode"])
    if c["kind"] == "combine_bwd":
        return total + (len(lengths) * c["C"] if c["d_ctx"] else 0)
    return total


def p_class_facts(c, cus):
    """what the restated geometry says about a P case at `cus` CUs"""
    lengths, targets = batch_of(c, cus)
    rows, units = p_grid_rows(c, lengths, targets), p_units(c)
    rp = host_rows_par(units)
    f = dict(rows=rows, units=units, rows_par=rp, tpr=host_tpr(units), vec=p_vec(c))
    if c["kind"] == "action_bwd":
        f["groups"] = action_bwd_groups(rows, units, cus)
        f["unclamped"] = action_bwd_groups_unclamped(rows, units)
        f["grid_y"] = action_bwd_grid_y(units)
        f["per"] = slab_rows(rows, f["groups"])
    else:
        f["grid"] = resident_blocks(rows, rp, cus)
        f["per"] = slab_rows(rows, f["grid"])
        f["capped"] = f["grid"] == cus * K_PRE_BLOCKS_PER_CU
        f["empty_slabs"] = f["grid"] - ceil_div(rows, f["per"])
    f["rows_per_slot"] = ceil_div(f["per"], rp)
    if c["kind"] == "combine_bwd":
        f["straddles"] = c["d_ctx"] and c["C"] > 0 and int(np.sum(lengths)) % f["per"] != 0
    # users one step of a row slot passes at most, along the offsets the kernel walks
    walked = lengths
    if c["kind"] == "combine_fwd":
        t = np.asarray(targets)
        walked = c["C"] + (lengths if c["mode"] == SUM else 2 * lengths if c["mode"] == INTERLEAVE_ALL else 2 * lengths - t)
    off = np.concatenate([[0], np.cumsum(walked)])
    r = np.arange(0, max(int(off[-1]) - rp, 0))
    user = lambda x: np.searchsorted(off, x, side="right") - 1
    f["max_users_per_step"] = int(np.max(user(r + rp) - user(r))) if r.size else 0
    return f


def p_lands_on_its_label(c, cus):
    f = p_class_facts(c, cus)
    lab = c["label"]
    if lab == WALK:
        # one step passes several users -- where a step can: C contextual rows per user keep a step of <= C output rows
        # from passing more than one
        several = 1 if (c["kind"] == "combine_fwd" and c["C"] >= f["rows_par"]) else 2
        ok = f["capped"] and f["rows_per_slot"] >= 3 and f["empty_slabs"] >= 1 and f["max_users_per_step"] >= several
        return ok and (c["kind"] != "combine_bwd" or not (c["d_ctx"] and c["C"]) or f["straddles"])
    if lab == WIDE:
        return f["units"] > f["tpr"] == K_PRE_THREADS
    if lab == BWD_Y:
        return f["grid_y"] == 2
    if lab == BWD_GROUPS:
        return f["groups"] == c["groups"] == f["unclamped"] and f["grid_y"] == 1
    if lab == BWD_CLAMP:
        return f["unclamped"] > f["groups"] == action_bwd_cap(cus) and f["rows_per_slot"] >= 8
    if lab == MISALIGNED:
        return f["vec"] == 1 and p_vec(c, aligned=True) > 1
    return False


# ------------------------------------------------------------------------------------------------ R: research_preprocess.hip
def _r(label, layout, emb, out, B, N, di, dr=0, R=0, extra_pos=0, p=0.0, seed=0, r64=True, mis=None, v=None, fwd=True,
       unused_rating=None, note=""):
    return dict(label=label, layout=layout, emb=emb, out=out, B=B, N=N, di=di, dr=dr, R=R, extra_pos=extra_pos, p=p, seed=seed,
                r64=r64, mis=dict(mis or {}), v=v, fwd=fwd, unused_rating=unused_rating, note=note)


STRIDE, POS_CLAMP, POS_FEWER, POS_BLOCKS, RATING, MATRIX, LOWERED = ("R-stride", "R-pos-clamp", "R-pos-fewer-slabs", "R-pos-by-blocks",
                                                                    "R-rating", "R-matrix", "R-matrix-lowered")

R_CASES = [
    # ---- R-stride: more than 1024 x 256 pieces, the piece loop takes a second step
    _r(STRIDE, PLAIN, F32, F32, 3, 1029, 257, v=1, extra_pos=2),
    _r(STRIDE, PLAIN, F32, F32, 3, 1029, 257, v=1, p=0.2, seed=0x1234567890ABCDEF),
    _r(STRIDE, INTERLEAVE, BF16, BF16, 2, 520, 2048, 2048, 5, v=8, unused_rating=2),
    # ---- R-pos-groups: the clamp at 64 with 64 slabs, with fewer slabs than groups, the limit by unit blocks
    _r(POS_CLAMP, PLAIN, F32, F32, 512, 9, 64, v=4, extra_pos=3),
    _r(POS_FEWER, CONCAT, F32, F32, 520, 9, 56, 8, 6, v=4, extra_pos=3, r64=False, unused_rating=4),
    # the heaviest case.  ceil(2048 / ub) < min(64, ceil(B / 8)) needs more than (ub - 1) 2048 elements per user and more
    # than 8 ceil(2048 / ub) users; the product of the two is smallest at ub = 36 (57 groups, 457 users); D 64 -> N 1121
    _r(POS_BLOCKS, PLAIN, BF16, BF16, 457, 1121, 64, v=8, extra_pos=1, fwd=False),
    # ---- R-rating: the 256-group clamp; 65 rows per slot and gridDim.z == 2; 32 slots of at least 2 rows
    _r(RATING, CONCAT, F32, F32, 130, 127, 5, 259, 6, v=1, unused_rating=3),
    _r(RATING, INTERLEAVE, BF16, BF16, 200, 100, 64, 64, 6, v=8, r64=False, unused_rating=1, extra_pos=2),
    # ---- R-matrix, B 40, N 9: every (emb, out) pair at every V it admits by size; the layouts take turns
    _r(MATRIX, PLAIN, F32, F32, 40, 9, 64, v=4), _r(MATRIX, CONCAT, F32, F32, 40, 9, 50, 14, 6, v=2, unused_rating=5),
    _r(MATRIX, INTERLEAVE, F32, F32, 40, 9, 67, 67, 6, v=1, r64=False, unused_rating=0),
    _r(MATRIX, CONCAT, BF16, BF16, 40, 9, 56, 8, 6, v=8, unused_rating=2), _r(MATRIX, INTERLEAVE, BF16, BF16, 40, 9, 68, 68, 6, v=4, unused_rating=3),
    _r(MATRIX, PLAIN, BF16, BF16, 40, 9, 66, v=2, extra_pos=2), _r(MATRIX, CONCAT, BF16, BF16, 40, 9, 5, 9, 6, v=1, r64=False, unused_rating=4),
    _r(MATRIX, INTERLEAVE, F16, F16, 40, 9, 64, 64, 6, v=8, unused_rating=1), _r(MATRIX, PLAIN, F16, F16, 40, 9, 68, v=4),
    _r(MATRIX, CONCAT, F16, F16, 40, 9, 50, 14, 6, v=2, r64=False, unused_rating=0, extra_pos=1),
    _r(MATRIX, INTERLEAVE, F16, F16, 40, 9, 67, 67, 6, v=1, unused_rating=5),
    _r(MATRIX, PLAIN, BF16, F32, 40, 9, 64, v=4, extra_pos=2), _r(MATRIX, CONCAT, BF16, F32, 40, 9, 50, 14, 6, v=2, unused_rating=3),
    _r(MATRIX, INTERLEAVE, BF16, F32, 40, 9, 67, 67, 6, v=1, r64=False, unused_rating=2),
    _r(MATRIX, CONCAT, F16, F32, 40, 9, 56, 8, 6, v=4, unused_rating=4), _r(MATRIX, INTERLEAVE, F16, F32, 40, 9, 66, 66, 6, v=2, unused_rating=1),
    _r(MATRIX, PLAIN, F16, F32, 40, 9, 67, v=1),
    _r(MATRIX, PLAIN, F16, F16, 40, 9, 64, v=8, p=0.2, seed=77),
    # ---- V lowered by one pointer 4 or 8 bytes off 16-byte alignment (forward: emb / pos / out; backward: d_emb / d_out)
    _r(LOWERED, PLAIN, BF16, BF16, 40, 9, 64, v=(2, 4), mis={"emb": 4, "d_out": 8}),
    _r(LOWERED, CONCAT, F32, F32, 40, 9, 56, 8, 6, v=(2, 1), mis={"out": 8, "d_emb": 4}, unused_rating=0),
]
R_LABELS = (STRIDE, POS_CLAMP, POS_FEWER, POS_BLOCKS, RATING, MATRIX, LOWERED)
R_PAIRS = ((F32, F32), (BF16, BF16), (F16, F16), (BF16, F32), (F16, F32))
FWD_EMB_ROLES, FWD_OUT_ROLES = ("emb",), ("pos", "rat", "out")
BWD_EMB_ROLES, BWD_OUT_ROLES = ("d_emb",), ("d_out",)        # (the workspace is 32-byte aligned by contract)
LAYOUT_NAMES = {PLAIN: "plain", CONCAT: "concat", INTERLEAVE: "interleave"}


def r_id(c):
    bits = [c["label"], LAYOUT_NAMES[c["layout"]], c["emb"] + ("" if c["emb"] == c["out"] else "-" + c["out"]),
            f"B{c['B']}-N{c['N']}-D{c['di']}" + (f"+{c['dr']}" if c["layout"] == CONCAT else "")]
    if c["p"]:
        bits.append("drop")
    if c["mis"]:
        bits += [f"{k}+{v}" for k, v in c["mis"].items()]
    return "-".join(bits)


def r_vecs(c):
    """(V of the forward, V of the backward) under the restated pick_vec"""
    m = c["mis"]
    fwd = research_pick_vec(c["layout"], c["di"], c["dr"], c["emb"], c["out"], [m.get(k, 0) for k in FWD_EMB_ROLES],
                            [m.get(k, 0) for k in FWD_OUT_ROLES])
    bwd = research_pick_vec(c["layout"], c["di"], c["dr"], c["emb"], c["out"], [m.get(k, 0) for k in BWD_EMB_ROLES],
                            [m.get(k, 0) for k in BWD_OUT_ROLES])
    return fwd, bwd


def r_class_facts(c):
    n_out, do = n_out_of(c["layout"], c["N"]), d_out_of(c["layout"], c["di"], c["dr"])
    vf, vb = r_vecs(c)
    f = dict(n_out=n_out, do=do, v_fwd=vf, v_bwd=vb, units=n_out * (do // vf), gx=unit_blocks(n_out, do, vf))
    f["strides"] = f["units"] > K_MAX_UNIT_BLOCKS * K_THREADS
    f["by_blocks"], f["by_users"] = bwd_groups_by_blocks(n_out, do), bwd_groups_by_users(c["B"])
    f["groups"] = bwd_groups(c["B"], n_out, do)
    f["slabs"], f["users_per_slab"] = slab_count(c["B"], f["groups"])
    if c["layout"] != PLAIN:
        f["rating_groups"] = rating_groups(c["B"], c["N"])
        f["rating_unclamped"] = ceil_div(c["B"] * c["N"], RATING_ROWS_PER_GROUP)
        f["rating_tpr"], f["rating_grid_z"] = rating_tpr(c["dr"], vb), rating_grid_z(c["dr"], vb)
        per = ceil_div(c["B"] * c["N"], f["rating_groups"])
        f["rating_rows_per_group"] = per
        f["rating_rows_per_slot_min"] = per // (K_THREADS // f["rating_tpr"])
    return f


def r_lands_on_its_label(c):
    f = r_class_facts(c)
    lab = c["label"]
    want_v = c["v"] if isinstance(c["v"], tuple) else (c["v"], c["v"])
    if (f["v_fwd"], f["v_bwd"]) != want_v:
        return False
    if lab == STRIDE:
        return f["strides"] and f["gx"] == K_MAX_UNIT_BLOCKS
    if lab == POS_CLAMP:
        return f["by_users"] >= K_BWD_GROUPS_MAX < f["by_blocks"] and f["groups"] == f["slabs"] == K_BWD_GROUPS_MAX
    if lab == POS_FEWER:
        return f["by_users"] > K_BWD_GROUPS_MAX < f["by_blocks"] and f["slabs"] < f["groups"] == K_BWD_GROUPS_MAX
    if lab == POS_BLOCKS:
        return f["groups"] == f["by_blocks"] < min(K_BWD_GROUPS_MAX, f["by_users"])
    if lab == RATING:
        return (f["rating_unclamped"] > f["rating_groups"] == K_RATING_GROUPS_MAX and f["rating_rows_per_slot_min"] >= 2
                and (f["rating_grid_z"] == 2 or K_THREADS // f["rating_tpr"] == 32))
    if lab == MATRIX:
        return not c["mis"] and (c["B"], c["N"]) == (40, 9)
    if lab == LOWERED:
        aligned = dict(c, mis={})
        return bool(c["mis"]) and all(a > b for a, b in zip(r_vecs(aligned), r_vecs(c)))
    return False


def admitted_vs(emb, out):
    """the piece widths a dtype pair admits by size: at most 16 bytes of the output dtype"""
    v, vs = 16 // ELEM_BYTES[out], []
    while v >= 1:
        vs.append(v)
        v >>= 1
    return vs
