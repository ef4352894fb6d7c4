"""The copy-width matrix of the 2-D jagged helpers (csrc/jagged_ops.hip): one literal table of calls, each with the copy
width V it is MEANT to reach.  tests/test_jagged_classes_gpu.py runs every row on the GPU, bit for bit against the numpy
oracle; tests/test_host_logic.py checks without a GPU that every row lands on its label and that the labels cover every
launch line of the three ``switch (v)`` blocks.

The rule (pick_vec): V = the lowest set bit of ``row_bytes | pointers...``, capped at 16.

Layout shared by both: every tensor of a call lives alone in a sentinel-filled byte allocation (256-byte aligned, which is
what torch's allocator hands out), GUARD bytes from its start plus the bytes ``mis`` lists for its role.  The kernels copy
bytes, so every payload is bytes; ``elem`` (1, 2 or 4) only sets how ``row_bytes`` is handed over as dim x elem_bytes.

Kernels:  concat / split      roles left, right, out   (out: the combined side -- split's input)
          to_dense / to_jagged roles values, dense     (jagged_to_padded_dense / dense_to_jagged)
          write_tail          roles dense, values
"""

GUARD = 256                 # bytes in front of and behind every tensor (the issue asks for 64 at least)
WIDTHS = (16, 8, 4, 2, 1)
K_ROWS_PER_BLOCK = 16       # jagged_ops.hip: kRowsPerBlock
K_COPY_THREADS = 256        # jagged_ops.hip: kCopyThreads -- a row of more than 256 * V bytes takes copy_row's loop twice

ROLES = {
    "concat": ("left", "right", "out"), "split": ("left", "right", "out"),
    "to_dense": ("values", "dense"), "to_jagged": ("values", "dense"),
    "write_tail": ("dense", "values"),
}

# ---- shapes.  concat / split: per-user lengths of both sides; a side given as an int is dense (NULL offsets).
# "jj": an empty user; totals of 16 and 17 (the two sides of kRowsPerBlock); user 3's total is max_seq_len; right lengths
#       of 0 and of 2 (below n_prefix = 3)
# "dl" / "dr": one side dense; "dl" keeps the right lengths 0 and 2, so n_prefix meets a short right side AND a dense left
# "dd": both dense (concat only)
CS_SHAPES = {
    "jj": dict(left=[0, 16, 5, 17, 3, 10], right=[0, 0, 2, 14, 14, 7], max_seq_len=31),
    "dl": dict(left=4, right=[0, 12, 13, 2, 27], max_seq_len=31),
    "dr": dict(left=[0, 11, 12, 26, 1], right=5, max_seq_len=31),
    "dd": dict(left=9, right=8, batch=3, max_seq_len=17),
}
# padded: an empty user, 16 and 17 rows, one of exactly max_len, one longer than max_len (truncated)
PD_SHAPES = {
    "a": dict(lengths=[0, 16, 17, 20, 25, 3], max_len=20),
    "b": dict(lengths=[33, 0, 32, 16, 1], max_len=32),
}


def wt_lengths(tail):
    """write_tail: user 0's whole region is the tail; nobody is shorter than the tail (the op's contract)"""
    return [tail, tail + 5, 40, tail + 16, tail + 1]


def c(kind, v, row_bytes, elem, shape=None, np=0, idx=64, mis=None, tail=None, why="size"):
    assert row_bytes % elem == 0 and (why in ("size", "tiny", "long") or why.startswith("mis-"))
    return dict(kind=kind, v=v, row_bytes=row_bytes, elem=elem, shape=shape, n_prefix=np, idx=idx, mis=dict(mis or {}),
                tail=tail, why=why)


def m(kind, role, by, elem, **kw):
    """row_bytes = 48 (a 16-byte multiple); ONE pointer `by` bytes off 16-byte alignment, so V = by"""
    return c(kind, by, 48, elem, mis={role: by}, why="mis-" + role, **kw)


CASES = [
    # ------------------------------------------------------------------------------------------------ concat
    # V by the row size alone, row_bytes == V: one lane per row, 256 rows in flight
    c("concat", 16, 16, 4, "jj", why="tiny"), c("concat", 8, 8, 4, "dl", np=1, idx=32, why="tiny"),
    c("concat", 4, 4, 4, "dr", np=3, why="tiny"), c("concat", 2, 2, 2, "dd", idx=32, why="tiny"),
    c("concat", 1, 1, 1, "jj", np=3, idx=32, why="tiny"),
    # V by the row size alone
    c("concat", 16, 96, 4, "dd", np=1), c("concat", 8, 40, 4, "jj", np=1, idx=32), c("concat", 4, 28, 4, "dl", np=3),
    c("concat", 2, 14, 2, "dr", idx=32), c("concat", 1, 13, 1, "dl"),
    # V by one misaligned pointer
    m("concat", "left", 8, 4, shape="jj", np=3), m("concat", "left", 4, 4, shape="dl", idx=32),
    m("concat", "left", 2, 2, shape="dr", np=1), m("concat", "left", 1, 1, shape="dd", np=3, idx=32),
    m("concat", "right", 8, 4, shape="dl", np=1), m("concat", "right", 4, 4, shape="dr", np=3, idx=32),
    m("concat", "right", 2, 2, shape="dd"), m("concat", "right", 1, 1, shape="jj", np=1, idx=32),
    m("concat", "out", 8, 4, shape="dr", idx=32), m("concat", "out", 4, 4, shape="dd", np=1),
    m("concat", "out", 2, 2, shape="jj", np=3, idx=32), m("concat", "out", 1, 1, shape="dl", np=3),
    # more than 256 * V bytes per row: copy_row loops
    c("concat", 16, 6144, 4, "jj", np=3, why="long"), c("concat", 8, 3080, 4, "dr", np=1, idx=32, why="long"),
    c("concat", 4, 1540, 4, "dl", why="long"), c("concat", 2, 770, 2, "jj", idx=32, why="long"),
    c("concat", 1, 1001, 1, "dd", np=1, why="long"),
    # ------------------------------------------------------------------------------------------------ split
    c("split", 16, 16, 4, "dl", np=3, idx=32, why="tiny"), c("split", 8, 8, 4, "jj", np=3, why="tiny"),
    c("split", 4, 4, 4, "jj", idx=32, why="tiny"), c("split", 2, 2, 2, "dr", np=1, why="tiny"),
    c("split", 1, 1, 1, "dl", np=1, idx=32, why="tiny"),
    c("split", 16, 96, 4, "jj", np=1), c("split", 8, 40, 4, "dr", np=3, idx=32), c("split", 4, 28, 4, "jj", np=3),
    c("split", 2, 14, 2, "dl", idx=32), c("split", 1, 13, 1, "jj", np=1),
    m("split", "left", 8, 4, shape="dl", np=3), m("split", "left", 4, 4, shape="jj", np=1, idx=32),
    m("split", "left", 2, 2, shape="jj", np=3), m("split", "left", 1, 1, shape="dr", idx=32),
    m("split", "right", 8, 4, shape="jj", idx=32), m("split", "right", 4, 4, shape="dl", np=1),
    m("split", "right", 2, 2, shape="dr", np=3, idx=32), m("split", "right", 1, 1, shape="jj", np=3),
    m("split", "out", 8, 4, shape="jj", np=1), m("split", "out", 4, 4, shape="dr", np=1, idx=32),
    m("split", "out", 2, 2, shape="dl", np=3), m("split", "out", 1, 1, shape="jj", idx=32),
    c("split", 16, 6144, 4, "dl", np=1, idx=32, why="long"), c("split", 8, 3080, 4, "jj", np=3, why="long"),
    c("split", 4, 1540, 4, "dr", np=3, idx=32, why="long"), c("split", 2, 770, 2, "jj", np=1, why="long"),
    c("split", 1, 1001, 1, "jj", np=3, idx=32, why="long"),
    # ------------------------------------------------------------------------------------------------ jagged -> padded dense
    c("to_dense", 16, 16, 4, "a", why="tiny"), c("to_dense", 8, 8, 4, "b", idx=32, why="tiny"),
    c("to_dense", 4, 4, 4, "a", idx=32, why="tiny"), c("to_dense", 2, 2, 2, "b", why="tiny"),
    c("to_dense", 1, 1, 1, "a", why="tiny"),
    c("to_dense", 16, 96, 4, "b", idx=32), c("to_dense", 8, 40, 4, "a"), c("to_dense", 4, 28, 4, "b"),
    c("to_dense", 2, 14, 2, "a", idx=32), c("to_dense", 1, 13, 1, "b", idx=32),
    m("to_dense", "values", 8, 4, shape="a"), m("to_dense", "values", 4, 4, shape="b", idx=32),
    m("to_dense", "values", 2, 2, shape="a", idx=32), m("to_dense", "values", 1, 1, shape="b"),
    m("to_dense", "dense", 8, 4, shape="b", idx=32), m("to_dense", "dense", 4, 4, shape="a"),
    m("to_dense", "dense", 2, 2, shape="b"), m("to_dense", "dense", 1, 1, shape="a", idx=32),
    c("to_dense", 16, 6144, 4, "a", idx=32, why="long"), c("to_dense", 8, 3080, 4, "b", why="long"),
    c("to_dense", 4, 1540, 4, "a", why="long"), c("to_dense", 2, 770, 2, "b", idx=32, why="long"),
    c("to_dense", 1, 1001, 1, "a", idx=32, why="long"),
    # ------------------------------------------------------------------------------------------------ padded dense -> jagged
    c("to_jagged", 16, 16, 4, "b", idx=32, why="tiny"), c("to_jagged", 8, 8, 4, "a", why="tiny"),
    c("to_jagged", 4, 4, 4, "b", why="tiny"), c("to_jagged", 2, 2, 2, "a", idx=32, why="tiny"),
    c("to_jagged", 1, 1, 1, "b", idx=32, why="tiny"),
    c("to_jagged", 16, 96, 4, "a"), c("to_jagged", 8, 40, 4, "b", idx=32), c("to_jagged", 4, 28, 4, "a", idx=32),
    c("to_jagged", 2, 14, 2, "b"), c("to_jagged", 1, 13, 1, "a"),
    m("to_jagged", "values", 8, 4, shape="b"), m("to_jagged", "values", 4, 4, shape="a", idx=32),
    m("to_jagged", "values", 2, 2, shape="b", idx=32), m("to_jagged", "values", 1, 1, shape="a"),
    m("to_jagged", "dense", 8, 4, shape="a", idx=32), m("to_jagged", "dense", 4, 4, shape="b"),
    m("to_jagged", "dense", 2, 2, shape="a"), m("to_jagged", "dense", 1, 1, shape="b", idx=32),
    c("to_jagged", 16, 6144, 4, "b", why="long"), c("to_jagged", 8, 3080, 4, "a", idx=32, why="long"),
    c("to_jagged", 4, 1540, 4, "b", idx=32, why="long"), c("to_jagged", 2, 770, 2, "a", why="long"),
    c("to_jagged", 1, 1001, 1, "a", why="long"),
    # ------------------------------------------------------------------------------------------------ write_tail
    c("write_tail", 16, 16, 4, tail=1, why="tiny"), c("write_tail", 8, 8, 4, tail=16, idx=32, why="tiny"),
    c("write_tail", 4, 4, 4, tail=17, why="tiny"), c("write_tail", 2, 2, 2, tail=17, idx=32, why="tiny"),
    c("write_tail", 1, 1, 1, tail=16, why="tiny"),
    c("write_tail", 16, 96, 4, tail=17, idx=32), c("write_tail", 8, 40, 4, tail=1), c("write_tail", 4, 28, 4, tail=16, idx=32),
    c("write_tail", 2, 14, 2, tail=1), c("write_tail", 1, 13, 1, tail=17, idx=32),
    m("write_tail", "dense", 8, 4, tail=16), m("write_tail", "dense", 4, 4, tail=17, idx=32),
    m("write_tail", "dense", 2, 2, tail=1, idx=32), m("write_tail", "dense", 1, 1, tail=16),
    m("write_tail", "values", 8, 4, tail=17, idx=32), m("write_tail", "values", 4, 4, tail=1),
    m("write_tail", "values", 2, 2, tail=16), m("write_tail", "values", 1, 1, tail=17, idx=32),
    c("write_tail", 16, 6144, 4, tail=17, why="long"), c("write_tail", 8, 3080, 4, tail=16, idx=32, why="long"),
    c("write_tail", 4, 1540, 4, tail=1, idx=32, why="long"), c("write_tail", 2, 770, 2, tail=17, why="long"),
    c("write_tail", 1, 1001, 1, tail=16, why="long"),
]


def case_id(k):
    bits = [k["kind"], f"v{k['v']}", k["why"], f"{k['row_bytes']}B", f"e{k['elem']}"]
    if k["shape"]:
        bits.append(k["shape"])
    if k["tail"]:
        bits.append(f"tail{k['tail']}")
    if k["n_prefix"]:
        bits.append(f"np{k['n_prefix']}")
    bits.append(f"i{k['idx']}")
    return "-".join(bits)


def offset(k, role):
    """bytes between the start of a role's (256-byte aligned) allocation and its first byte"""
    return GUARD + k["mis"].get(role, 0)


def width_rule(row_bytes, *ptrs):
    """pick_vec restated: the lowest set bit of row_bytes | pointers, capped at 16"""
    bits = row_bytes
    for p in ptrs:
        bits |= p
    return min(bits & -bits, 16)


# ---- what the table must hold, per kernel (checked by tests/test_host_logic.py)
def required(kind):
    """(why, V) pairs every kernel needs: each width by the row size alone, by a row of exactly V bytes and by a row
    of more than 256 * V bytes; each of 8, 4, 2, 1 by one misaligned pointer, every role in turn"""
    need = {(why, v) for why in ("size", "tiny", "long") for v in WIDTHS}
    need |= {("mis-" + role, v) for role in ROLES[kind] for v in WIDTHS[1:]}
    return need
