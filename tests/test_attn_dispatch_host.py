"""CPU test of the attention dispatch: the kernel names and the backward's workspace size over a fixed grid of shapes,
against the values recorded from the commit before the dispatch plan (tests/golden/attn_dispatch.json.gz).  No kernel is
launched: the library's name and workspace functions run without a device (256 compute units are assumed then)."""

import ctypes as C
import gzip
import itertools
import json
import os

import pytest

DTYPES = (0, 1, 2)                      # HSTU_DTYPE_BF16, _F16, _F32
DIMS = (16, 32, 64, 128)
LENGTHS = (32, 61, 64, 65, 200, 224, 225, 256, 2048)
HEADS = (1, 4)
BATCHES = (3, 130, 600)
BIASES = (False, "position", True)      # as _launch._shape_params: no bias, the position table only, both tables (128 buckets)
CONTEXTUAL = (0, 4)
DETERMINISTIC = (0, 1)


def grid():
    return itertools.product(DTYPES, DIMS, DIMS, LENGTHS, HEADS, BATCHES, BIASES, CONTEXTUAL, DETERMINISTIC)


def dispatch_of(lib, row):
    """(forward name, backward name, backward workspace bytes) of one grid row; a name the library refuses is None"""
    from generative_recommenders_amd import _lib

    dtype, dqk, dv, n, heads, batch, bias, ctx, det = row
    bp = _lib.HstuAttnBwdParams()
    p = bp.fwd
    p.batch, p.heads, p.dqk, p.dv, p.max_seq_len = batch, heads, dqk, dv, n
    p.alpha, p.scale = 1.0, 1.0 / n
    p.contextual_seq_len = ctx
    p.dtype = dtype
    if bias:
        p.pos_w = 1                      # only NULL / non-NULL is looked at
        if bias is True:
            p.ts_w, p.timestamps, p.num_buckets = 1, 1, 128
    bp.total_rows = batch * n
    bp.deterministic = det
    buf = C.create_string_buffer(128)
    fwd = buf.value.decode() if lib.hstu_attn_fwd_kernel_name(C.byref(p), buf, 128) == 0 else None
    bwd = buf.value.decode() if lib.hstu_attn_bwd_kernel_name(C.byref(bp), buf, 128) == 0 else None
    return fwd, bwd, int(lib.hstu_attn_bwd_workspace_bytes(C.byref(bp)))


def test_dispatch_table_matches_the_recorded_one(golden_dir):
    from generative_recommenders_amd import _lib

    lib = _lib.lib()
    with gzip.open(os.path.join(golden_dir, "attn_dispatch.json.gz"), "rt") as f:
        rec = json.load(f)
    names = rec["names"]
    rows = list(grid())
    assert len(rows) == len(rec["fwd"]) == len(rec["bwd"]) == len(rec["workspace"])
    bad = []
    for i, row in enumerate(rows):
        fwd, bwd, ws = dispatch_of(lib, row)
        want_fwd, want_bwd, want_ws = names[rec["fwd"][i]], names[rec["bwd"][i]], rec["workspace"][i]
        ok = fwd == want_fwd and bwd == want_bwd
        if not row[6]:
            ok = ok and ws == want_ws                    # without bias: the same bytes
        if want_ws == 0:
            ok = ok and ws == 0                          # a path that needed no workspace still needs none
        if not ok:
            bad.append((row, (fwd, bwd, ws), (want_fwd, want_bwd, want_ws)))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ, the first: {bad[:3]}"


def test_solo_bias_workspace_covers_its_rows():
    """one head, 130 users of up to 61 rows: both length classes write min(B, CUs) + min(B, 2 CUs) partial rows, and the
    reduce its chunk sums behind them"""
    from generative_recommenders_amd import _lib

    lib = _lib.lib()
    for batch in (130, 256, 600):
        fwd, bwd, ws = dispatch_of(lib, (0, 16, 16, 61, 1, batch, True, 0, 0))
        assert bwd == "hstu_attn_bwd_solo_bias_kernel<bf16>"
        rows = min(batch, 256) + min(batch, 512)
        assert ws >= (rows + 1) * (2 * 61 + 128) * 4
