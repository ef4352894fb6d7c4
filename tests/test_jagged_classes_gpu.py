"""Every copy width of the 2-D jagged helpers (csrc/jagged_ops.hip), bit for bit against the numpy oracle.

The rows of tests/jagged_class_cases.py -- each labelled with the width V it is meant to reach -- run here through the C
ABI with raw pointers.  Every tensor of a call sits alone inside a sentinel-filled byte allocation, off 16-byte alignment
by the bytes its row says, so that
  * the label is checked against the actual pointers before the launch (a row that drifts to another width fails),
  * the output is compared byte for byte with the oracle (oracle/hstu_oracle.py; write_tail: a few lines of numpy),
  * every byte the oracle does not write -- the guard bands, the rows of a truncated user, the rows in front of a tail,
    two spare rows behind every output -- must still hold the sentinel, and
  * the inputs must come back unchanged."""

import zlib

import numpy as np
import pytest
import torch

import jagged_class_cases as T
from oracle import hstu_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0xA5            # payload bytes are drawn from 1 .. 0x9F: neither the sentinel nor the zero fill
SPARE_ROWS = 2         # allocated behind every output, never to be written


def _lib():
    from generative_recommenders_amd import _lib as L

    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Bytes:
    """(rows, row_bytes) bytes, `off` bytes into their own sentinel-filled allocation"""

    def __init__(self, rows, row_bytes, off, data=None):
        self.rows, self.row_bytes, self.off, self.n = rows, row_bytes, off, rows * row_bytes
        self.buf = torch.full((off + self.n + T.GUARD,), SENT, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 256 == 0      # what the layout of jagged_class_cases (and the CPU test of it) assumes
        if data is not None:
            assert data.shape == (rows, row_bytes) and data.dtype == np.uint8
            self.buf[off:off + self.n].copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(-1))
        self.before = self.buf.cpu().numpy().copy()

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def check(self, want, what):
        """payload == want byte for byte, and both guard bands still hold the sentinel"""
        flat = self.buf.cpu().numpy()
        assert (flat[:self.off] == SENT).all(), f"{what}: bytes in front of the tensor were written"
        assert (flat[self.off + self.n:] == SENT).all(), f"{what}: bytes behind the tensor were written"
        got = flat[self.off:self.off + self.n].reshape(self.rows, self.row_bytes)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: {len(bad)} bytes differ, the first at (row, byte) {bad[0].tolist()}"

    def unchanged(self, what):
        assert np.array_equal(self.buf.cpu().numpy(), self.before), f"{what}: an input was written"


def _payload(rng, rows, row_bytes):
    return rng.integers(1, 0xA0, size=(rows, row_bytes), dtype=np.uint8)


def _offsets(lengths, idx):
    off = O.complete_cumsum(np.asarray(lengths, dtype=np.int32 if idx == 32 else np.int64))
    return off, torch.from_numpy(off).to(DEV)


def _with_spare(want, row_bytes):
    """the oracle's rows, then SPARE_ROWS rows that nothing may write"""
    return np.concatenate([want, np.full((SPARE_ROWS, row_bytes), SENT, dtype=np.uint8)], axis=0)


def _assert_label(k, *ptrs):
    got = T.width_rule(k["row_bytes"], *ptrs)
    assert got == k["v"], f"{T.case_id(k)}: meant for V = {k['v']}, these pointers give V = {got}"


def _cases(*kinds):
    return [pytest.param(k, id=T.case_id(k)) for k in T.CASES if k["kind"] in kinds]


@pytest.mark.parametrize("k", _cases("concat", "split"))
def test_concat_split_widths(k):
    L = _lib()
    lib, cid, rb, npre = L.lib(), T.case_id(k), k["row_bytes"], k["n_prefix"]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    sh = T.CS_SHAPES[k["shape"]]
    dense_l, dense_r = isinstance(sh["left"], int), isinstance(sh["right"], int)
    B = sh["batch"] if dense_l and dense_r else len(sh["right"] if dense_l else sh["left"])
    assert 3 <= B <= 6
    ll = [sh["left"]] * B if dense_l else sh["left"]
    lr = [sh["right"]] * B if dense_r else sh["right"]
    ml, mr = max(ll), max(lr)
    ol, ol_d = _offsets(ll, k["idx"])
    orr, or_d = _offsets(lr, k["idx"])
    nl, nr = int(ol[-1]), int(orr[-1])
    o_args = (None if dense_l else ol, None if dense_r else orr)
    p_args = (None if dense_l else ol_d.data_ptr(), None if dense_r else or_d.data_ptr())
    tail_args = (ml, mr, sh["max_seq_len"], B, rb // k["elem"], k["elem"], npre, L.HSTU_INDEX_I32 if k["idx"] == 32 else L.HSTU_INDEX_I64,
                 _stream())
    off = lambda role: T.offset(k, role)
    if k["kind"] == "concat":
        left, right = _payload(rng, nl, rb), _payload(rng, nr, rb)
        LEFT, RIGHT = Bytes(nl, rb, off("left"), left), Bytes(nr, rb, off("right"), right)
        OUT = Bytes(nl + nr + SPARE_ROWS, rb, off("out"))
        _assert_label(k, LEFT.ptr, RIGHT.ptr, OUT.ptr)
        L.check(lib.hstu_concat_2d_jagged(LEFT.ptr, RIGHT.ptr, OUT.ptr, *p_args, *tail_args))
        torch.cuda.synchronize()
        want = O.concat_2D_jagged(left, right, ml, mr, *o_args, n_prefix_from_right=npre)
        assert want.shape == (nl + nr, rb)
        OUT.check(_with_spare(want, rb), f"{cid} out")
        LEFT.unchanged(f"{cid} left"), RIGHT.unchanged(f"{cid} right")
    else:
        comb = _payload(rng, nl + nr, rb)
        IN = Bytes(nl + nr, rb, off("out"), comb)
        LEFT, RIGHT = Bytes(nl + SPARE_ROWS, rb, off("left")), Bytes(nr + SPARE_ROWS, rb, off("right"))
        _assert_label(k, LEFT.ptr, RIGHT.ptr, IN.ptr)
        L.check(lib.hstu_split_2d_jagged(IN.ptr, LEFT.ptr, RIGHT.ptr, *p_args, *tail_args))
        torch.cuda.synchronize()
        wl, wr = O.split_2D_jagged(comb, ml if dense_l else None, mr if dense_r else None, *o_args, n_prefix_to_right=npre)
        assert wl.shape == (nl, rb) and wr.shape == (nr, rb)
        LEFT.check(_with_spare(wl, rb), f"{cid} left"), RIGHT.check(_with_spare(wr, rb), f"{cid} right")
        IN.unchanged(f"{cid} in")


@pytest.mark.parametrize("k", _cases("to_dense", "to_jagged"))
def test_padded_dense_widths(k):
    L = _lib()
    lib, cid, rb = L.lib(), T.case_id(k), k["row_bytes"]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    sh = T.PD_SHAPES[k["shape"]]
    lengths, max_len = sh["lengths"], sh["max_len"]
    B = len(lengths)
    assert 3 <= B <= 6 and max(lengths) > max_len and max_len in lengths and 0 in lengths
    offs, offs_d = _offsets(lengths, k["idx"])
    total = int(offs[-1])
    args = (offs_d.data_ptr(), B, max_len, rb // k["elem"], k["elem"], L.HSTU_INDEX_I32 if k["idx"] == 32 else L.HSTU_INDEX_I64, _stream())
    off = lambda role: T.offset(k, role)
    if k["kind"] == "to_dense":
        vals = _payload(rng, total, rb)
        VALUES, DENSE = Bytes(total, rb, off("values"), vals), Bytes(B * max_len + SPARE_ROWS, rb, off("dense"))
        _assert_label(k, VALUES.ptr, DENSE.ptr)
        L.check(lib.hstu_jagged_to_padded_dense(VALUES.ptr, DENSE.ptr, *args))
        torch.cuda.synchronize()
        want = O.jagged_to_padded_dense(vals, offs, max_len).reshape(B * max_len, rb)
        DENSE.check(_with_spare(want, rb), f"{cid} dense")
        VALUES.unchanged(f"{cid} values")
    else:
        dense = _payload(rng, B * max_len, rb)
        DENSE, VALUES = Bytes(B * max_len, rb, off("dense"), dense), Bytes(total + SPARE_ROWS, rb, off("values"))
        _assert_label(k, VALUES.ptr, DENSE.ptr)
        L.check(lib.hstu_dense_to_jagged(DENSE.ptr, VALUES.ptr, *args))
        torch.cuda.synchronize()
        d3 = dense.reshape(B, max_len, rb)
        # the oracle zero-fills the rows it does not write (a user's rows past max_len): the same call on all-ones tells which
        wrote = O.dense_to_jagged(np.ones_like(d3), offs) == 1
        assert not wrote.all() and wrote.any()
        want = np.where(wrote, O.dense_to_jagged(d3, offs), SENT).astype(np.uint8)
        VALUES.check(_with_spare(want, rb), f"{cid} values")
        DENSE.unchanged(f"{cid} dense")


@pytest.mark.parametrize("k", _cases("write_tail"))
def test_write_tail_widths(k):
    L = _lib()
    lib, cid, rb, tail = L.lib(), T.case_id(k), k["row_bytes"], k["tail"]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    lengths = T.wt_lengths(tail)
    B = len(lengths)
    assert 3 <= B <= 6 and tail in lengths and min(lengths) >= tail
    offs, offs_d = _offsets(lengths, k["idx"])
    total = int(offs[-1])
    dense = _payload(rng, B * tail, rb)
    off = lambda role: T.offset(k, role)
    DENSE, VALUES = Bytes(B * tail, rb, off("dense"), dense), Bytes(total + SPARE_ROWS, rb, off("values"))
    _assert_label(k, DENSE.ptr, VALUES.ptr)
    L.check(lib.hstu_jagged_write_tail(DENSE.ptr, VALUES.ptr, offs_d.data_ptr(), B, tail, rb // k["elem"], k["elem"],
                                       L.HSTU_INDEX_I32 if k["idx"] == 32 else L.HSTU_INDEX_I64, _stream()))
    torch.cuda.synchronize()
    want = np.full((total + SPARE_ROWS, rb), SENT, dtype=np.uint8)
    for b in range(B):
        end = int(offs[b + 1])
        want[end - tail:end] = dense[b * tail:(b + 1) * tail]
    VALUES.check(want, f"{cid} values")
    DENSE.unchanged(f"{cid} dense")
