"""csrc/embedding_optim_dispatch.h, compiled alone (tests/embedding_optim_probe.py) and swept: the row class and chunk size
against a Python restatement of the rule, the workspace sizes against what the built library reports, the room of the partial
sums, the LDS bytes and the grids -- and the kernels inside the built library against the classes the header can name
(tests/test_kernel_resources.py's reader, nothing else).  No GPU."""

import ctypes as C
import re

import embedding_optim_probe as P
import pytest
import test_kernel_resources as KR

K = P.consts()
NS = (0, 1, 31, 32, 33, 127, 128, 129, K["small_batch"] - 1, K["small_batch"], 2**31 - 1)
SINKS = (("bf16", 1), ("f16", 1), ("f32", 1), ("bf16", 0), ("f16", 0), ("f32", 0))


def _want_class(elem_bytes, dim, n, applies):
    """the rule as the unit spelled it before the header: opt_dispatch's four branches and opt_chunk"""
    row_bytes = dim * elem_bytes
    if row_bytes <= 1024:
        np_, u = 1, 8
    elif row_bytes <= 2048:
        np_, u = 2, 4
    elif elem_bytes == 4 and applies and row_bytes > 4096:
        np_, u = 8, 2
    else:
        np_, u = 4, (2 if elem_bytes == 2 else 4)
    return np_, u, (32 if n < 262144 and dim <= 512 else 128)


def _ceil(a, b):
    return (a + b - 1) // b


def test_the_constants_are_the_ones_the_kernels_were_built_around():
    assert (K["chunk_large"], K["chunk_small"], K["small_batch"], K["small_chunk_max_dim"]) == (128, 32, 262144, 512)
    assert (K["opt_waves"], K["combine_waves"], K["max_pieces"], K["max_dim"], K["max_blocks"]) == (4, 8, 4, 2048, 8192)
    assert (K["scan_threads"], K["scan_items"], K["scan_tile"], K["tile_scan_threads"]) == (256, 8, 2048, 1024)
    # 16-bit rows: 4 KiB everywhere; fp32 rows: 8 KiB where the entry point takes the coalesced lists of wide tables
    assert P.max_row_bytes() == {(2, False): 4096, (2, True): 4096, (4, False): 4096, (4, True): 8192}


@pytest.mark.parametrize("dtype,applies", SINKS)
def test_every_legal_row_and_batch_gets_todays_class_grids_and_room(dtype, applies):
    eb = P.DTYPES[dtype]
    plans = P.sweep(dtype, applies, NS)
    widest = P.max_row_bytes()[(eb, bool(applies))]
    assert sorted({d for d, _ in plans}) == list(range(16 // eb, widest // eb + 1, 16 // eb))     # every 16-byte multiple
    assert max(d for d, _ in plans) == (K["max_dim"] if applies or eb == 2 else 1024)
    for (dim, n), p in plans.items():
        where = (dtype, applies, dim, n, p)
        assert (p["np"], p["u"], p["chunk"]) == _want_class(eb, dim, n, applies), where
        assert 64 * p["np"] * 16 >= dim * eb, where                                # the lanes' pieces cover the row
        chunks = _ceil(n, p["chunk"])
        assert p["chunks"] == chunks, where
        assert p["chunk_grid"] == min(_ceil(chunks, K["opt_waves"]), K["max_blocks"]), where
        assert p["combine_grid"] == (0 if chunks < 2 else min(chunks - 1, K["max_blocks"])), where
        assert p["scan_tiles"] == _ceil(n, K["scan_tile"]) and p["scan_grid"] == min(p["scan_tiles"], K["max_blocks"]), where
        assert max(p["chunk_grid"], p["combine_grid"], p["scan_grid"]) <= K["max_blocks"], where
        assert p["combine_lds"] == (K["combine_waves"] - 1) * dim * 4 <= 56 * 1024, where
        # two partial sums per chunk at the row's own width fit the room laid out for large chunks of the widest row
        assert p["partials_bytes"] == 2 * chunks * dim * 4 <= p["partials_room"], where


def test_the_workspace_sizes_are_the_librarys():
    from generative_recommenders_amd import _lib

    lib = _lib.lib()
    for rows in (1, 2**16, 2**24, 10**7):
        for n in NS:
            opt, coalesce = C.c_int64(-1), C.c_int64(-1)
            assert lib.hstu_embedding_rowwise_adagrad_workspace_bytes(n, rows, C.byref(opt)) == 0
            assert lib.hstu_embedding_grad_coalesce_workspace_bytes(n, rows, C.byref(coalesce)) == 0
            # the sort's temporary is the one number the header takes from outside (rocprim's): read it off the first size
            temp = opt.value - P.layout(n, 0)["opt_total"]
            assert temp >= 0 and temp % 256 == 0 and (n > 0 or temp == 0), (rows, n, temp)
            l = P.layout(n, temp)
            assert l["opt_total"] == opt.value and l["total"] == coalesce.value, (rows, n, l)
            assert l["part"] >= 4 * n and l["partials_off"] == 2 * l["part"] and l["rank_off"] == l["opt_total"], (rows, n, l)
            assert l["temp_off"] - l["partials_off"] >= 2 * _ceil(n, K["chunk_large"]) * K["max_dim"] * 4, (rows, n, l)
            assert l["tiles_off"] - l["rank_off"] >= 4 * n and l["total"] - l["tiles_off"] >= 4 * _ceil(n, K["scan_tile"]), (rows, n, l)
            assert all(v % 256 == 0 for k, v in l.items() if k != "temp_bytes"), (rows, n, l)


_T = {"DF16b": "bf16", "DF16_": "f16", "f": "f32"}


def _optimizer_kernels():
    ks = KR._kernels()
    chunk = {k: v for k, v in ks.items() if "optim_chunk_kernel" in k}
    combine = {k: v for k, v in ks.items() if "optim_combine_kernel" in k}
    return chunk, combine


def test_the_library_holds_exactly_the_classes_the_header_can_name():
    chunk, combine = _optimizer_kernels()
    want_chunk = {s: {(p["np"], p["u"], p["chunk"]) for p in P.sweep(*s, NS).values()} for s in SINKS}
    # the header's own list of what it compiles is the sweep's
    assert P.reachable() == {(P.DTYPES[d], a) + c for (d, a), cs in want_chunk.items() for c in cs}
    got_chunk, got_combine = {}, {}
    for name in chunk:
        m = re.match(r"_ZN4hstu18optim_chunk_kernelI(DF16b|DF16_|f)Li(\d+)ELi(\d+)ELi(\d+)ENS_(\d+)(EmitSink|UpdateSink)(.*?)EEvP", name)
        assert m, name
        sink = m.group(6) + m.group(7)
        got_chunk.setdefault((sink, _T[m.group(1)]), set()).add(tuple(int(m.group(i)) for i in (2, 3, 4)))
    for name in combine:
        m = re.match(r"_ZN4hstu20optim_combine_kernelILi(\d+)ELi(\d+)ELi(\d+)ENS_(\d+)(EmitSink|UpdateSink)(.*?)EEvP", name)
        assert m, name
        got_combine.setdefault(m.group(5) + m.group(6), set()).add(tuple(int(m.group(i)) for i in (1, 2, 3)))
    sinks = sorted({s for s, _ in got_chunk})
    assert len(sinks) == 10 and sum(s.startswith("UpdateSink") for s in sinks) == 9, sinks    # three rules x three table types, and the coalesce
    assert sorted(got_combine) == sinks
    for sink in sinks:
        applies = int(sink.startswith("UpdateSink"))
        for dtype in P.DTYPES:
            assert got_chunk[(sink, dtype)] == want_chunk[(dtype, applies)], (sink, dtype)
        want = {(16 // P.DTYPES[d], np_, c) for d in P.DTYPES for np_, _, c in want_chunk[(d, applies)]}
        assert got_combine[sink] == want, sink
    assert (len(chunk), len(combine)) == (139, 99)


def test_no_optimizer_kernel_spills_or_uses_scratch():
    chunk, combine = _optimizer_kernels()
    assert chunk and combine
    for name, v in {**chunk, **combine}.items():
        assert v["scratch"] == 0 and v["spill"] == 0, (name, v)
