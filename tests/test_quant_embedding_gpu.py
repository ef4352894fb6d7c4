"""The int8 row-wise quantized embedding kernels on the GPU, through the C ABI and through the module.

The test owns every output: each lives alone in a 0xFF-filled allocation with guard bytes in front and behind that must be
intact afterwards (the idiom of tests/test_input_stage_classes_gpu.py).  Every reference is the numpy restatement
(tests/quant_embedding_ref.py), which imports nothing from the package:

* quantize: codes, scale and bias bit for bit (subtract-then-multiply cannot contract; the divisions are correctly rounded),
  pad bytes zero;
* gather, fp32 out: |out - ref64| <= 2^-23 (|code * scale| + |bias|) -- one rounding of the product, one of the sum, which
  covers the fused and the unfused form (the unfused fp32 restatement reaches 0.79 of it on the CPU);
* gather, 16-bit out: that plus half an ulp of the output type at |ref64|, computed exactly from ref64's exponent
  (quant_embedding_ref.half_ulp16: 2^-9 2^e for bf16, 2^-12 2^e and at least 2^-25 for fp16, |ref| = m 2^e, 0.5 <= m < 1)."""

import numpy as np
import pytest
import torch

import quant_embedding_probe as P
import quant_embedding_ref as Q
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
BF16, F16, F32 = 0, 1, 2
I32, I64 = 0, 1
DTYPES = {"float32": (torch.float32, F32, 4), "float16": (torch.float16, F16, 2), "bfloat16": (torch.bfloat16, BF16, 2)}
QUANT_DIMS = (1, 3, 4, 16, 50, 64, 192, 200, 256, 1000, 1024, 1040, 2048)
GATHER_DIMS = (1, 3, 16, 50, 192, 200, 256, 1040, 2048)


class Owned:
    """`nbytes` bytes behind GUARD bytes of a 0xFF-filled allocation, GUARD more behind"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 256 == 0
        self.ptr = self.raw.data_ptr() + GUARD

    def read(self, dtype=np.uint8, shape=None):
        a = self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype)
        return a if shape is None else a.reshape(shape)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xFF).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xFF).all())


def placed(t, mis=0):
    """a host tensor's bytes on the GPU, `mis` bytes off 256-byte alignment: (keep-alive, pointer)"""
    t = t.contiguous()
    raw = torch.zeros(t.numel() * t.element_size() + 256, dtype=torch.uint8, device=DEV)
    raw[mis:mis + t.numel() * t.element_size()] = t.view(torch.uint8).reshape(-1).to(DEV)
    assert raw.data_ptr() % 256 == 0
    return raw, raw.data_ptr() + mis


@pytest.fixture(scope="module")
def lib():
    from generative_recommenders_amd import _lib

    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def widen(bits, dtype_name):
    """the bytes of an output in `dtype_name` -> float64 values"""
    t = torch.from_numpy(bits.copy())
    return t.view(DTYPES[dtype_name][0]).double().numpy()


# ---------------------------------------------------------------------------------------------------------------- quantize
def _source(dim, rows, dtype_name, seed):
    """float32 rows (the special ones first) -> the tensor in `dtype_name` and its exact float32 values.  Zeros are made +0:
    1e-30 rounds to zeros of both signs in float16, and the sign of min(-0, +0) is nobody's to define"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, dim)) * rng.uniform(0.01, 10.0, (rows, 1)) + rng.uniform(-3.0, 3.0, (rows, 1))).astype(np.float32)
    special = Q.special_rows(dim, rng)
    x[:min(rows, 6)] = special[:min(rows, 6)]
    if dtype_name == "float16":
        x = np.clip(x, -6e4, 6e4)                        # 1e30 is not a float16: the row becomes a wide finite one
    t = torch.from_numpy(x).to(DTYPES[dtype_name][0])
    t = torch.where(t == 0, torch.zeros_like(t), t)
    return t, t.to(torch.float32).numpy()


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("dim", QUANT_DIMS)
def test_quantize_is_bit_equal_to_the_restatement(lib, dim, dtype_name):
    stride = Q.row_stride(dim)
    for rows, mis in ((1, 0), (5, 0), (67, 0), (67, 4), (1000, 0)):          # mis = 4: rows off 16 bytes, read element by element
        t, x = _source(dim, rows, dtype_name, 1000 * dim + rows)
        keep, src = placed(t, mis)
        dst = Owned(rows * stride)
        assert lib.hstu_quantize_rows_int8(src, dim, rows, dim, dst.ptr, stride, DTYPES[dtype_name][1], stream()) == 0, lib.hstu_last_error()
        torch.cuda.synchronize()
        assert dst.guards_intact(), (rows, mis)
        got = dst.read(np.uint8, (rows, stride))
        codes, scale, bias, pad = Q.unpack(got, dim)
        wc, ws, wb = Q.quantize(x)
        where = (dim, dtype_name, rows, mis)
        assert np.array_equal(codes, wc), where
        assert np.array_equal(scale.view(np.uint32), ws.view(np.uint32)), where
        assert np.array_equal(bias.view(np.uint32), wb.view(np.uint32)), where
        assert not pad.any(), where
        assert scale[0] == 0.0 and not codes[0].any()                          # the constant row


def test_quantize_wider_destination_rows_and_op(lib):
    """dst_row_stride above the format's stride: the first `stride` bytes of every row are written, the rest is the caller's;
    and the op (any source stride) equals the C ABI call"""
    from generative_recommenders_amd.ops.quant_embedding import quantize_rows_int8

    dim, rows = 50, 37
    stride, wide = Q.row_stride(dim), Q.row_stride(dim) + 32
    t, x = _source(dim, rows, "float32", 5)
    keep, src = placed(t)
    dst = Owned(rows * wide)
    assert lib.hstu_quantize_rows_int8(src, dim, rows, dim, dst.ptr, wide, F32, stream()) == 0
    torch.cuda.synchronize()
    got = dst.read(np.uint8, (rows, wide))
    want = Q.pack(*Q.quantize(x))
    assert dst.guards_intact() and np.array_equal(got[:, :stride], want) and (got[:, stride:] == 0xFF).all()
    big = torch.zeros(rows, dim + 7, device=DEV)
    big[:, 3:3 + dim] = t.to(DEV)
    assert np.array_equal(quantize_rows_int8(big[:, 3:3 + dim]).cpu().numpy(), want)          # a column slice as the source
    assert tuple(quantize_rows_int8(torch.zeros(0, dim, device=DEV)).shape) == (0, stride)


# ------------------------------------------------------------------------------------------------------------------ gather
def _table(dim, rows, seed, dtype_name="float32"):
    """a quantized table whose values the output type `dtype_name` can hold (the 1e30 row is no float16: clipped to a wide
    finite one)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, dim)) * rng.uniform(0.01, 10.0, (rows, 1)) + rng.uniform(-3.0, 3.0, (rows, 1))).astype(np.float32)
    x[:min(rows, 6)] = Q.special_rows(dim, rng)[:min(rows, 6)]
    if dtype_name == "float16":
        x = np.clip(x, -6e4, 6e4)
    codes, scale, bias = Q.quantize(x)
    return codes, scale, bias, Q.pack(codes, scale, bias)


def _check_gather(got64, codes, scale, bias, rows, dtype_name, what):
    """the derived gate on the rows `rows` of the table; returns the worst error over its bound"""
    c, s, b = codes[rows], scale[rows], bias[rows]
    ref = Q.dequant64(c, s, b)
    bound = Q.bound_fp32(c, s, b)
    if dtype_name != "float32":
        bound = bound + Q.half_ulp16(ref, dtype_name)
    err = np.abs(got64 - ref)
    ok = err <= bound
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{what}: worst error / bound = {worst:.4f}")
    assert ok.all(), (what, worst, int((~ok).sum()))
    return worst, ref


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("dim", GATHER_DIMS)
def test_gather_stays_inside_the_derived_bounds(lib, dim, dtype_name):
    table_rows = 77
    codes, scale, bias, q = _table(dim, table_rows, dim, dtype_name)
    keep, table = placed(torch.from_numpy(q))
    stride = q.shape[1]
    _, code, es = DTYPES[dtype_name]
    out_rs = -(-dim * es // 16) * 16 // es                                   # rows 16-byte aligned
    rng = np.random.default_rng(dim + 1)
    worst = 0.0
    for n in (0, 1, 63, 64, 65, 1000):
        ids = rng.integers(0, table_rows, n)
        if n >= 63:
            ids[:8] = (0, table_rows - 1, 5, 5, 5, 0, table_rows - 1, 0)    # the first and the last row, repeats
            ids[8:12] = (-1, -2**31, table_rows, 2**31 - 1)                   # outside the table: clamped
        rows = np.clip(ids, 0, table_rows - 1)
        for index_type, np_type in ((I32, np.int32), (I64, np.int64)):
            keep_i, idx = placed(torch.from_numpy(ids.astype(np_type))) if n else (None, None)
            out = Owned(max(n, 1) * out_rs * es)
            assert lib.hstu_gather_rows_int8(table, stride, table_rows, dim, idx, index_type, n, out.ptr, out_rs, code, stream()) == 0, \
                lib.hstu_last_error()
            torch.cuda.synchronize()
            assert out.guards_intact(), (n, index_type)
            raw = out.read(np.uint8, (max(n, 1), out_rs * es))
            if n == 0:
                assert (raw == 0xFF).all()
                continue
            assert (raw[:, dim * es:] == 0xFF).all(), "bytes between the rows were written"
            got = widen(np.ascontiguousarray(raw[:, :dim * es]), dtype_name)
            w, ref = _check_gather(got, codes, scale, bias, rows, dtype_name, f"gather D={dim} n={n} {dtype_name} idx{32 * (index_type + 1)}")
            worst = max(worst, w)
            if n == 1000 and index_type == I32:
                record_parity(f"int8 gather D={dim}", got, ref, dtype_name if dtype_name != "float32" else None, worst_over_bound=w)
    # idx == NULL: the identity
    out = Owned(table_rows * out_rs * es)
    assert lib.hstu_gather_rows_int8(table, stride, table_rows, dim, None, I32, table_rows, out.ptr, out_rs, code, stream()) == 0
    torch.cuda.synchronize()
    got = widen(np.ascontiguousarray(out.read(np.uint8, (table_rows, out_rs * es))[:, :dim * es]), dtype_name)
    _check_gather(got, codes, scale, bias, np.arange(table_rows), dtype_name, f"dequantize D={dim} {dtype_name}")
    assert out.guards_intact()
    if dtype_name == "float32":
        assert np.array_equal(got[0], Q.dequant64(codes[:1], scale[:1], bias[:1])[0])          # the constant row: exact
    assert worst <= 1.0


def test_gather_beyond_the_grid_cap_walks_several_steps_per_workgroup(lib):
    """D = 8, fp32 out: 2 lanes per row, 128 rows per chunk, 4 chunks per loop step.  n is chosen from the dispatch header so
    that the grid is capped and a workgroup takes more than one step (the strided walk), the last one ragged"""
    dim, table_rows = 8, 1000
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = P.sweep("gather4")[dim]
    per = s["rows"] * s["chunks"]
    cap = P.grid("gather4", 1, dim, cus)["cap"]
    n = (2 * cap + 1) * per + 37
    g = P.grid("gather4", n, dim, cus)
    assert g["grid"] == cap and g["steps_per_wg"] == 3 > 1 and g["steps"] % cap != 0
    codes, scale, bias, q = _table(dim, table_rows, 8)
    ids = np.random.default_rng(8).integers(0, table_rows, n).astype(np.int32)
    keep, table = placed(torch.from_numpy(q))
    keep_i, idx = placed(torch.from_numpy(ids))
    out = Owned(n * dim * 4)
    assert lib.hstu_gather_rows_int8(table, q.shape[1], table_rows, dim, idx, I32, n, out.ptr, dim, F32, stream()) == 0
    torch.cuda.synchronize()
    assert out.guards_intact()
    got = out.read(np.float32, (n, dim)).astype(np.float64)
    _check_gather(got, codes, scale, bias, ids, "float32", f"gather D=8 n={n} (cap {cap})")


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_gather_into_a_column_slice_and_twice_the_same_bits(dtype_name):
    from generative_recommenders_amd.ops.quant_embedding import dequantize_rows_int8, gather_rows_int8

    dtype, _, es = DTYPES[dtype_name]
    for dim in (50, 192):
        codes, scale, bias, q = _table(dim, 300, 3 * dim, dtype_name)
        qd = torch.from_numpy(q).to(DEV)
        ids = torch.from_numpy(np.random.default_rng(dim).integers(0, 300, 500)).to(DEV)
        first = 16 // es * 3
        wide = torch.full((500, first + dim + 16 // es * 2 + (-dim) % (16 // es)), 7.0, dtype=dtype, device=DEV)
        view = wide[:, first:first + dim]
        assert gather_rows_int8(qd, dim, ids, dtype, out=view) is view
        assert bool((wide[:, :first] == 7.0).all()) and bool((wide[:, first + dim:] == 7.0).all()), "a neighbouring column was written"
        plain = gather_rows_int8(qd, dim, ids, dtype)
        again = gather_rows_int8(qd, dim, ids.int(), dtype)
        bits = lambda t: t.contiguous().view(torch.int16 if es == 2 else torch.int32)
        assert torch.equal(bits(view), bits(plain)) and torch.equal(bits(plain), bits(again))          # two calls: equal bits
        _check_gather(plain.double().cpu().numpy(), codes, scale, bias, ids.cpu().numpy(), dtype_name, f"op gather D={dim} {dtype_name}")
        assert torch.equal(dequantize_rows_int8(qd, dim, dtype)[ids], plain)
        with pytest.raises(ValueError, match="16-byte aligned"):
            gather_rows_int8(qd, dim, ids, dtype, out=wide[:, 1:1 + dim])


def test_gpu_quantize_then_gather_round_trip_property():
    """the property of the host test, on the kernels: |dequant - x| <= (0.5 + 1e-4) scale + 1e-8"""
    from generative_recommenders_amd.ops.quant_embedding import dequantize_rows_int8, quantize_rows_int8

    rng = np.random.default_rng(11)
    x = np.concatenate([((rng.uniform(-1.0, 1.0, (8, 192)) + off) * s).astype(np.float32)
                        for s in 10.0 ** np.arange(-6, 7) for off in (0.0, 1.0, -2.0)])
    q = quantize_rows_int8(torch.from_numpy(x).to(DEV))
    _, scale, _, _ = Q.unpack(q.cpu().numpy(), 192)
    got = dequantize_rows_int8(q, 192).double().cpu().numpy()
    assert (np.abs(got - x.astype(np.float64)) <= Q.round_trip_bound(scale)).all()


def test_refusals_before_any_launch(lib):
    q = torch.zeros(4, 64, dtype=torch.uint8, device=DEV)
    out = torch.zeros(4, 32, device=DEV)
    idx = torch.zeros(4, dtype=torch.int32, device=DEV)
    src = torch.zeros(4, 32, device=DEV)
    s = stream()
    gather = lambda table=q.data_ptr(), trs=64, dim=32, it=I32, dt=F32: lib.hstu_gather_rows_int8(
        table, trs, 4, dim, idx.data_ptr(), it, 4, out.data_ptr(), 32, dt, s)
    quant = lambda dst=q.data_ptr(), drs=64, dim=32, dt=F32: lib.hstu_quantize_rows_int8(src.data_ptr(), 32, 4, dim, dst, drs, dt, s)
    assert gather() == 0 and quant() == 0
    for call in (gather, quant):
        assert call(dim=2049) == -2 and b"2048" in lib.hstu_last_error()
        assert call(dim=0) == -1
        assert call(q.data_ptr() + 8) == -1 and b"16-byte aligned" in lib.hstu_last_error()
        assert call(q.data_ptr(), 32) == -1 and b"row stride" in lib.hstu_last_error()        # short: 32 columns need 48 bytes
        assert call(q.data_ptr(), 56) == -1                                                    # long enough, no multiple of 16
        assert call(dt=7) == -1 and b"dtype" in lib.hstu_last_error()
    assert gather(it=5) == -1 and b"index_type" in lib.hstu_last_error()
    assert lib.hstu_gather_rows_int8(q.data_ptr(), 64, 4, 32, idx.data_ptr(), I32, 2**31, out.data_ptr(), 32, F32, s) == -1
    assert lib.hstu_gather_rows_int8(q.data_ptr(), 64, 4, 32, idx.data_ptr(), I32, 0, out.data_ptr(), 32, F32, s) == 0
    assert lib.hstu_quantize_rows_int8(src.data_ptr(), 32, 0, 32, q.data_ptr(), 64, F32, s) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ module
def test_quant_collection_on_gpu_equals_the_float_collection_over_the_dequantized_tables():
    from generative_recommenders_amd.modules.dlrm_hstu import (EmbeddingCollection, EmbeddingConfig, KeyedJaggedTensor,
                                                               QuantEmbeddingCollection, quantize_embeddings)
    from generative_recommenders_amd.ops.quant_embedding import dequantize_rows_int8

    tables = lambda dt: [EmbeddingConfig(num_embeddings=400, embedding_dim=192, name="item", feature_names=["uih_item", "cand_item"], data_type=dt),
                         EmbeddingConfig(num_embeddings=30, embedding_dim=20, name="user", feature_names=["user"], data_type=dt)]
    g = torch.Generator().manual_seed(3)
    lengths = torch.tensor([40, 0, 25, 1, 1, 1, 6, 3, 0])
    values = torch.cat([torch.randint(0, 400, (65,), generator=g), torch.randint(0, 30, (3,), generator=g),
                        torch.randint(0, 400, (9,), generator=g)])
    feats = KeyedJaggedTensor.from_lengths_sync(["uih_item", "user", "cand_item"], values.to(DEV), lengths.to(DEV))
    for dt in ("FP32", "FP16", "BF16"):
        torch.manual_seed(1)
        floats = EmbeddingCollection(tables(dt), device=torch.device(DEV))
        quant = quantize_embeddings(floats)
        assert isinstance(quant, QuantEmbeddingCollection) and quant.embeddings["item"].weight.is_cuda
        control = EmbeddingCollection(tables("FP32"), device=torch.device(DEV))
        with torch.no_grad():
            for name, dim in (("item", 192), ("user", 20)):
                control.embeddings[name].weight.copy_(dequantize_rows_int8(quant.embeddings[name].weight, dim))
            got, want = quant(feats), control(feats)
        assert list(got) == list(want) == ["uih_item", "user", "cand_item"]
        for k in got:
            assert torch.equal(got[k].lengths(), want[k].lengths()) and torch.equal(got[k].values(), want[k].values()), (dt, k)
        # the GPU tables carry the bits the CPU path makes of the same weights
        cpu = quantize_embeddings(floats.cpu())
        for name in ("item", "user"):
            assert torch.equal(cpu.embeddings[name].weight, quant.embeddings[name].weight.cpu()), (dt, name)


def test_quantized_inference_model_equals_the_model_over_the_dequantized_tables():
    import copy

    import dlrm_hstu_ref as R
    from generative_recommenders_amd.modules.dlrm_hstu import QuantEmbeddingCollection, quantize_embeddings
    from generative_recommenders_amd.ops.quant_embedding import dequantize_rows_int8

    inputs = R.load("model_small")
    m = R.build(True, inputs).to(DEV).eval()
    m.set_training_dtype(torch.float32)
    qm = quantize_embeddings(m)
    assert isinstance(qm._embedding_collection, QuantEmbeddingCollection)
    control = copy.deepcopy(m)
    with torch.no_grad():
        for name, table in qm._embedding_collection.embeddings.items():
            control._embedding_collection.embeddings[name].weight.copy_(dequantize_rows_int8(table.weight, table.embedding_dim))
    uih, cand = R.features(inputs, DEV)
    with torch.no_grad():
        outs = [model(uih_features=uih, candidates_features=cand) for model in (qm, control, m)]
    torch.cuda.synchronize()
    for i, name in ((0, "user_embeddings"), (1, "item_embeddings"), (3, "preds")):
        assert torch.equal(outs[0][i], outs[1][i]), name
        record_parity(f"int8 tables against float tables: {name}", outs[0][i].double().cpu().numpy(), outs[2][i].double().cpu().numpy())
