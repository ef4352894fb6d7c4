"""Host tests of the int8 row-wise quantized embedding tables: the dispatch header compiled alone and swept over every row
width, the CPU path of ops/quant_embedding.py bit for bit against the numpy restatement (tests/quant_embedding_ref.py), the
round-trip property, the fbgemm layout converters and QuantEmbeddingCollection / quantize_embeddings on the CPU.  No GPU."""

import numpy as np
import pytest
import torch

import quant_embedding_probe as P
import quant_embedding_ref as Q

TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
DIMS = (1, 3, 4, 16, 50, 64, 192, 200, 256, 1000, 1024, 1040, 2048)


# ------------------------------------------------------------------------------------------------------ dispatch header
MAX_LANES = {"quantize": 64, "gather4": 256, "gather2": 256}        # a quantized row stays inside one wave (its min / max exchange)
PIECE = {"quantize": 16, "gather4": 4, "gather2": 8}                # codes per lane and pass = what one 16-byte store holds


@pytest.mark.parametrize("kind", P.KINDS)
def test_every_code_byte_has_exactly_one_lane_and_pass_and_no_load_leaves_the_row(kind):
    c = P.consts()
    assert c["threads"] == 256 and c["wave"] == 64 and c["quantize_piece"] == 16 and c["max_dim"] == Q.MAX_DIM == 2048
    sweep = P.sweep(kind)
    assert sorted(sweep) == list(range(1, 2049))
    for d, g in sweep.items():
        assert g["ok"] == 1
        lanes, passes, piece = g["lanes"], g["passes"], g["piece"]
        assert piece == PIECE[kind]
        assert 1 <= lanes <= MAX_LANES[kind] and lanes & (lanes - 1) == 0, d        # a power of two
        assert g["rows"] * lanes == c["threads"], d
        assert 1 <= passes <= c["max_passes"], d
        assert passes == 1 or lanes == MAX_LANES[kind], d                          # a second pass only once the lanes are used up
        assert g["chunks"] == (1 if kind == "quantize" else c["gather_chunks"])
        cover = np.zeros(g["stride"], dtype=np.int32)
        for off_of_lane in g["offsets"]:
            for off in off_of_lane:
                if off < 0:
                    continue
                assert off % piece == 0 and off + piece <= g["stride"], (d, off)   # an aligned load that stays inside the row
                cover[off:off + piece] += 1
        assert (cover[:d] == 1).all(), d                                           # every code byte: one lane, one pass
        assert cover.max() == 1, d                                                 # and no piece twice
        assert g["pieces"] == -(-d // piece) and g["row_pieces"] * 16 == g["stride"], d
        assert g["meta"] >= d and g["meta"] + 8 <= g["stride"], d                  # scale and bias lie behind the codes, inside the row
        if kind == "quantize":
            assert g["row_pieces"] - g["pieces"] in (0, 1), d                      # the kernel writes at most one piece behind the codes


def test_meta_offset_and_stride_equal_the_python_and_the_library():
    from generative_recommenders_amd import _lib
    from generative_recommenders_amd.ops.quant_embedding import int8_row_stride

    lib = _lib.lib()
    for d, g in P.sweep("quantize").items():
        assert g["meta"] == Q.meta_offset(d) == (d + 3) // 4 * 4
        assert g["stride"] == Q.row_stride(d) == int8_row_stride(d) == lib.hstu_int8_row_stride(d)
        assert g["stride"] % 16 == 0 and g["stride"] - (g["meta"] + 8) < 16
    assert lib.hstu_int8_row_stride(0) == -1 and lib.hstu_int8_row_stride(2049) == -2
    for bad in (0, -3, 2049):
        with pytest.raises(ValueError, match="1 <= D <= 2048"):
            int8_row_stride(bad)


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("cus", [1, 8, 256, 304])
def test_the_grid_covers_n_rows_around_a_workgroup_and_around_the_cap(cus, kind):
    sweep = P.sweep(kind)
    for d in (1, 8, 16, 17, 192, 256, 1000, 2048):
        per = sweep[d]["rows"] * sweep[d]["chunks"]          # rows of one loop step of a workgroup
        cap = P.grid(kind, 1, d, cus)["cap"]
        assert cap == 8 * cus
        for n in (1, per - 1, per, per + 1, (cap - 1) * per, cap * per - 1, cap * per, cap * per + 1, (cap + 1) * per, 2**31 - 1):
            if n < 1:
                continue
            g = P.grid(kind, n, d, cus)
            assert g["steps"] == -(-n // per)                # workgroup b walks steps b, b + grid, ..: together rows 0 .. steps * per
            assert g["grid"] == min(g["steps"], cap) >= 1
            assert g["steps_per_wg"] * g["grid"] >= g["steps"] > (g["steps_per_wg"] - 1) * g["grid"]
    assert P.grid(kind, 0, 16, cus)["grid"] == 1



# ------------------------------------------------------------------------------------- the CPU path against the restatement
def _rows(dim, rows, seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([Q.special_rows(dim, rng), (rng.standard_normal((rows, dim)) * rng.uniform(0.01, 10.0, (rows, 1))
                                                    + rng.uniform(-3.0, 3.0, (rows, 1))).astype(np.float32)])
    return x


def _as_dtype(x, name):
    """float32 rows -> (the torch tensor in `name`, its values widened back to float32).  Zeros are made +0: the 1e-30 row
    rounds to zeros of both signs in float16, and the sign of min(-0, +0) is nobody's to define"""
    t = torch.from_numpy(x).to(TORCH[name])
    t = torch.where(t == 0, torch.zeros_like(t), t)
    return t, t.to(torch.float32).numpy()


@pytest.mark.parametrize("name", list(TORCH))
@pytest.mark.parametrize("dim", DIMS)
def test_cpu_quantize_is_bit_equal_to_the_restatement(dim, name):
    from generative_recommenders_amd.ops.quant_embedding import dequantize_rows_int8, gather_rows_int8, quantize_rows_int8

    t, x = _as_dtype(_rows(dim, 9, dim), name)
    if name == "float16":
        t, x = _as_dtype(np.clip(x, -6e4, 6e4), name)          # 1e30 is not a float16: the row becomes a wide finite one
    want = Q.pack(*Q.quantize(x))
    got = quantize_rows_int8(t)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (x.shape[0], Q.row_stride(dim))
    codes, scale, bias, pad = Q.unpack(got.numpy(), dim)
    wc, ws, wb = Q.quantize(x)
    assert np.array_equal(codes, wc)
    assert np.array_equal(scale.view(np.uint32), ws.view(np.uint32)) and np.array_equal(bias.view(np.uint32), wb.view(np.uint32))
    assert not pad.any()
    assert np.array_equal(got.numpy(), want)
    # a constant row: scale 0, codes 0, exact round trip
    assert scale[0] == 0.0 and not codes[0].any()
    deq = dequantize_rows_int8(got, dim)
    assert np.array_equal(deq.numpy()[0], x[0])
    # the CPU dequantization is the unfused fp32 form; a gather is that of the picked rows
    assert np.array_equal(deq.numpy().view(np.uint32), Q.dequant32(wc, ws, wb).view(np.uint32))
    idx = torch.tensor([3, 0, 3, x.shape[0] - 1], dtype=torch.int32)
    assert torch.equal(gather_rows_int8(got, dim, idx), deq[idx.long()])
    for out_name, out_dtype in TORCH.items():
        assert torch.equal(gather_rows_int8(got, dim, idx.long(), out_dtype), deq[idx.long()].to(out_dtype)), out_name


def test_round_trip_error_stays_under_half_a_step():
    """|dequant - x| <= (0.5 + 1e-4) scale + 1e-8 over rows scaled 1e-6 .. 1e6.  The offsets are a few row scales: the bound
    speaks of roundings on values of at most 255 code steps, and a row that sits far from zero compared to its own range
    adds the rounding of the final sum at the offset's magnitude, which no multiple of `scale` covers."""
    from generative_recommenders_amd.ops.quant_embedding import dequantize_rows_int8, quantize_rows_int8

    rng = np.random.default_rng(7)
    worst = 0.0
    for s in 10.0 ** np.arange(-6, 7):
        for off in (0.0, 1.0, -1.0, 2.0, -2.0):
            x = ((rng.uniform(-1.0, 1.0, (16, 192)) + off) * s).astype(np.float32)
            codes, scale, bias = Q.quantize(x)
            bound = Q.round_trip_bound(scale)
            ref = np.abs(Q.dequant32(codes, scale, bias).astype(np.float64) - x.astype(np.float64)) / bound
            got = dequantize_rows_int8(quantize_rows_int8(torch.from_numpy(x)), 192).numpy().astype(np.float64)
            worst = max(worst, float(ref.max()))
            assert ref.max() <= 1.0 and (np.abs(got - x.astype(np.float64)) <= bound).all(), (s, off, float(ref.max()))
    print(f"round trip: the restatement reaches {worst:.4f} of the bound")


def test_fbgemm_converters_round_trip_and_place_scale_and_bias():
    from generative_recommenders_amd.ops.quant_embedding import (from_fbgemm_fused_8bit_rowwise, quantize_rows_int8,
                                                                 to_fbgemm_fused_8bit_rowwise)

    for dim in (1, 3, 4, 50, 192, 200):
        x = _rows(dim, 5, 100 + dim)
        codes, scale, bias = Q.quantize(x)
        # the documented packed layout: D codes, fp32 scale, fp32 bias, no padding
        packed = np.concatenate([codes, scale.astype("<f4").view(np.uint8).reshape(-1, 4), bias.astype("<f4").view(np.uint8).reshape(-1, 4)], axis=1)
        assert packed.shape == (x.shape[0], dim + 8)
        q = from_fbgemm_fused_8bit_rowwise(torch.from_numpy(packed))
        assert np.array_equal(q.numpy(), Q.pack(codes, scale, bias))
        assert torch.equal(q, quantize_rows_int8(torch.from_numpy(x)))
        back = to_fbgemm_fused_8bit_rowwise(q, dim)
        assert np.array_equal(back.numpy(), packed)
        assert np.array_equal(back.numpy()[:, dim:dim + 4].copy().view("<f4").reshape(-1), scale)
        assert np.array_equal(back.numpy()[:, dim + 4:].copy().view("<f4").reshape(-1), bias)
    with pytest.raises(ValueError, match="uint8"):
        from_fbgemm_fused_8bit_rowwise(torch.zeros(3, 8, dtype=torch.uint8))


def test_op_refusals_name_the_limit():
    from generative_recommenders_amd.ops.quant_embedding import gather_rows_int8, quantize_rows_int8

    with pytest.raises(ValueError, match="1 <= D <= 2048"):
        quantize_rows_int8(torch.zeros(2, 2049))
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        quantize_rows_int8(torch.zeros(2, 4, dtype=torch.float64))
    q = quantize_rows_int8(torch.randn(4, 20))
    with pytest.raises(ValueError, match="at least int8_row_stride"):
        gather_rows_int8(q, 30, torch.tensor([0]))
    with pytest.raises(ValueError, match="uint8"):
        gather_rows_int8(q.float(), 20, torch.tensor([0]))
    with pytest.raises(ValueError, match="int32 or int64"):
        gather_rows_int8(q, 20, torch.tensor([0.0]))
    with pytest.raises(ValueError, match="out_dtype"):
        gather_rows_int8(q, 20, torch.tensor([0]), torch.float64)
    with pytest.raises(ValueError, match="out must be"):
        gather_rows_int8(q, 20, torch.tensor([0, 1]), out=torch.zeros(2, 21))
    assert tuple(gather_rows_int8(q, 20, torch.zeros(0, dtype=torch.int64)).shape) == (0, 20)


# ------------------------------------------------------------------------------------------------------------- the module
def _tables(data_type="FP32"):
    from generative_recommenders_amd.modules.dlrm_hstu import EmbeddingConfig

    return [EmbeddingConfig(num_embeddings=40, embedding_dim=24, name="item", feature_names=["uih_item", "cand_item"], data_type=data_type),
            EmbeddingConfig(num_embeddings=11, embedding_dim=5, name="user", feature_names=["user"], data_type=data_type)]


def _features():
    from generative_recommenders_amd.modules.dlrm_hstu import KeyedJaggedTensor

    lengths = torch.tensor([3, 0, 2, 1, 1, 1, 2, 1, 0, 4, 0, 1])        # 4 keys x 3 users; "other" has no table
    values = torch.tensor([5, 39, 0, 7, 7, 10, 0, 3, 12, 5, 39, 1, 2, 3, 4, 9])
    return KeyedJaggedTensor.from_lengths_sync(["uih_item", "user", "cand_item", "other"], values, lengths)


@pytest.mark.parametrize("data_type", ["FP32", "FP16", "BF16"])
def test_quant_collection_on_cpu_equals_the_float_collection_over_the_dequantized_tables(data_type):
    from generative_recommenders_amd.modules.dlrm_hstu import EmbeddingCollection, QuantEmbeddingCollection, quantize_embeddings
    from generative_recommenders_amd.ops.quant_embedding import dequantize_rows_int8, int8_row_stride

    torch.manual_seed(0)
    floats = EmbeddingCollection(_tables(data_type))
    quant = quantize_embeddings(floats)
    assert isinstance(quant, QuantEmbeddingCollection)
    sd = quant.state_dict()
    assert sorted(sd) == ["embeddings.item.weight", "embeddings.user.weight"]
    assert sd["embeddings.item.weight"].dtype == torch.uint8 and tuple(sd["embeddings.item.weight"].shape) == (40, int8_row_stride(24))
    assert tuple(sd["embeddings.user.weight"].shape) == (11, int8_row_stride(5))
    control = EmbeddingCollection(_tables("FP32"))
    with torch.no_grad():
        for name, dim in (("item", 24), ("user", 5)):
            control.embeddings[name].weight.copy_(dequantize_rows_int8(sd[f"embeddings.{name}.weight"], dim))
    feats = _features()
    got, want, orig = quant(feats), control(feats), floats(feats)
    assert list(got) == list(want) == list(orig) == ["uih_item", "user", "cand_item"]          # one table shared by two features
    for k in got:
        assert torch.equal(got[k].lengths(), want[k].lengths())
        assert got[k].values().dtype == torch.float32 and torch.equal(got[k].values(), want[k].values()), k
        assert float((got[k].values() - orig[k].values().detach().float()).abs().max()) < 0.02          # it IS the same table, coarsely
    half = QuantEmbeddingCollection.from_float(floats, torch.bfloat16)(feats)
    for k in got:
        assert torch.equal(half[k].values(), got[k].values().to(torch.bfloat16))
    # state_dict round trip into a freshly built collection
    fresh = QuantEmbeddingCollection(_tables())
    assert not fresh.embeddings["item"].weight.any()
    fresh.load_state_dict(sd)
    again = fresh(feats)
    for k in got:
        assert torch.equal(again[k].values(), got[k].values())


def test_quantize_embeddings_refusals_and_model_conversion():
    import dlrm_hstu_ref as R
    from generative_recommenders_amd.modules.dlrm_hstu import EmbeddingCollection, QuantEmbeddingCollection, quantize_embeddings

    with pytest.raises(RuntimeError, match="is_inference=True"):
        quantize_embeddings(R.build(is_inference=False).eval())
    with pytest.raises(RuntimeError, match="eval"):
        quantize_embeddings(R.build(is_inference=True).train())
    with pytest.raises(TypeError, match="EmbeddingCollection or a DlrmHSTU"):
        quantize_embeddings(torch.nn.Linear(2, 2))
    m = R.build(is_inference=True).eval()
    q = quantize_embeddings(m)
    assert q is not m and isinstance(m._embedding_collection, EmbeddingCollection)        # the original keeps its float tables
    assert isinstance(q._embedding_collection, QuantEmbeddingCollection) and q._is_inference and not q.training
    assert not any(k.startswith("_embedding_collection") for k, _ in q.named_parameters())
    assert sorted(k for k in q.state_dict() if k.startswith("_embedding_collection")) == [
        "_embedding_collection.embeddings.item_id.weight", "_embedding_collection.embeddings.user_id.weight"]
    for (k, a), (k2, b) in zip(sorted(m._hstu_transducer.state_dict().items()), sorted(q._hstu_transducer.state_dict().items())):
        assert k == k2 and torch.equal(a, b) and (a.numel() == 0 or a.data_ptr() != b.data_ptr())     # a copy, not a view
    with pytest.raises(RuntimeError, match="already"):
        quantize_embeddings(q)
    assert quantize_embeddings(m, inplace=True) is m and isinstance(m._embedding_collection, QuantEmbeddingCollection)


def test_int8_stays_refused_as_a_table_data_type():
    from generative_recommenders_amd.modules.dlrm_hstu import EmbeddingConfig, table_dtype

    with pytest.raises(ValueError, match="not supported"):
        EmbeddingConfig(num_embeddings=4, embedding_dim=8, name="t", data_type="INT8")
    with pytest.raises(ValueError, match="not supported"):
        table_dtype(torch.uint8)
