"""CPU tests of the 16-bit embedding tables: csrc/stochastic_round.h compiled alone by g++ against the numpy restatement of
embedding_lowp_ref.py, bit for bit; the properties of the rule (neighbours, fixed points, unbiasedness, independent
draws) on that restatement; ``EmbeddingConfig.data_type``, the declared-dtype checks, the state-dict keys and the
refusals of ``EmbeddingCollection``; the new entry points' argument checks.  No kernel is launched."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import embedding_lowp_ref as LR
from generative_recommenders_amd.modules.dlrm_hstu import (EmbeddingCollection, EmbeddingConfig, KeyedJaggedTensor,
                                                          apply_rowwise_adagrad_in_backward, table_dtype)
from generative_recommenders_amd.ops import embedding as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")
DTYPES = ("f16", "bf16")
RS = np.array([0, 1, 0x0FFF, 0x1000, 0x1FFF, 0x2000, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF], dtype=np.uint32)

PROGRAM = r"""
#include <stdio.h>
#include "stochastic_round.h"
int main() {
  char mode;
  unsigned long long seed;
  unsigned a, b, c;
  // "r <fp32 bits> <r>": the rule with given random bits;  "h <seed> <row> <col> <fp32 bits>": with the generator's
  while (scanf(" %c", &mode) == 1) {
    if (mode == 'r') {
      if (scanf("%u %u", &a, &b) != 2) return 1;
      printf("%u %u\n", (unsigned)hstu_sr_f16(a, b), (unsigned)hstu_sr_bf16(a, b));
    } else {
      if (scanf("%llu %u %u %u", &seed, &a, &b, &c) != 4) return 1;
      const unsigned r = hstu_sr_bits(seed, a, b);
      printf("%u %u %u %u\n", (unsigned)hstu_sr_hash(seed, a, b >> 1), r, (unsigned)hstu_sr_f16(c, r), (unsigned)hstu_sr_bf16(c, r));
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    """the header, compiled by g++ alone (so it is plain host C++), as a function of input lines -> rows of integers"""
    d = tmp_path_factory.mktemp("sr")
    src, exe = d / "sr.cpp", d / "sr"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.uint64)

    return run


def _random_fp32_bits(n, seed):
    """fp32 bit patterns: uniform bits (every exponent, NaNs among them), and values around the fp16 range's ends"""
    g = np.random.default_rng(seed)
    uniform = g.integers(0, 1 << 32, size=n // 2, dtype=np.uint64).astype(np.uint32)
    near = (g.standard_normal(n - n // 2) * np.exp2(g.integers(-30, 18, size=n - n // 2))).astype(np.float32).view(np.uint32)
    return np.concatenate([uniform, near])


def test_compiled_header_matches_the_numpy_rule_on_special_values(rule):
    sv = LR.special_values()
    b, r = np.repeat(sv, len(RS)), np.tile(RS, len(sv))
    got = rule([f"r {x} {y}" for x, y in zip(b, r)])
    assert got.shape == (len(b), 2)
    assert np.array_equal(got[:, 0], LR.sr_f16(b, r)) and np.array_equal(got[:, 1], LR.sr_bf16(b, r))


def test_compiled_header_matches_the_numpy_rule_and_generator_on_random_values(rule):
    n = 100_000
    b = _random_fp32_bits(n, 1)
    g = np.random.default_rng(2)
    rows = g.integers(0, 1 << 31, size=n, dtype=np.uint64)
    rows[:1000] = np.arange(1000)
    cols = g.integers(0, 2048, size=n, dtype=np.uint64)
    seeds = [0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1]
    seed_of = g.integers(0, len(seeds), size=n)
    got = rule([f"h {seeds[s]} {row} {col} {x}" for s, row, col, x in zip(seed_of, rows, cols, b)])
    assert got.shape == (n, 4)
    for k, seed in enumerate(seeds):
        m = seed_of == k
        h, r = LR.sr_hash(seed, rows[m], cols[m] >> np.uint64(1)), LR.sr_bits(seed, rows[m], cols[m])
        assert np.array_equal(got[m, 0], h) and np.array_equal(got[m, 1], r)
        assert np.array_equal(got[m, 2], LR.sr_f16(b[m], r)) and np.array_equal(got[m, 3], LR.sr_bf16(b[m], r))


def _rule(dtype):
    return LR.sr_f16 if dtype == "f16" else LR.sr_bf16


@pytest.mark.parametrize("dtype", DTYPES)
def test_result_is_one_of_the_two_neighbours(dtype):
    b = np.concatenate([_random_fp32_bits(100_000, 3), LR.special_values()])
    b = b[np.isfinite(b.view(np.float32))]
    x = b.view(np.float32).astype(np.float64)
    lo, hi = LR.down16(x, dtype), LR.up16(x, dtype)
    top = LR.MAX16[dtype]
    lo, hi = np.clip(lo, -top, top), np.clip(hi, -top, top)          # a finite input never becomes infinite
    r = np.random.default_rng(4).integers(0, 1 << 16, size=b.size, dtype=np.uint64)
    for rr in (r, np.zeros_like(r), np.full_like(r, 0xFFFF)):
        out = _rule(dtype)(b, rr)
        got = LR.widen16(out, dtype)
        assert np.isfinite(got).all()
        assert ((got == lo) | (got == hi)).all()
        assert np.array_equal(np.signbit(got), np.signbit(x))        # -0 stays -0, and a negative x that rounds to zero gives -0


@pytest.mark.parametrize("dtype", DTYPES)
def test_representable_values_and_specials_are_fixed_points_for_every_draw(dtype):
    bits16 = np.arange(1 << 16, dtype=np.uint16)
    wide = LR.widen16(bits16, dtype)
    keep = ~np.isnan(wide)                                           # every finite value, both zeros, both infinities
    b = wide[keep].astype(np.float32).view(np.uint32)
    for seed in (0, 1, 12345, (1 << 64) - 1):
        r = LR.sr_bits(seed, np.arange(b.size) // 64, np.arange(b.size) % 64)
        assert np.array_equal(_rule(dtype)(b, r), bits16[keep])
    for r in (0, 0x1FFF, 0xFFFF):
        assert np.array_equal(_rule(dtype)(b, np.full(b.size, r)), bits16[keep])
    nan = np.array([0x7FC00000, 0x7F800001, 0xFFC00000, 0x7F80FFFF], dtype=np.uint32)
    out = LR.widen16(_rule(dtype)(nan, np.full(4, 0xFFFF)), dtype)
    assert np.isnan(out).all()
    quiet = 0x0200 if dtype == "f16" else 0x0040
    assert (_rule(dtype)(nan, np.zeros(4)) & quiet).all()


SEED, K = 20260101, 4096
# (dtype, the lower neighbour, the grid spacing there): the normal range of both types, the fp16-subnormal range
SPOTS = [("f16", 1.0, 2.0 ** -10), ("f16", -3.0, 2.0 ** -9), ("bf16", 1.0, 2.0 ** -7), ("bf16", -3.0, 2.0 ** -6),
         ("f16", 5 * 2.0 ** -24, 2.0 ** -24), ("f16", -1000 * 2.0 ** -24, 2.0 ** -24)]


@pytest.mark.parametrize("dtype,base,ulp", SPOTS)
@pytest.mark.parametrize("f", [1 / 8, 1 / 2, 7 / 8])
def test_round_up_frequency_is_the_fractional_position(dtype, base, ulp, f):
    """K distinct (row, column) counters under one seed: the round-ups (away from zero) number K f within 5 sigma + 1"""
    x = np.float32(base + np.sign(base) * f * ulp)
    assert float(x) == base + np.sign(base) * f * ulp               # exactly representable in fp32
    rows, cols = np.divmod(np.arange(K), 64)
    out = LR.widen16(LR.stochastic_round(np.full((64, 64), x, dtype=np.float32), dtype, SEED), dtype)
    assert out.shape == (64, 64) and rows.max() == 63 and cols.max() == 63
    away = base + np.sign(base) * ulp
    assert ((out == base) | (out == away)).all()
    ups = int((out == away).sum())
    assert abs(ups - K * f) <= 5 * np.sqrt(K * f * (1 - f)) + 1, (ups, K * f)


def test_draws_differ_between_seeds_rows_and_columns():
    rows, cols = np.arange(64).reshape(64, 1), np.arange(64).reshape(1, 64)
    base = LR.sr_bits(SEED, rows, cols)
    assert len(np.unique(base)) > 0.9 * K                            # 4096 draws of 65536 values: ~ 125 collisions expected
    for other in (LR.sr_bits(SEED + 1, rows, cols), LR.sr_bits(SEED ^ (1 << 32), rows, cols), LR.sr_bits(SEED, rows + 64, cols),
                  LR.sr_bits(SEED, rows, cols + 64)):
        assert int((other == base).sum()) <= 8                       # independent 16-bit draws agree with probability 2^-16 each
    # consecutive steps of one run never share a seed, and the seed mix is the documented one
    seeds = [E.update_seed(7, s) for s in range(1000)]
    assert len(set(seeds)) == 1000 and all(0 <= s < 1 << 64 for s in seeds)
    z = (7 + 1 * 0x9E3779B97F4A7C15) % (1 << 64)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
    assert E.update_seed(7, 0) == z ^ (z >> 31)


# ------------------------------------------------------------------------------- EmbeddingConfig / EmbeddingCollection
class _DataType:                                                     # TorchRec's DataType, as far as it is touched
    def __init__(self, name, value):
        self.name, self.value = name, value


def test_data_type_is_parsed_and_unknown_types_are_refused():
    assert EmbeddingConfig(4, 8, "t").data_type == "FP32" and table_dtype("FP32") == torch.float32
    for given, want in (("FP16", torch.float16), ("bf16", torch.bfloat16), (torch.float16, torch.float16), (torch.float32, torch.float32),
                        (_DataType("FP16", "FP16"), torch.float16), (_DataType("BF16", "BF16"), torch.bfloat16),
                        (_DataType("x", "FP16"), torch.float16)):
        assert table_dtype(EmbeddingConfig(4, 8, "t", ["f"], data_type=given).data_type) == want
    for bad in ("INT8", _DataType("INT8", "INT8"), torch.int8, torch.float64, None, 16):
        with pytest.raises(ValueError, match="FP32 / FP16 / BF16"):
            EmbeddingConfig(4, 8, "t", ["f"], data_type=bad)


def _tables(data_type):
    return [EmbeddingConfig(10, 8, "item", ["a", "b"], data_type=data_type), EmbeddingConfig(6, 8, "user", ["c"])]


def _features():
    return KeyedJaggedTensor(["a", "b", "c"], torch.tensor([1, 2, 2, 2, 3, 5, 0]), torch.tensor([3, 2, 2]))


@pytest.mark.parametrize("data_type,dtype", [("FP16", torch.float16), ("BF16", torch.bfloat16)])
def test_collection_creates_16_bit_weights_from_the_fp32_initial_values(data_type, dtype):
    torch.manual_seed(5)
    plain = EmbeddingCollection(_tables("FP32"))
    torch.manual_seed(5)
    ec = EmbeddingCollection(_tables(data_type))
    assert ec.embeddings["item"].weight.dtype == dtype and ec.embeddings["user"].weight.dtype == torch.float32
    assert torch.equal(ec.embeddings["item"].weight, plain.embeddings["item"].weight.to(dtype))      # round to nearest
    assert torch.equal(ec.embeddings["user"].weight, plain.embeddings["user"].weight)
    assert ec._table_dtype == {"item": dtype, "user": torch.float32}
    assert sorted(ec.state_dict()) == ["embeddings.item.weight", "embeddings.user.weight"]
    out = ec(_features())                                            # the unfused path gathers 16-bit rows
    assert out["a"].values().dtype == dtype and torch.equal(out["a"].values(), ec.embeddings["item"].weight[[1, 2, 2]])

    class Duck:                                                      # no data_type attribute: fp32
        name, num_embeddings, embedding_dim, feature_names = "t", 4, 8, ["f"]

    assert EmbeddingCollection([Duck()]).embeddings["t"].weight.dtype == torch.float32


def test_weights_are_checked_against_their_declared_dtype():
    with pytest.raises(RuntimeError, match="float32"):               # the fp32 table of a mixed collection, cast away
        apply_rowwise_adagrad_in_backward(EmbeddingCollection(_tables("FP16")).to(torch.bfloat16), lr=0.1, tables=["user"])
    with pytest.raises(RuntimeError, match="must be float16"):       # a declared FP16 table cast to fp32
        apply_rowwise_adagrad_in_backward(EmbeddingCollection(_tables("FP16")).to(torch.float32), lr=0.1, tables=["item"])
    ec = EmbeddingCollection(_tables("FP16"))
    ec.apply_rowwise_adagrad_in_backward(lr=0.1, seed=3)
    assert ec._fused["item"].seed == 3 and E.RowWiseAdagradConfig(0.1).seed == 0
    ec.to(torch.float32)                                             # cast away afterwards: the first forward raises
    with pytest.raises(RuntimeError, match="must stay float16"):
        ec(_features())
    ec = EmbeddingCollection(_tables("BF16"))
    ec.apply_rowwise_adagrad_in_backward(lr=0.1)
    out = ec(_features())                                            # as declared: accepted
    assert out["a"].values().dtype == torch.bfloat16 and out["c"].values().dtype == torch.float32
    ec.to(torch.float16)
    with pytest.raises(RuntimeError, match="must stay bfloat16"):
        ec(_features())


def test_state_dict_keys_and_the_step_counter():
    ec = EmbeddingCollection(_tables("FP16"))
    keys = sorted(ec.state_dict())
    ec.apply_rowwise_adagrad_in_backward(lr=0.1)
    assert sorted(ec.state_dict()) == keys                           # both states are non-persistent buffers
    state = ec.fused_optimizer_state_dict()
    assert sorted(state) == ["item.momentum1", "item.rounding_step", "user.momentum1"]      # fp32 tables: no new key
    step = state["item.rounding_step"]
    assert step.dtype == torch.int64 and step.shape == () and int(step) == 0
    assert state["item.momentum1"].dtype == torch.float32
    other = EmbeddingCollection(_tables("FP16"))
    other.apply_rowwise_adagrad_in_backward(lr=0.1)
    saved = {k: v.clone() for k, v in state.items()}
    saved["item.rounding_step"] += 41
    saved["item.momentum1"] += 0.5
    other.load_fused_optimizer_state_dict(saved)
    got = other.fused_optimizer_state_dict()
    assert int(got["item.rounding_step"]) == 41 and torch.equal(got["item.momentum1"], saved["item.momentum1"])
    with pytest.raises(KeyError, match="rounding_step"):
        other.load_fused_optimizer_state_dict({k: v for k, v in saved.items() if not k.endswith("rounding_step")})
    assert sorted(E._fused_steps(other)) == ["item"]


def test_cpu_tensors_and_bad_arguments_are_refused():
    w, m1 = torch.zeros(4, 8, dtype=torch.float16), torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.rowwise_adagrad_update_(w, m1, torch.tensor([1]), torch.zeros(1, 8), 0.1, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.stochastic_round(torch.zeros(2, 8), torch.float16, 0)
    ec = EmbeddingCollection(_tables("FP16"))
    ec.apply_rowwise_adagrad_in_backward(lr=0.1)
    out = ec(_features())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sum(v.values().float().sum() for v in out.values()).backward()
    assert all(e.weight.grad is None for e in ec.embeddings.values())
    assert int(ec.fused_optimizer_state_dict()["item.rounding_step"]) == 0


def test_abi_version_and_the_new_entry_points_argument_checks():
    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    assert _lib.ABI_VERSION == 13 and lib.hstu_abi_version() == 13
    assert {"hstu_embedding_rowwise_adagrad_lowp", "hstu_stochastic_round"} <= set(_lib.SIGNATURES)
    buf = (C.c_char * 512)()
    a = (C.addressof(buf) + 255) & ~255
    F16, BF16, F32 = 1, 0, 2
    assert (_lib.HSTU_DTYPE_F16, _lib.HSTU_DTYPE_BF16, _lib.HSTU_DTYPE_F32) == (F16, BF16, F32)
    call = lambda n=0, dim=8, w=a, wdt=F16, dt=BF16: lib.hstu_embedding_rowwise_adagrad_lowp(a, a, n, dim, 4, w, wdt, a, 0.1, 1e-8, 7, a,
                                                                                          0, dt, None)
    assert call() == 0 and call(wdt=BF16, dt=F32, dim=2048) == 0     # n == 0: nothing to do; fp32 rows of 8 KiB are in the domain
    assert call(wdt=F32) == -1 and b"weight_dtype" in lib.hstu_last_error()
    assert call(w=None) == -1 and b"non-NULL" in lib.hstu_last_error()
    assert call(dim=12, dt=F32) == -1 and b"multiple of 8" in lib.hstu_last_error()
    assert call(dim=2056) == -2 and b"rows of" in lib.hstu_last_error()
    assert call(dim=2056, dt=F32) == -2 and b"rows of" in lib.hstu_last_error()
    assert call(dt=3) == -1 and b"dtype" in lib.hstu_last_error()
    assert call(n=4) == -1 and b"workspace too small" in lib.hstu_last_error()
    sr = lambda src=a, dst=a, n=0, dim=8, dt=F16: lib.hstu_stochastic_round(src, None, dst, n, dim, dt, 7, None)
    assert sr() == 0
    assert sr(dt=F32) == -1 and b"dst_dtype" in lib.hstu_last_error()
    assert sr(dim=0) == -1 and sr(n=-1) == -1
    assert sr(n=1, src=None) == -1 and b"NULL" in lib.hstu_last_error()
