"""The fast-addressing predicate of the folded / four-wave attention backward (csrc/attn_dma_addr.h) without a GPU: the header
is compiled alone with g++ and asked at the boundaries of its two limits -- a row stride of 2^24 bytes (the 24-bit multiply)
and a sequence span of 2^32 bytes (the 32-bit lane offset) -- for each of the four tensors on its own."""

import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "generative_recommenders_amd", "csrc")

_PROGRAM = r"""
#include "attn_dma_addr.h"

#include <cstdio>
int main() {
  long long q, k, v, d, n;
  while (scanf("%lld %lld %lld %lld %lld", &q, &k, &v, &d, &n) == 5) printf("%d\n", hstu::attn_bwd_dma_fast(q, k, v, d, n) ? 1 : 0);
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("attn_dma_addr")
    src, exe = d / "ask.cpp", d / "ask"
    src.write_text(_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(rows):
        text = "".join(" ".join(str(x) for x in r) + "\n" for r in rows)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == len(rows)
        return [bool(int(x)) for x in out]

    return run


def _expected(q, k, v, do, len_max):
    """restated from the kernels' own words: strides below 16 MiB, a sequence's rows within 4 GiB of its first"""
    return all(rs < 2 ** 24 and len_max * rs < 2 ** 32 for rs in (q, k, v, do))


COMPACT = 1024          # 4 heads x 128 x 2 bytes: the benchmark's rows
LEN = 224               # 32 x tmax at tmax = 7


def test_the_benchmark_layouts_are_fast(ask):
    rows = [(COMPACT,) * 4 + (LEN,),              # q, k, v, dO compact
            (3 * COMPACT,) * 3 + (COMPACT, LEN),  # q, k, v views of one fused (L, H, 3 d) buffer
            (256, 256, 256, 256, 32)]
    assert ask(rows) == [True, True, True]


@pytest.mark.parametrize("which", range(4), ids=["q", "k", "v", "dO"])
def test_stride_limit_for_each_tensor_alone(ask, which):
    """2^24 - 1 bytes passes, 2^24 does not; at len_max = 32 the span (2^29) is far from its own limit"""
    def row(stride):
        s = [COMPACT] * 4
        s[which] = stride
        return tuple(s) + (32,)
    rows = [row(2 ** 24 - 1), row(2 ** 24), row(2 ** 24 + 16), row(2 ** 40)]
    assert ask(rows) == [True, False, False, False]
    assert [_expected(*r) for r in rows] == [True, False, False, False]


@pytest.mark.parametrize("which", range(4), ids=["q", "k", "v", "dO"])
def test_span_limit_for_each_tensor_alone(ask, which):
    """len_max x stride = 2^32 - 1 passes (a stride below 2^24), 2^32 does not"""
    # 2^32 - 1 = 3 x 5 x 17 x 257 x 65537: len_max = 257, stride = 16711935 (< 2^24)
    assert 257 * 16711935 == 2 ** 32 - 1 and 16711935 < 2 ** 24
    def row(stride, n):
        s = [COMPACT] * 4
        s[which] = stride
        return tuple(s) + (n,)
    rows = [row(16711935, 257),          # 2^32 - 1
            row(2 ** 23, 512),           # 2^32 exactly, stride well below its limit
            row(2 ** 24 - 16, 257),      # just past 2^32 with a legal stride
            row(2 ** 23, 511)]           # 2^32 - 2^23
    want = [True, False, False, True]
    assert ask(rows) == want
    assert [_expected(*r) for r in rows] == want


def test_agrees_with_the_restatement_on_a_grid(ask):
    strides = [16, 256, COMPACT, 2 ** 20, 2 ** 24 - 16, 2 ** 24, 2 ** 25]
    lens = [32, 64, 224, 256, 4096, 2 ** 16]
    rows = [(a, b, COMPACT, COMPACT, n) for a in strides for b in strides for n in lens]
    rows += [(COMPACT, COMPACT, a, b, n) for a in strides for b in strides for n in lens]
    assert ask(rows) == [_expected(*r) for r in rows]
