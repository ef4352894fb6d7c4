"""numpy restatement, on integers, of csrc/stochastic_round.h -- the counter-based random bits and the stochastic rounding of
fp32 to fp16 / bf16 -- and the 16-bit grid neighbours of fp64 values that the tests of the 16-bit embedding tables bound
their results with.  Nothing here imports the package: the header and the kernels are compared AGAINST this file."""

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & M32


def _rotl(x, k):
    return ((x << np.uint64(k)) | (x >> np.uint64(32 - k))) & M32


def sr_hash(seed, row, pair):
    """the 32 random bits of columns 2 * pair and 2 * pair + 1 of table row `row` (arrays broadcast); uint32"""
    seed = int(seed) & ((1 << 64) - 1)
    s0, s1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    row, pair = _u32(row), _u32(pair)
    k = (s1 + row * np.uint64(0x9E3779B9)) & M32
    h = pair ^ (s0 ^ _rotl(k, 16))
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h = (h + (s1 ^ _rotl(s0, 13))) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def sr_bits(seed, row, col):
    """the 16 random bits of column `col` of table row `row`; uint32 in [0, 65536)"""
    col = _u32(col)
    h = sr_hash(seed, row, col >> np.uint64(1)).astype(np.uint64)
    return np.where(col & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF)).astype(np.uint32)


def sr_bf16(b, r):
    """fp32 bit patterns b (uint32), 16 random bits r -> bf16 bit patterns (uint16)"""
    b, r = _u32(b), _u32(r)
    a = b & np.uint64(0x7FFFFFFF)
    o = ((b + r) >> np.uint64(16)) & np.uint64(0xFFFF)
    o = np.where((o & np.uint64(0x7FFF)) >= np.uint64(0x7F80), (o & np.uint64(0x8000)) | np.uint64(0x7F7F), o)
    special = np.where(a > np.uint64(0x7F800000), (b >> np.uint64(16)) | np.uint64(0x0040), b >> np.uint64(16))
    return np.where(a >= np.uint64(0x7F800000), special, o).astype(np.uint16)


def sr_f16(b, r):
    """fp32 bit patterns b (uint32), 16 random bits r -> fp16 bit patterns (uint16)"""
    b, r = _u32(b), _u32(r)
    s = (b >> np.uint64(16)) & np.uint64(0x8000)
    a = b & np.uint64(0x7FFFFFFF)
    special = np.where(a > np.uint64(0x7F800000), np.uint64(0x7E00), np.uint64(0x7C00))
    # |x| >= 2^-14: 13 random bits added below the fp16 mantissa, truncated, rebiased (127 - 15 = 112 = 0x1c000 >> 10), clamped
    t = (a + (r & np.uint64(0x1FFF))) >> np.uint64(13)
    normal = np.minimum(np.maximum(t, np.uint64(0x1C000)) - np.uint64(0x1C000), np.uint64(0x7BFF))
    # below: |x| = sig 2^(e - 150); t = |x| 2^24 = sig / 2^sh, sh = 126 - e; up iff r 2^sh < (sig mod 2^sh) 2^16
    e = a >> np.uint64(23)
    sig = np.where(e > 0, (a & np.uint64(0x7FFFFF)) | np.uint64(0x800000), a)
    e = np.maximum(e, np.uint64(1))
    sh = np.uint64(126) - np.minimum(e, np.uint64(126))                       # (lanes of the normal branch: any value)
    far = sh >= np.uint64(40)
    shc = np.where(far, np.uint64(0), sh)
    i = sig >> shc
    frac = sig & ((np.uint64(1) << shc) - np.uint64(1))
    up = (r << shc) < (frac << np.uint64(16))
    sub = np.where(far, ((r == 0) & (sig != 0)).astype(np.uint64), i + up.astype(np.uint64))
    mag = np.where(a >= np.uint64(0x38800000), normal, sub)
    return np.where(a >= np.uint64(0x7F800000), s | special, s | mag).astype(np.uint16)


def stochastic_round(x, dtype, seed, row_ids=None):
    """x (n, dim) fp32 -> the (n, dim) uint16 bit patterns of its stochastic rounding to dtype ("f16" / "bf16") with the bits of
    (seed, row_ids[i] or i, column)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, dim = x.shape
    rows = np.arange(n) if row_ids is None else np.asarray(row_ids)
    r = sr_bits(seed, rows.reshape(n, 1), np.arange(dim).reshape(1, dim))
    return (sr_f16 if dtype == "f16" else sr_bf16)(x.view(np.uint32), r)


# ---- the 16-bit grids as fp64 values
def widen16(bits, dtype):
    """uint16 bit patterns -> fp64 values"""
    bits = np.asarray(bits, dtype=np.uint16)
    if dtype == "f16":
        return bits.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):               # a signalling NaN is quieted by the widening
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def _ulp16(ax, dtype):
    """the grid spacing at magnitude ax (fp64, finite): 2^(floor(log2 ax) - mantissa bits), at least the subnormal spacing"""
    mant, emin = (10, -14) if dtype == "f16" else (7, -126)
    e = np.frexp(np.maximum(ax, 2.0 ** emin))[1] - 1          # exact: ax = m 2^(e + 1) with m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e, emin) - mant)


def down16(x, dtype):
    """the largest value of the 16-bit grid <= x (fp64 in, fp64 out; the grid is unbounded above its largest finite value:
    values beyond it are the caller's to clamp)"""
    x = np.asarray(x, dtype=np.float64)
    u = _ulp16(np.abs(x), dtype)
    return np.floor(x / u) * u                    # exact: u is a power of two, |x / u| < 2^53


def up16(x, dtype):
    """the smallest value of the 16-bit grid >= x"""
    return -down16(-np.asarray(x, dtype=np.float64), dtype)


MAX16 = {"f16": 65504.0, "bf16": float(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0])}


def special_values():
    """fp32 bit patterns (uint32) that reach every branch of the rule, each with both signs: zeros, fp32 subnormals, the
    fp16-subnormal range on and between grid points and at the width where the integer comparison changes form (2^-40),
    the smallest fp16 normal and its lower neighbourhood, values on and between grid points of both types, the largest
    finite values of both types and beyond them (the clamp), infinities, and quiet / signalling NaNs (one whose upper 16
    bits alone would read as an infinity)"""
    f = np.array([0.0, 2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 0.5 * 2.0 ** -24, 1.25 * 2.0 ** -24, 1022.875 * 2.0 ** -24,
                  1023.9375 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 * (1 + 2.0 ** -11), 2.0 ** -126, 2.0 ** -40, 2.0 ** -41, 1.5 * 2.0 ** -41,
                  2.0 ** -39, 2.0 ** -25, 1.0, 1 + 2.0 ** -10, 1 + 2.0 ** -7, 1 + 2.0 ** -11, 1 + 2.0 ** -13, 1 + 2.0 ** -23, 1 + 2.0 ** -8,
                  1 + 2.0 ** -16, 1 - 2.0 ** -24, 0.1, 3.14159274, 1000.123, 65504.0, 65505.0, 65519.99, 65520.0, 1e5, 1e30],
                 dtype=np.float32).view(np.uint32)
    b = np.array([0x00000001, 0x007FFFFF, 0x7F7F0000, 0x7F7F0001, 0x7F7FFFFF, 0x7F7E8000, 0x7F800000, 0x7FC00000, 0x7F800001,
                  0x7F80FFFF, 0x7FFFFFFF], dtype=np.uint32)
    pos = np.concatenate([f, b])
    return np.concatenate([pos, pos | np.uint32(0x80000000)])
