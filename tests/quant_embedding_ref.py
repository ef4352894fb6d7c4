"""numpy restatement of the int8 row-wise quantized embedding format (include/hstu_hip.h), one fp32 operation per line, plus
the fp64 evaluation of ``code * scale + bias`` and the bounds the tests gate with.  Imports nothing from the package.

    meta = round_up(D, 4);  stride = round_up(meta + 8, 16)
    [0, D) codes | [meta, meta + 4) fp32 scale | [meta + 4, meta + 8) fp32 bias | zeros elsewhere"""

import numpy as np

F32 = np.float32
MAX_DIM = 2048


def meta_offset(dim):
    return (dim + 3) // 4 * 4


def row_stride(dim):
    return (meta_offset(dim) + 8 + 15) // 16 * 16


def quantize(x):
    """x (rows, D) float32 (16-bit sources: widened exactly by the caller) -> codes uint8 (rows, D), scale, bias float32 (rows)"""
    x = np.ascontiguousarray(x, dtype=F32)
    assert x.ndim == 2 and x.shape[1] >= 1
    with np.errstate(over="ignore", invalid="ignore"):
        mn = x.min(axis=1)
        mx = x.max(axis=1)
        rng = (mx - mn).astype(F32)
        scale = (rng / F32(255.0)).astype(F32)
        inv = (F32(255.0) / (rng + F32(1e-8)).astype(F32)).astype(F32)
        t = (x - mn[:, None]).astype(F32)                    # subtract ...
        t = (t * inv[:, None]).astype(F32)                   # ... then multiply, each rounded to fp32
        codes = np.clip(np.rint(t), 0.0, 255.0).astype(np.uint8)      # rint: ties to even
    return codes, scale, mn.astype(F32)


def pack(codes, scale, bias):
    """-> uint8 (rows, stride), every byte outside codes / scale / bias zero"""
    rows, dim = codes.shape
    meta = meta_offset(dim)
    q = np.zeros((rows, row_stride(dim)), dtype=np.uint8)
    q[:, :dim] = codes
    q[:, meta:meta + 4] = np.ascontiguousarray(scale, dtype="<f4").view(np.uint8).reshape(rows, 4)
    q[:, meta + 4:meta + 8] = np.ascontiguousarray(bias, dtype="<f4").view(np.uint8).reshape(rows, 4)
    return q


def unpack(q, dim):
    """uint8 (rows, >= stride) -> codes, scale, bias, pad (the bytes of the first `stride` that are none of the three)"""
    q = np.ascontiguousarray(q)
    meta, stride = meta_offset(dim), row_stride(dim)
    codes = q[:, :dim].copy()
    scale = np.ascontiguousarray(q[:, meta:meta + 4]).view("<f4").reshape(-1).astype(F32)
    bias = np.ascontiguousarray(q[:, meta + 4:meta + 8]).view("<f4").reshape(-1).astype(F32)
    pad = np.concatenate([q[:, dim:meta], q[:, meta + 8:stride]], axis=1)
    return codes, scale, bias, pad


def dequant32(codes, scale, bias):
    """the unfused fp32 form: fl(fl(code * scale) + bias)"""
    p = (codes.astype(F32) * scale[:, None].astype(F32)).astype(F32)
    return (p + bias[:, None].astype(F32)).astype(F32)


def dequant64(codes, scale, bias):
    return codes.astype(np.float64) * scale.astype(np.float64)[:, None] + bias.astype(np.float64)[:, None]


def bound_fp32(codes, scale, bias):
    """2^-23 (|code * scale| + |bias|): one rounding of the product, one of the sum (|sum| <= |product| + |bias|); a fused
    multiply-add makes one rounding of the sum alone, which the same bound covers"""
    return 2.0**-23 * (np.abs(codes.astype(np.float64) * scale.astype(np.float64)[:, None]) + np.abs(bias.astype(np.float64))[:, None])


def half_ulp16(ref64, dtype_name):
    """half an ulp of the 16-bit output type at |ref|, exactly: with |ref| = m 2^e, 0.5 <= m < 1 (frexp), the spacing of a type
    of p significant bits there is 2^(e - p), half of it 2^(e - p - 1): 2^-9 2^e for bfloat16 (p = 8), 2^-12 2^e and at
    least 2^-25 (half the subnormal spacing) for float16 (p = 11).  Between 2^-9 |ref| and 2^-8 |ref| for bfloat16, 2^-12 |ref|
    and 2^-11 |ref| for float16: 2^-9 |ref| / 2^-12 |ref| themselves hold only at the top of a binade, and the nearest float16
    of 0.37 (0.37011719, 1.17e-4 away) is already outside 2^-12 * 0.37 = 9.0e-5"""
    _, e = np.frexp(np.abs(ref64))
    if dtype_name == "bfloat16":
        return np.where(ref64 == 0, 0.0, np.ldexp(2.0**-9, e))
    assert dtype_name == "float16"
    return np.maximum(np.where(ref64 == 0, 0.0, np.ldexp(2.0**-12, e)), 2.0**-25)


def round_trip_bound(scale):
    """|dequant - x| <= (0.5 + 1e-4) scale + 1e-8: half a code step, four fp32 roundings on a value of at most 255 and the
    epsilon in inv"""
    return (0.5 + 1e-4) * scale.astype(np.float64)[:, None] + 1e-8


def special_rows(dim, rng):
    """constant, one outlier, all negative, sign-crossing, magnitudes 1e-30 and 1e30 -> float32 (6, dim)"""
    u = rng.uniform(-1.0, 1.0, size=(6, dim)).astype(F32)
    rows = np.empty((6, dim), dtype=F32)
    rows[0] = F32(0.37)
    rows[1] = u[1] * F32(0.01)
    rows[1, dim // 2] = F32(100.0)
    rows[2] = -np.abs(u[2]) - F32(3.0)
    rows[3] = u[3] * F32(5.0)
    rows[4] = u[4] * F32(1e-30)
    rows[5] = u[5] * F32(1e30)
    return rows
