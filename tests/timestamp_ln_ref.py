"""numpy fp32 restatement of the time features of TimestampLayerNormPostprocessor (the arithmetic of the issue: torch's
fmod-based floor division, torch.remainder, the constant 3.14 -- no code under test is involved), the loader of the
fixtures under tests/golden/timestamp_ln/ and the helpers the CPU and GPU tests share."""

import glob
import os

import numpy as np
import torch

from conftest import GOLDEN
from multitask_ref import gate_multiplier, rel_fro  # noqa: F401  (the gate of every fused row pass)

FIXTURES = os.path.join(GOLDEN, "timestamp_ln")
COMBINER_W = "_time_feature_combiner.weight"
PARAMS = ("_layer_norm.weight", "_layer_norm.bias", COMBINER_W, "_time_feature_combiner.bias")
BUFFERS = ("_period_units", "_units_per_period")
TORCH_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
F32 = np.float32


def floor_div_f32(a, b):
    """torch.div(a, b, rounding_mode="floor") on fp32 arrays (c10::div_floor_floating), every step rounded to fp32"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        mod = np.fmod(a, b).astype(F32)
        div = ((a - mod).astype(F32) / b).astype(F32)
        div = np.where((mod != 0) & ((b < 0) != (mod < 0)), (div - F32(1)).astype(F32), div)
        fl = np.floor(div).astype(F32)
        fl = np.where((div - fl).astype(F32) > F32(0.5), (fl + F32(1)).astype(F32), fl)
        zero = np.copysign(F32(0), (a / b).astype(F32))
        out = np.where(div != 0, fl, zero)
        return np.where(b == 0, (a / b).astype(F32), out).astype(F32)


def remainder_f32(a, b):
    """torch.remainder on fp32 arrays: the sign of the divisor"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    mod = np.fmod(a, b).astype(F32)
    return np.where((mod != 0) & ((b < 0) != (mod < 0)), (mod + b).astype(F32), mod).astype(F32)


def time_buckets_and_angles(timestamps, periods):
    """(units, angles), each (rows, F) fp32: units = floor(fp32(t) / period), angle = ((units mod upp) / upp * 2) * 3.14"""
    a = np.asarray(timestamps, dtype=np.int64).astype(F32)[:, None]      # int64 -> fp32, round to nearest
    periods = np.asarray(periods, dtype=np.int64)
    pu, upp = periods[:, 0].astype(F32)[None, :], periods[:, 1].astype(F32)[None, :]
    units = floor_div_f32(a, pu)
    angles = (((remainder_f32(units, upp) / upp).astype(F32) * F32(2)).astype(F32) * F32(3.14)).astype(F32)
    return units, angles


def time_features(timestamps, periods):
    """(rows, 2F): [cos, sin] per period, interleaved (numpy's fp32 cos / sin: equal to torch's up to libm noise)"""
    _, angles = time_buckets_and_angles(timestamps, periods)
    return np.stack([np.cos(angles), np.sin(angles)], axis=-1).reshape(angles.shape[0], -1).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _widen(a):
    """bf16 bit patterns (uint16) -> the float32 values they stand for"""
    return (a.astype(np.uint32) << 16).view(np.float32) if a.dtype == np.uint16 else a


def case_files():
    return sorted(glob.glob(os.path.join(FIXTURES, "case_*.npz")))


def case_id(path):
    return os.path.basename(path)[5:-4]


def load_case(path):
    z = np.load(path, allow_pickle=False)
    c = {k: _widen(z[k]) for k in z.files}
    c["name"] = case_id(path)
    c["tags"] = [str(t) for t in z["tags"]]
    c["periods"] = [(int(p), int(u)) for p, u in z["periods"]]
    c["eps"] = float(z["eps"])
    dim = c["x"].shape[1]
    if "factor_a" in c:      # W = A B in fp64 (exact), rounded to fp32 and then to bf16-representable values
        w = torch.from_numpy(c["factor_a"].astype(np.float64)) @ torch.from_numpy(c["factor_b"].astype(np.float64))
        c["sd:" + COMBINER_W] = w.float().to(torch.bfloat16).float().numpy()
    assert c["sd:" + COMBINER_W].shape == (dim, dim + 2 * len(c["periods"]))
    c["params"] = {k: c["sd:" + k] for k in PARAMS}
    return c


def result_names():
    return ("out", "g:x", "gp:_layer_norm.weight", "gp:_layer_norm.bias", f"gp:{COMBINER_W}@rows", f"gp:{COMBINER_W}@time",
            "gp:_time_feature_combiner.bias")


def results_of(c, out, x, params):
    """the fixture's result names from an output, the input (with .grad) and the module's named parameters (with .grad)"""
    dim = c["x"].shape[1]
    rows = torch.from_numpy(c["w_rows"]).to(out.device)
    res = {"out": out, "g:x": x.grad}
    for k, p in params.items():
        if k == COMBINER_W:
            res[f"gp:{k}@rows"], res[f"gp:{k}@time"] = p.grad[rows], p.grad[:, dim:]
        else:
            res["gp:" + k] = p.grad
    return {k: v.detach().double().cpu().numpy() for k, v in res.items()}


def check_gate(c, tag, got, what, report=print):
    """e_hip <= m * e_ref for every result, both errors relative Frobenius against the fp64 truth; prints the ratios"""
    dtype_name = "float32" if tag == "f32" else "bfloat16"
    failures = []
    for k in result_names():
        truth, ref = c["f64:" + k], c[f"{tag}:{k}"]
        e_hip, e_ref = rel_fro(got[k], truth), rel_fro(ref, truth)
        m = gate_multiplier(dtype_name, truth.size)
        report(f"{what} {c['name']} {tag} {k}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {e_hip / max(e_ref, 1e-300):.3f} (gate {m})")
        if not (got[k].shape == truth.shape and np.isfinite(got[k]).all() and e_hip <= m * e_ref):
            failures.append((k, e_hip, e_ref, m))
    assert not failures, failures
