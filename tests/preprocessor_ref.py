"""numpy restatement of the two input-preprocessor ops (action encode, combine), forward and backward, as per-user Python
loops over the formulas of include/hstu_hip.h -- no code under test is involved -- plus the loader of the fixtures under
tests/golden/preprocessor/.

Both forwards and the combine backward only MOVE values (or add two of them once), so the restatement works on whatever
numpy dtype it is given: tests hand it bf16 / fp16 bit patterns (uint16) and compare bit for bit.  The one add of the SUM
mode is the caller's (``summed``: content + action in the activation dtype, e.g. by torch on the CPU)."""

import glob
import os

import numpy as np

from conftest import GOLDEN

FIXTURES = os.path.join(GOLDEN, "preprocessor")
SUM, INTERLEAVE_ALL, INTERLEAVE_UIH = 0, 1, 2


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------ action encode
def effective_actions(actions, watchtimes, thresholds):
    a = np.asarray(actions, dtype=np.int64).copy()
    for thr, w in thresholds:
        a |= np.where(np.asarray(watchtimes, dtype=np.int64) >= int(thr), np.int64(w), np.int64(0))     # note ">="
    return a


def signed_zero(x):
    """0 * x: the zero that keeps the sign of x (the reference multiplies a boolean into the table), also on bit patterns"""
    x = np.asarray(x)
    if x.dtype.kind == "u":
        return x & x.dtype.type(1 << (8 * x.dtype.itemsize - 1))
    return x * x.dtype.type(0)


def action_encode(actions, watchtimes, uih_offsets, target_offsets, table, target_table, weights, thresholds):
    """table (T, Da) and target_table (T * Da) ALREADY in the output dtype (any numpy dtype, bit patterns included);
    returns (sum L, T * Da): per user the UIH rows, then the target rows"""
    table, target_table = np.asarray(table), np.asarray(target_table).reshape(-1)
    T, da = table.shape
    a = effective_actions(actions, watchtimes, thresholds)
    rows = []
    for b in range(len(uih_offsets) - 1):
        for r in range(int(uih_offsets[b]), int(uih_offsets[b + 1])):
            row = signed_zero(table).reshape(-1)
            for t in range(T):
                if (int(a[r]) & int(weights[t])) > 0:
                    row[t * da:(t + 1) * da] = table[t]
            rows.append(row)
        for _ in range(int(target_offsets[b + 1]) - int(target_offsets[b])):
            rows.append(target_table.copy())
    return np.stack(rows) if rows else np.zeros((0, T * da), dtype=table.dtype)


def action_encode_bwd(d_out, actions, watchtimes, uih_offsets, target_offsets, weights, thresholds, da):
    """fp64 sums of d_out: d_table (T, Da), d_target (T * Da), and per element the sum of |terms| and the number of terms
    (for the bound n * 2^-24 * sum |terms| of an fp32 sum in any order)"""
    d_out = np.asarray(d_out, dtype=np.float64)
    T = len(weights)
    a = effective_actions(actions, watchtimes, thresholds)
    d_table, abs_table, n_table = np.zeros((T, da)), np.zeros((T, da)), np.zeros((T, da))
    d_target, abs_target, n_target = np.zeros(T * da), np.zeros(T * da), 0
    row = 0
    for b in range(len(uih_offsets) - 1):
        for r in range(int(uih_offsets[b]), int(uih_offsets[b + 1])):
            for t in range(T):
                if (int(a[r]) & int(weights[t])) > 0:
                    g = d_out[row, t * da:(t + 1) * da]
                    d_table[t] += g
                    abs_table[t] += np.abs(g)
                    n_table[t] += 1
            row += 1
        for _ in range(int(target_offsets[b + 1]) - int(target_offsets[b])):
            d_target += d_out[row]
            abs_target += np.abs(d_out[row])
            n_target += 1
            row += 1
    assert row == d_out.shape[0]
    return dict(d_table=d_table, d_target=d_target, abs_table=abs_table, abs_target=abs_target, n_table=n_table,
                n_target=np.full(T * da, n_target, dtype=np.float64))


# ------------------------------------------------------------------------------------------------------ combine
def out_lengths(lengths, num_targets, C, mode):
    L, T = np.asarray(lengths, dtype=np.int64), np.asarray(num_targets, dtype=np.int64)
    return C + (L if mode == SUM else 2 * L if mode == INTERLEAVE_ALL else 2 * L - T)


def _source(p, L, T, mode):
    """output position p (behind the contextual rows) of a user -> (source row, takes the action row?)"""
    if mode == SUM:
        return p, False
    U = L - T if mode == INTERLEAVE_UIH else L
    if p < 2 * U:
        return p >> 1, bool(p & 1)
    return U + (p - 2 * U), False


def combine(content, action, contextual, timestamps, lengths, num_targets, mode, summed=None):
    """content / action (sum L, D), contextual (B, C, D) or None, timestamps (sum L); ``summed`` = content + action in the
    activation dtype (SUM with an action).  Returns (embeddings, timestamps int64, lengths)"""
    content = np.asarray(content)
    D = content.shape[1]
    C = 0 if contextual is None else contextual.shape[1]
    off = offsets_of(lengths)
    rows, ts = [], []
    for b in range(len(lengths)):
        L, T, o = int(lengths[b]), int(num_targets[b]), int(off[b])
        for j in range(C):
            rows.append(contextual[b, j])
            ts.append(0)
        n = int(out_lengths([L], [T], 0, mode)[0])
        for p in range(n):
            i, act = _source(p, L, T, mode)
            if mode == SUM:
                rows.append(content[o + i] if action is None else summed[o + i])
            else:
                rows.append(action[o + i] if act else content[o + i])
            ts.append(int(timestamps[o + i]))
    emb = np.stack(rows) if rows else np.zeros((0, D), dtype=content.dtype)
    return emb, np.asarray(ts, dtype=np.int64), out_lengths(lengths, num_targets, C, mode)


def combine_bwd(d_out, lengths, num_targets, C, mode, has_action):
    """the inverse gather: (d_content, d_action or None, d_contextual (B, C, D) or None), each row a copy of one row of d_out"""
    d_out = np.asarray(d_out)
    D = d_out.shape[1]
    B, total = len(lengths), int(np.sum(lengths))
    oo, off = offsets_of(out_lengths(lengths, num_targets, C, mode)), offsets_of(lengths)
    d_content = np.zeros((total, D), dtype=d_out.dtype)
    d_action = np.zeros((total, D), dtype=d_out.dtype) if has_action else None
    d_ctx = np.zeros((B, C, D), dtype=d_out.dtype) if C > 0 else None
    for b in range(B):
        L, T, o, g = int(lengths[b]), int(num_targets[b]), int(off[b]), int(oo[b])
        for j in range(C):
            d_ctx[b, j] = d_out[g + j]
        for p in range(int(oo[b + 1]) - g - C):
            i, act = _source(p, L, T, mode)
            if mode == SUM:
                d_content[o + i] = d_out[g + C + p]
                if has_action:
                    d_action[o + i] = d_out[g + C + p]
            elif act:
                d_action[o + i] = d_out[g + C + p]
            else:
                d_content[o + i] = d_out[g + C + p]
    return d_content, d_action, d_ctx


# ------------------------------------------------------------------------------------------------------ index maps
# The same formulas as whole-array index maps, for batches of 10^5 rows (tests/test_input_stage_classes_gpu.py);
# tests/test_preprocessor_host.py shows them equal to the per-row loops above.
def action_row_map(uih_offsets, target_offsets):
    """per output row: (the UIH row it encodes, or -1 for a target row)"""
    uo, to = np.asarray(uih_offsets, dtype=np.int64), np.asarray(target_offsets, dtype=np.int64)
    U, Tn = np.diff(uo), np.diff(to)
    b = np.repeat(np.arange(len(U)), U + Tn)
    i = np.arange(int((U + Tn).sum())) - (uo + to)[b]
    return np.where(i < U[b], uo[b] + i, -1)


def _action_bits(actions, watchtimes, weights, thresholds):
    """(rows, T) bool: the bit test of every UIH row against every combined weight"""
    a = effective_actions(actions, watchtimes, thresholds)
    return (a[:, None] & np.asarray([int(w) for w in weights], dtype=np.int64)[None, :]) > 0


def action_encode_mapped(actions, watchtimes, uih_offsets, target_offsets, table, target_table, weights, thresholds):
    table, target_table = np.asarray(table), np.asarray(target_table).reshape(-1)
    T, da = table.shape
    src = action_row_map(uih_offsets, target_offsets)
    out = np.empty((src.size, T * da), dtype=table.dtype)
    out[src < 0] = target_table
    s = src[src >= 0]
    on = np.repeat(_action_bits(actions, watchtimes, weights, thresholds)[s], da, axis=1)
    out[src >= 0] = np.where(on, table.reshape(-1)[None, :], signed_zero(table).reshape(-1)[None, :])
    return out


def action_encode_bwd_mapped(d_out, actions, watchtimes, uih_offsets, target_offsets, weights, thresholds, da):
    d_out = np.asarray(d_out, dtype=np.float64)
    T = len(weights)
    src = action_row_map(uih_offsets, target_offsets)
    assert src.size == d_out.shape[0]
    g = d_out[src >= 0].reshape(-1, T, da)
    on = _action_bits(actions, watchtimes, weights, thresholds)[src[src >= 0]].astype(np.float64)
    tg = d_out[src < 0]
    return dict(d_table=np.einsum("rt,rtd->td", on, g), abs_table=np.einsum("rt,rtd->td", on, np.abs(g)),
                n_table=np.repeat(on.sum(0)[:, None], da, axis=1), d_target=tg.sum(0), abs_target=np.abs(tg).sum(0),
                n_target=np.full(T * da, tg.shape[0], dtype=np.float64))


def combine_row_map(lengths, num_targets, C, mode):
    """per output row: (user, contextual index or -1, source row or -1, takes the action row?)"""
    L, T = np.asarray(lengths, dtype=np.int64), np.asarray(num_targets, dtype=np.int64)
    n = out_lengths(L, T, C, mode)
    b = np.repeat(np.arange(len(L)), n)
    j = np.arange(int(n.sum())) - offsets_of(n)[b]
    p = j - C
    if mode == SUM:
        i, act = p, np.zeros(p.shape, dtype=bool)
    else:
        U = (L - T if mode == INTERLEAVE_UIH else L)[b]
        i, act = np.where(p < 2 * U, p >> 1, p - U), (p < 2 * U) & ((p & 1) == 1)
    ctx = j < C
    return b, np.where(ctx, j, -1), np.where(ctx, -1, offsets_of(L)[b] + i), act & ~ctx


def combine_mapped(content, action, contextual, timestamps, lengths, num_targets, mode, summed=None):
    content = np.asarray(content)
    C = 0 if contextual is None else contextual.shape[1]
    b, j, src, act = combine_row_map(lengths, num_targets, C, mode)
    emb = np.empty((b.size, content.shape[1]), dtype=content.dtype)
    seq = j < 0
    if C:
        emb[~seq] = contextual[b[~seq], j[~seq]]
    first = content if (mode != SUM or action is None) else summed
    emb[seq] = first[src[seq]]
    if mode != SUM:
        emb[act] = action[src[act]]
    ts = np.where(seq, np.asarray(timestamps, dtype=np.int64)[np.maximum(src, 0)], 0) if b.size else np.zeros(0, dtype=np.int64)
    return emb, ts.astype(np.int64), out_lengths(lengths, num_targets, C, mode)


def combine_bwd_mapped(d_out, lengths, num_targets, C, mode, has_action):
    d_out = np.asarray(d_out)
    D, B, total = d_out.shape[1], len(lengths), int(np.sum(lengths))
    b, j, src, act = combine_row_map(lengths, num_targets, C, mode)
    seq = j < 0
    d_content = np.zeros((total, D), dtype=d_out.dtype)
    d_content[src[seq & ~act]] = d_out[seq & ~act]
    d_action = None
    if has_action:
        d_action = d_content.copy() if mode == SUM else np.zeros((total, D), dtype=d_out.dtype)
        if mode != SUM:
            d_action[src[act]] = d_out[act]
    d_ctx = None
    if C > 0:
        d_ctx = np.zeros((B, C, D), dtype=d_out.dtype)
        d_ctx[b[~seq], j[~seq]] = d_out[~seq]
    return d_content, d_action, d_ctx


def candidates(values, lengths, num_targets, interleave):
    """the last num_targets rows of every user (of the OUTPUT sequence), every second one when the targets are interleaved"""
    off = offsets_of(lengths)
    rows = []
    for b in range(len(lengths)):
        tail = values[int(off[b + 1]) - int(num_targets[b]):int(off[b + 1])]
        rows.extend(tail[::2] if interleave else tail)
    return np.stack(rows) if rows else np.zeros((0,) + tuple(values.shape[1:]), dtype=values.dtype)


# ------------------------------------------------------------------------------------------------------ fixtures
def widen(a):
    """bf16 bit patterns (uint16) -> the float32 values they stand for"""
    return (a.astype(np.uint32) << 16).view(np.float32) if a.dtype == np.uint16 else a


def fixture_files(prefix):
    return sorted(glob.glob(os.path.join(FIXTURES, prefix + "_*.npz")))


def load(path):
    z = np.load(path, allow_pickle=False)
    c = {k: z[k] for k in z.files}
    c["name"] = os.path.basename(path)[:-4]
    return c


def tags_of(case):
    return [t for t in ("f32", "bf16", "f64") if any(k.startswith(t + ":") for k in case)]


def mode_of(case):
    if case["kind"] == "contextual" or not int(case["enable_interleaving"]):
        return SUM
    return INTERLEAVE_UIH if int(case["is_inference"]) else INTERLEAVE_ALL
