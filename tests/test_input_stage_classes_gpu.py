"""Every class of the input-stage kernels (tests/input_stage_class_cases.py) on the GPU, through the C ABI.

The test owns every output and workspace: each lives alone in a byte allocation filled with 0xFF -- NaN as fp32, bf16 and
fp16, -1 as a timestamp: no correct result holds it -- with GUARD bytes in front and behind that must be intact afterwards.
A row that was skipped or an address out of place shows.  No reference involves the code under test:

* action encode forward, combine forward and backward: bit for bit against tests/preprocessor_ref.py (its index-map path,
  which tests/test_preprocessor_host.py shows equal to the per-row loops);
* action encode backward: against the fp64 sums under n * 2^-24 * sum |terms|; for the slab-count classes the workspace is
  read back -- exactly groups x 2 x width floats are written -- and the partials, added in numpy fp32 in the finish kernel's
  order, give the returned gradients bit for bit;
* the research forward: bit for bit against the op-by-op numpy float32 chain fl(fl(fl(x s) + pos) [scale]) m, rounded once
  more for 16-bit outputs; d_emb bit for bit against fl(h s); d_pos and d_rating against the fp64 sums under
  (B + 1) 2^-24 sum |h| and (n_r + 2) 2^-24 sum |h| s;
* every table gradient twice, the same bits both times."""

import ctypes as C

import numpy as np
import pytest
import torch

import input_stage_class_cases as K
import preprocessor_ref as R
from oracle.hstu_oracle import dropout_keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH = {K.BF16: torch.bfloat16, K.F16: torch.float16, K.F32: torch.float32}
NP_BITS = {2: np.uint16, 4: np.uint32}


# ------------------------------------------------------------------------------------------------ buffers the test owns
class Owned:
    """`nbytes` bytes at GUARD + mis from the start of a 0xFF-filled allocation, GUARD (and the slack to 16) behind"""

    def __init__(self, nbytes, mis=0):
        self.nbytes, self.lo = int(nbytes), K.GUARD + mis
        self.raw = torch.full((self.lo + self.nbytes + K.GUARD + 16,), 0xFF, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 256 == 0
        self.ptr = self.raw.data_ptr() + self.lo

    def read(self, dtype, shape=None):
        a = self.raw[self.lo:self.lo + self.nbytes].cpu().numpy().view(dtype)
        return a if shape is None else a.reshape(shape)

    def guards_intact(self):
        return bool((self.raw[:self.lo] == 0xFF).all()) and bool((self.raw[self.lo + self.nbytes:] == 0xFF).all())

    def refill(self):
        self.raw.fill_(0xFF)


def placed(t, mis=0):
    """an input tensor's bytes at `mis` bytes off 256-byte alignment: (keep-alive, pointer)"""
    t = t.contiguous()
    if t.numel() == 0:
        return t, None
    if not mis:
        d = t.to(DEV)
        assert d.data_ptr() % 256 == 0
        return d, d.data_ptr()
    raw = torch.zeros(t.numel() * t.element_size() + 256, dtype=torch.uint8, device=DEV)
    raw[mis:mis + t.numel() * t.element_size()] = t.view(torch.uint8).reshape(-1).to(DEV)
    return raw, raw.data_ptr() + mis


def bits(t):
    t = t.detach().contiguous().cpu()
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int32).numpy().view(np.uint32)


def lib_and_stream():
    from generative_recommenders_amd import _lib as L

    return L, L.lib(), L.current_stream_ptr(torch.device(DEV))


def dtype_code(L, name):
    return L.torch_dtype_code(TORCH[name])


def i64_array(values):
    values = [int(v) for v in values]
    return (C.c_int64 * max(len(values), 1))(*values)


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ preprocess_ops.hip
def _weights(c):
    w = K.wide_weights() if c["weights"] == "wide" else [1 << t for t in range(c["T"])]
    assert len(w) == c["T"]
    return w


def _action_inputs(c, lengths, targets):
    g = torch.Generator().manual_seed(1000 + c["seed"])
    weights, thresholds = _weights(c), [(int(t), int(w)) for t, w in c["thresholds"]]
    uih = lengths - targets
    n = int(uih.sum())
    hi = 2**63 - 1 if c["weights"] == "wide" else 2 * max(weights)
    actions = torch.randint(0, hi, (n,), generator=g)
    watch = torch.randint(0, 100, (n,), generator=g)
    if thresholds and n > 1:
        watch[0], watch[1] = thresholds[0][0], thresholds[0][0] - 1               # ">=": at the threshold and just below it
    table = torch.randn(c["T"], c["da"], generator=g)
    target = torch.randn(c["T"] * c["da"], generator=g)
    return weights, thresholds, uih, actions, watch, table, target, g


def _offsets_dev(a, idx):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(torch.int32 if idx == 32 else torch.int64).to(DEV)


def _run_action_fwd(c, lengths, targets, mis):
    L, lib, stream = lib_and_stream()
    weights, thresholds, uih, actions, watch, table, target, _ = _action_inputs(c, lengths, targets)
    uo, to = R.offsets_of(uih), R.offsets_of(targets)
    rows, width = int(lengths.sum()), c["T"] * c["da"]
    dt = TORCH[c["dtype"]]
    out = Owned(rows * width * dt.itemsize, mis.get("out", 0))
    keep = [placed(actions), placed(watch), placed(table, mis.get("table", 0)), placed(target, mis.get("target_table", 0)),
            _offsets_dev(uo, c["idx"]), _offsets_dev(to, c["idx"])]
    w, th, tw = i64_array(weights), i64_array([t for t, _ in thresholds]), i64_array([x for _, x in thresholds])
    L.check(lib.hstu_action_encode_fwd(keep[0][1], keep[1][1] if thresholds else None, keep[4].data_ptr(), keep[5].data_ptr(),
                                       keep[2][1], keep[3][1], w, c["T"], th, tw, len(thresholds), out.ptr, int(uih.sum()),
                                       int(targets.sum()), len(lengths), c["da"], dtype_code(L, c["dtype"]),
                                       L.HSTU_INDEX_I32 if c["idx"] == 32 else L.HSTU_INDEX_I64, stream))
    torch.cuda.synchronize()
    got = out.read(NP_BITS[dt.itemsize], (rows, width))
    want = R.action_encode_mapped(actions.numpy(), watch.numpy(), uo, to, bits(table.to(dt)), bits(target.to(dt)), weights,
                                  thresholds)
    return got, want, out


def _run_action_bwd(c, lengths, targets, mis, cus):
    L, lib, stream = lib_and_stream()
    weights, thresholds, uih, actions, watch, _, _, g = _action_inputs(c, lengths, targets)
    uo, to = R.offsets_of(uih), R.offsets_of(targets)
    rows, width = int(lengths.sum()), c["T"] * c["da"]
    dt = TORCH[c["dtype"]]
    if c["label"] == K.MISALIGNED:
        # the element path splits the rows into other slots and slabs than the 16-byte path, so the two add in another
        # order: integer terms, whose fp32 sums are exact in every order, make "the same bits as the aligned call" a
        # statement about which rows and columns were read
        d_out = torch.randint(-8, 9, (rows, width), generator=g).to(dt)
    else:
        d_out = torch.randn(rows, width, generator=g).to(dt)
    ws_bytes = lib.hstu_action_encode_bwd_workspace_bytes(rows, width)
    assert ws_bytes == K.K_ACTION_BWD_GROUPS_MAX * 2 * width * 4
    d_table, d_target, ws = Owned(width * 4), Owned(width * 4), Owned(ws_bytes)
    keep = [placed(actions), placed(watch), placed(d_out, mis.get("d_out", 0)), _offsets_dev(uo, c["idx"]), _offsets_dev(to, c["idx"])]
    w, th, tw = i64_array(weights), i64_array([t for t, _ in thresholds]), i64_array([x for _, x in thresholds])

    def call():
        for o in (d_table, d_target, ws):
            o.refill()
        L.check(lib.hstu_action_encode_bwd(keep[2][1], keep[0][1], keep[1][1] if thresholds else None, keep[3].data_ptr(),
                                           keep[4].data_ptr(), w, c["T"], th, tw, len(thresholds), d_table.ptr, d_target.ptr,
                                           ws.ptr, int(uih.sum()), int(targets.sum()), len(lengths), c["da"],
                                           dtype_code(L, c["dtype"]), L.HSTU_INDEX_I32 if c["idx"] == 32 else L.HSTU_INDEX_I64,
                                           stream))
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in (d_table, d_target, ws)), "a guard of d_table / d_target / the workspace was written"
        return d_table.read(np.float32).copy(), d_target.read(np.float32).copy(), ws.read(np.float32).copy()

    first, again = call(), call()
    for a, b, name in zip(first, again, ("d_table", "d_target", "workspace")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: two calls differ"
    ref = R.action_encode_bwd_mapped(d_out.double().numpy(), actions.numpy(), watch.numpy(), uo, to, weights, thresholds, c["da"])
    for name, got in (("table", first[0]), ("target", first[1])):
        assert np.isfinite(got).all(), f"d_{name} holds the sentinel"
        err = np.abs(got.astype(np.float64).reshape(ref["d_" + name].shape) - ref["d_" + name])
        bound = ref["n_" + name] * 2.0**-24 * ref["abs_" + name]
        print(f"{K.p_id(c)} d_{name}: max err {err.max():.3e}, max bound {bound.max():.3e}")
        assert (err <= bound).all(), f"d_{name}: {float((err - bound).max()):.3e} over the bound"
    units = K.p_units(dict(c, mis=mis))
    return first, K.action_bwd_groups(rows, units, cus), width


@pytest.mark.parametrize("case", K.P_CASES, ids=K.p_id)
def test_preprocess_class(case):
    c, cus = case, device_cus()
    assert K.p_lands_on_its_label(c, cus), (cus, K.p_class_facts(c, cus))
    lengths, targets = K.batch_of(c, cus)
    if c["kind"] == "action_fwd":
        got, want, out = _run_action_fwd(c, lengths, targets, c["mis"])
        assert out.guards_intact(), "a guard of out was written"
        assert np.array_equal(got, want), f"{int((got != want).any(1).sum())} of {got.shape[0]} rows differ"
        if c["mis"]:
            aligned, _, _ = _run_action_fwd(c, lengths, targets, {})
            assert np.array_equal(got, aligned), "the misaligned call differs from the aligned one"
    elif c["kind"] == "action_bwd":
        first, groups, width = _run_action_bwd(c, lengths, targets, c["mis"], cus)
        if c["mis"]:
            aligned, _, _ = _run_action_bwd(c, lengths, targets, {}, cus)
            for a, b in zip(first[:2], aligned[:2]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the misaligned call differs from the aligned one"
        if c["label"] in (K.BWD_GROUPS, K.BWD_CLAMP, K.BWD_Y):
            ws = first[2]
            n = groups * 2 * width
            assert np.isfinite(ws[:n]).all(), "a partial of a slab was not written"
            assert (ws[n:].view(np.uint32) == 0xFFFFFFFF).all(), "floats beyond groups x 2 x width were written"
            part = ws[:n].reshape(groups, 2 * width)
            s = np.zeros((4, 2 * width), dtype=np.float32)
            full = groups - groups % 4
            for g in range(full):                      # four running sums over g ...
                s[g % 4] += part[g]
            for g in range(full, groups):              # ... the remainder into the first ...
                s[0] += part[g]
            total = (s[0] + s[1]) + (s[2] + s[3])      # ... then (s0 + s1) + (s2 + s3)
            assert total.dtype == np.float32
            assert np.array_equal(total[:width].view(np.uint32), first[0].view(np.uint32)), "d_table is not the partials' sum"
            assert np.array_equal(total[width:].view(np.uint32), first[1].view(np.uint32)), "d_target is not the partials' sum"
    elif c["kind"] == "combine_fwd":
        _combine_fwd(c, lengths, targets)
    else:
        _combine_bwd(c, lengths, targets)


def _combine_fwd(c, lengths, targets):
    L, lib, stream = lib_and_stream()
    g = torch.Generator().manual_seed(2000 + c["seed"])
    dt, D, Cn, mode = TORCH[c["dtype"]], c["D"], c["C"], c["mode"]
    B, total = len(lengths), int(lengths.sum())
    has_action = c["action"] or mode != K.SUM
    content = torch.randn(total, D, generator=g).to(dt)
    action = torch.randn(total, D, generator=g).to(dt) if has_action else None
    ctx = torch.randn(B, Cn, D, generator=g).to(dt) if Cn else None
    ts = torch.randint(1, 10**9, (total,), generator=g)
    out_len = R.out_lengths(lengths, targets, Cn, mode)
    out_rows = int(out_len.sum())
    out, out_ts = Owned(out_rows * D * dt.itemsize), Owned(out_rows * 8)
    keep = [placed(content), placed(action) if has_action else (None, None), placed(ctx) if Cn else (None, None), placed(ts),
            _offsets_dev(R.offsets_of(lengths), c["idx"]), _offsets_dev(targets, c["idx"]), _offsets_dev(R.offsets_of(out_len), c["idx"])]
    L.check(lib.hstu_combine_embeddings_fwd(keep[0][1], keep[1][1], keep[2][1], keep[3][1], keep[4].data_ptr(), keep[5].data_ptr(),
                                            keep[6].data_ptr(), out.ptr, out_ts.ptr, total - int(targets.sum()), int(targets.sum()),
                                            B, Cn, D, mode, dtype_code(L, c["dtype"]),
                                            L.HSTU_INDEX_I32 if c["idx"] == 32 else L.HSTU_INDEX_I64, stream))
    torch.cuda.synchronize()
    assert out.guards_intact() and out_ts.guards_intact(), "a guard of out / out_ts was written"
    summed = bits(content + action) if (mode == K.SUM and has_action) else None
    want, want_ts, _ = R.combine_mapped(bits(content), bits(action) if has_action else None, bits(ctx) if Cn else None, ts.numpy(),
                                        lengths, targets, mode, summed)
    got = out.read(NP_BITS[dt.itemsize], (out_rows, D))
    assert np.array_equal(got, want), f"{int((got != want).any(1).sum())} of {out_rows} rows differ"
    assert np.array_equal(out_ts.read(np.int64), want_ts), "timestamps"


def _combine_bwd(c, lengths, targets):
    L, lib, stream = lib_and_stream()
    g = torch.Generator().manual_seed(3000 + c["seed"])
    dt, D, Cn, mode = TORCH[c["dtype"]], c["D"], c["C"], c["mode"]
    B, total = len(lengths), int(lengths.sum())
    out_len = R.out_lengths(lengths, targets, Cn, mode)
    out_rows = int(out_len.sum())
    d_out = torch.randn(out_rows, D, generator=g).to(dt)
    want_ctx = bool(Cn and c["d_ctx"])
    d_content = Owned(total * D * dt.itemsize)
    d_action = Owned(total * D * dt.itemsize) if c["d_action"] else None
    d_ctx = Owned(B * Cn * D * dt.itemsize) if want_ctx else None
    keep = [placed(d_out), _offsets_dev(R.offsets_of(lengths), c["idx"]), _offsets_dev(targets, c["idx"]),
            _offsets_dev(R.offsets_of(out_len), c["idx"])]
    L.check(lib.hstu_combine_embeddings_bwd(keep[0][1], keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), d_content.ptr,
                                            d_action.ptr if d_action else None, d_ctx.ptr if d_ctx else None,
                                            total - int(targets.sum()), int(targets.sum()), B, Cn, D, mode, dtype_code(L, c["dtype"]),
                                            L.HSTU_INDEX_I32 if c["idx"] == 32 else L.HSTU_INDEX_I64, stream))
    torch.cuda.synchronize()
    assert all(o.guards_intact() for o in (d_content, d_action, d_ctx) if o), "a guard of a gradient was written"
    dc, da, dx = R.combine_bwd_mapped(bits(d_out), lengths, targets, Cn, mode, c["d_action"])
    u = NP_BITS[dt.itemsize]
    got = d_content.read(u, (total, D))
    assert np.array_equal(got, dc), f"d_content: {int((got != dc).any(1).sum())} of {total} rows differ"
    if d_action:
        got = d_action.read(u, (total, D))
        assert np.array_equal(got, da), f"d_action: {int((got != da).any(1).sum())} of {total} rows differ"
    if d_ctx:
        assert np.array_equal(d_ctx.read(u, (B, Cn, D)), dx), "d_contextual"


# ------------------------------------------------------------------------------------------------ research_preprocess.hip
def bf16_round(x):
    """float32 -> bf16 bit patterns, round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def to_bits(x32, name):
    """a float32 array rounded once to the dtype `name`, as bit patterns"""
    if name == K.F32:
        return np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    return bf16_round(x32) if name == K.BF16 else np.ascontiguousarray(x32, dtype=np.float32).astype(np.float16).view(np.uint16)


def _research_inputs(c):
    g = torch.Generator().manual_seed(4000 + c["B"] + 7 * c["N"] + c["di"])
    B, N, di, dr, Rn, layout = c["B"], c["N"], c["di"], c["dr"], c["R"], c["layout"]
    n_out, do = K.n_out_of(layout, N), K.d_out_of(layout, di, dr)
    te, to = TORCH[c["emb"]], TORCH[c["out"]]
    t = dict(n_out=n_out, do=do, P=n_out + c["extra_pos"])
    t["ids"] = torch.randint(0, 4, (B, N), generator=g)                                # a quarter of the ids are zero
    t["ratings"] = None
    if layout != K.PLAIN:
        allowed = torch.tensor([r for r in range(Rn) if r != c["unused_rating"]])
        t["ratings"] = allowed[torch.randint(0, len(allowed), (B, N), generator=g)]
        t["rat"] = (0.1 * torch.randn(Rn, dr, generator=g)).to(to)
    t["emb"] = (0.05 * torch.randn(B, N, di, generator=g)).to(te) if c["fwd"] else None
    t["pos"] = (0.1 * torch.randn(t["P"], do, generator=g)).to(to)
    t["g"] = torch.randn(B, n_out, do, generator=g).to(to)
    return t


def _ratings_dev(c, t):
    if t["ratings"] is None:
        return None
    return t["ratings"].to(torch.int64 if c["r64"] else torch.int32).to(DEV)


def _source_rows(c, t, f32):
    """(B, N', Do) float32: what every output element scales -- the embedding, or the rating row of the rated layouts --
    and (B, N') the 0 / 1 mask of its source row"""
    x = f32(t["emb"])
    m = (t["ids"].numpy() != 0).astype(np.float32)
    if c["layout"] == K.PLAIN:
        return x, m
    rr = f32(t["rat"])[t["ratings"].numpy()]
    if c["layout"] == K.CONCAT:
        return np.concatenate([x, rr], axis=2), m
    return np.stack([x, rr], axis=2).reshape(c["B"], 2 * c["N"], c["di"]), np.repeat(m, 2, axis=1)


def _keep_scale(c, t):
    if not c["p"]:
        return None, None
    keep, scale = dropout_keep_mask(c["seed"], c["B"] * t["n_out"], t["do"], c["p"])
    return keep.reshape(c["B"], t["n_out"], t["do"]), np.float32(scale)


def _research_fwd(c, t):
    L, lib, stream = lib_and_stream()
    B, N, n_out, do, mis = c["B"], c["N"], t["n_out"], t["do"], c["mis"]
    to = TORCH[c["out"]]
    out, valid = Owned(B * n_out * do * to.itemsize, mis.get("out", 0)), Owned(B * n_out * 4)
    rt = _ratings_dev(c, t)
    keep = [placed(t["ids"]), placed(t["emb"], mis.get("emb", 0)), placed(t["pos"], mis.get("pos", 0)),
            placed(t["rat"], mis.get("rat", 0)) if c["layout"] != K.PLAIN else (None, None)]
    L.check(lib.hstu_input_preprocess_fwd(keep[0][1], keep[1][1], rt.data_ptr() if rt is not None else None, keep[2][1], keep[3][1],
                                          out.ptr, valid.ptr, B, N, c["di"], c["dr"], t["P"], c["R"], c["layout"], float(c["p"]),
                                          int(c["seed"]), dtype_code(L, c["emb"]), dtype_code(L, c["out"]),
                                          L.HSTU_INDEX_I64 if c["r64"] else L.HSTU_INDEX_I32, stream))
    torch.cuda.synchronize()
    assert out.guards_intact() and valid.guards_intact(), "a guard of out / valid_mask was written"
    f32 = lambda x: x.float().numpy()
    src, m = _source_rows(c, t, f32)
    s = np.float32(float(do) ** 0.5)
    v = (src * s) + f32(t["pos"])[:n_out][None]                 # fl(fl(x s) + pos): float32 arrays, one rounding per operator
    keep_mask, scale = _keep_scale(c, t)
    if keep_mask is not None:
        v = np.where(keep_mask, v * scale, np.float32(0))
    v = v * m[:, :, None]
    assert v.dtype == np.float32
    want = to_bits(v, c["out"])
    got = out.read(NP_BITS[to.itemsize], (B, n_out, do))
    assert np.array_equal(got, want), f"out: {int((got != want).sum())} of {got.size} elements differ"
    assert np.array_equal(valid.read(np.float32, (B, n_out)).view(np.uint32), m.view(np.uint32)), "valid_mask"


def _research_bwd(c, t):
    L, lib, stream = lib_and_stream()
    B, N, n_out, do, di, dr, Rn, mis, layout = c["B"], c["N"], t["n_out"], t["do"], c["di"], c["dr"], c["R"], c["mis"], c["layout"]
    te = TORCH[c["emb"]]
    rated = layout != K.PLAIN
    ws_bytes = lib.hstu_input_preprocess_bwd_workspace_bytes(B, N, di, dr, Rn, layout)
    pos_bytes, rat_bytes = K.research_workspace_bytes(layout, B, N, di, dr, Rn)
    assert ws_bytes == pos_bytes + rat_bytes
    d_emb = Owned(B * N * di * te.itemsize, mis.get("d_emb", 0))
    d_pos, ws = Owned(t["P"] * do * 4), Owned(ws_bytes)
    d_rat = Owned(Rn * dr * 4) if rated else None
    outs = [o for o in (d_emb, d_pos, d_rat, ws) if o]
    rt = _ratings_dev(c, t)
    keep = [placed(t["ids"]), placed(t["g"], mis.get("d_out", 0))]

    def call():
        for o in outs:
            o.refill()
        L.check(lib.hstu_input_preprocess_bwd(keep[1][1], keep[0][1], rt.data_ptr() if rt is not None else None, d_emb.ptr, d_pos.ptr,
                                              d_rat.ptr if rated else None, ws.ptr, B, N, di, dr, t["P"], Rn, layout, float(c["p"]),
                                              int(c["seed"]), dtype_code(L, c["emb"]), dtype_code(L, c["out"]),
                                              L.HSTU_INDEX_I64 if c["r64"] else L.HSTU_INDEX_I32, stream))
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in outs), "a guard of a gradient / the workspace was written"
        return [o.raw.clone() for o in outs]

    first, again = call(), call()
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two backward calls differ"

    # the truth on the device, a slab of users at a time: h = fl(g m) [fl(. scale) where kept], exact in fp64
    ids, g, ratings = t["ids"].to(DEV), keep[1][0] if not mis.get("d_out") else t["g"].to(DEV), (t["ratings"].to(DEV) if rated else None)
    keep_mask, scale = _keep_scale(c, t)
    s32 = torch.tensor(float(np.float32(float(do) ** 0.5)), dtype=torch.float32, device=DEV)
    s64 = s32.double()
    m_src = (ids != 0).float()
    m_out = m_src.repeat_interleave(2, dim=1) if layout == K.INTERLEAVE else m_src
    pos_sum, pos_abs = (torch.zeros(n_out, do, dtype=torch.float64, device=DEV) for _ in range(2))
    if rated:
        rat_sum, rat_abs = (torch.zeros(Rn, dr, dtype=torch.float64, device=DEV) for _ in range(2))
        n_r = torch.stack([((ratings == k) & (ids != 0)).sum() for k in range(Rn)]).double().view(-1, 1)
    got_emb = torch.from_numpy(d_emb.read(np.int16 if te.itemsize == 2 else np.int32, (B, N, di))).to(DEV)
    step = max(1, (1 << 22) // (n_out * do))
    bad = 0
    for b0 in range(0, B, step):
        sl = slice(b0, min(b0 + step, B))
        h = g[sl].float() * m_out[sl].unsqueeze(-1)
        if keep_mask is not None:
            km = torch.from_numpy(keep_mask[sl]).to(DEV)
            h = torch.where(km, h * torch.tensor(float(scale), dtype=torch.float32, device=DEV), torch.zeros((), device=DEV))
        item = h[:, :, :di] if layout == K.CONCAT else (h[:, 0::2] if layout == K.INTERLEAVE else h)
        want = (item * s32).to(te)                                                   # d_emb = fl(h s), rounded to the embedding dtype
        bad += int((want.view(got_emb.dtype) != got_emb[sl]).sum())
        h64 = h.double()
        pos_sum += h64.sum(0)
        pos_abs += h64.abs().sum(0)
        if rated:
            part = h64[:, :, di:] if layout == K.CONCAT else h64[:, 1::2]            # (b, N, Dr): the rating part of every source row
            onehot = torch.nn.functional.one_hot(ratings[sl], Rn).double() * (ids[sl] != 0).unsqueeze(-1)
            rat_sum += torch.einsum("bnr,bnd->rd", onehot, part)
            rat_abs += torch.einsum("bnr,bnd->rd", onehot, part.abs())
    assert bad == 0, f"d_past_embeddings: {bad} of {got_emb.numel()} elements differ from fl(h s)"

    got_pos = torch.from_numpy(d_pos.read(np.float32, (t["P"], do))).to(DEV)
    assert bool(torch.isfinite(got_pos).all()), "d_pos holds the sentinel"
    err, bound = (got_pos[:n_out].double() - pos_sum).abs(), (B + 1) * 2.0**-24 * pos_abs
    print(f"{K.r_id(c)} d_pos: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
    assert bool((err <= bound).all()), f"d_pos: {float((err - bound).max()):.3e} over the bound"
    assert bool((got_pos[n_out:].view(torch.int32) == 0).all()), "position rows beyond N' are exactly zero"
    if rated:
        got_rat = torch.from_numpy(d_rat.read(np.float32, (Rn, dr))).to(DEV)
        assert bool(torch.isfinite(got_rat).all()), "d_rating holds the sentinel"
        err, bound = (got_rat.double() - rat_sum * s64).abs(), (n_r + 2) * 2.0**-24 * rat_abs * s64
        print(f"{K.r_id(c)} d_rating: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
        assert bool((err <= bound).all()), f"d_rating: {float((err - bound).max()):.3e} over the bound"
        assert float(n_r[c["unused_rating"]]) == 0 and float(n_r.sum()) > 0
        assert bool((got_rat[c["unused_rating"]].view(torch.int32) == 0).all()), "the row of a rating never seen is exactly zero"

    # the workspace: exactly the slabs the geometry names were written
    f = K.r_class_facts(c)
    part = ws.read(np.float32)
    n = f["slabs"] * n_out * do
    assert np.isfinite(part[:n]).all(), "a d_pos partial of a slab was not written"
    assert (part[n:pos_bytes // 4].view(np.uint32) == 0xFFFFFFFF).all(), "d_pos partials beyond the slabs were written"
    if rated:
        rp = part[pos_bytes // 4:]
        n = f["rating_groups"] * Rn * dr
        assert np.isfinite(rp[:n]).all() and (rp[n:].view(np.uint32) == 0xFFFFFFFF).all(), "the d_rating partials"


def test_the_python_wrapper_takes_fp16():
    """the op through its wrapper in fp16 at an odd D (one-element pieces): the float32 chain rounded once, the sign of a
    masked row's zeros included, and gradients in the dtypes of their leaves"""
    from generative_recommenders_amd.ops.research_preprocess import research_input_preprocess

    c = dict(K.R_CASES[0], layout=K.PLAIN, emb=K.F16, out=K.F16, B=5, N=7, di=67, dr=0, R=0, extra_pos=1, p=0.0, fwd=True)
    t = _research_inputs(c)
    emb, pos = t["emb"].to(DEV).requires_grad_(True), t["pos"].to(DEV).requires_grad_(True)
    out, valid = research_input_preprocess(t["ids"].to(DEV), emb, pos, layout=K.PLAIN)
    assert out.dtype == torch.float16 and valid.dtype == torch.float32
    m = (t["ids"].numpy() != 0).astype(np.float32)
    v = ((t["emb"].float().numpy() * np.float32(67.0 ** 0.5)) + t["pos"].float().numpy()[:7][None]) * m[:, :, None]
    assert (to_bits(v, K.F16) == 0x8000).any(), "the case holds a negative zero"
    assert np.array_equal(bits(out), to_bits(v, K.F16))
    (out * t["g"].to(DEV)).sum().backward()
    h = (t["g"].float().numpy() * m[:, :, None]) * np.float32(67.0 ** 0.5)
    assert emb.grad.dtype == torch.float16 and np.array_equal(bits(emb.grad), to_bits(h, K.F16))
    assert pos.grad.dtype == torch.float16 and float(pos.grad[7:].abs().max()) == 0.0


@pytest.mark.parametrize("case", K.R_CASES, ids=K.r_id)
def test_research_class(case):
    assert K.r_lands_on_its_label(case), K.r_class_facts(case)
    t = _research_inputs(case)
    if case["fwd"]:
        _research_fwd(case, t)
    _research_bwd(case, t)
