"""GPU tests of the research-path (relative position + bucketed time bias) attention and layer
against the golden vectors of the reference's research/modeling/sequential/hstu.py and the oracle."""

import numpy as np
import pytest
import torch

from conftest import load_cases, record_parity
from oracle import hstu_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mods():
    from generative_recommenders_amd.research.modeling.sequential import hstu

    return hstu


def _close(got, ref, rtol, atol_scale, what):
    g = got.detach().float().cpu().numpy().astype(np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert g.shape == ref.shape, f"{what}: {g.shape} vs {ref.shape}"
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(g - ref)
    m = record_parity(what, g, ref, str(got.dtype).replace("torch.", ""))
    # relative Frobenius gate by output dtype: 1.5 x the largest error measured on MI355X (profiles/r02_parity_errors.md)
    gate = {torch.float32: 1.5e-6, torch.bfloat16: 3.6e-3, torch.float16: 4.5e-4}[got.dtype]
    assert m["rel_fro"] <= gate, f"{what}: relative Frobenius error {m['rel_fro']:.3e} (gate {gate})"
    bad = err > rtol * np.abs(ref) + atol_scale * scale
    assert not bad.any(), f"{what}: {bad.sum()}/{bad.size} out of tolerance, max err {err.max():.3e}, scale {scale:.3e}"


def test_golden_rel_bias_attention_fwd_bwd():
    """fp32, vs the reference's _hstu_attention_maybe_from_cache + RelativeBucketedTimeAndPositionBasedBias."""
    c = load_cases("research_attention.npz")[0]
    m = _mods()
    n, H, A, Ld = int(c["n"]), int(c["H"]), int(c["A"]), int(c["Ld"])
    bias = m.RelativeBucketedTimeAndPositionBasedBias(max_seq_len=n, num_buckets=128).to(DEV)
    with torch.no_grad():
        bias._pos_w.copy_(torch.from_numpy(c["pos_w"]))
        bias._ts_w.copy_(torch.from_numpy(c["ts_w"]))
    q = torch.from_numpy(c["q"]).to(DEV).requires_grad_()
    k = torch.from_numpy(c["k"]).to(DEV).requires_grad_()
    v = torch.from_numpy(c["v"]).to(DEV).requires_grad_()
    out = m.hstu_rel_bias_attention(H, A, Ld, q, k, v, torch.from_numpy(c["offsets"]).to(DEV),
                                    torch.from_numpy(c["ts"]).to(DEV), n, bias)
    _close(out, c["out"], 1e-3, 2e-6, "out")
    out.backward(torch.from_numpy(c["g"]).to(DEV))
    _close(q.grad, c["dq"], 1e-3, 1e-5, "dq")
    _close(k.grad, c["dk"], 1e-3, 1e-5, "dk")
    _close(v.grad, c["dv_"], 1e-3, 1e-5, "dv")
    _close(bias._pos_w.grad, c["dpos_w"], 2e-3, 1e-4, "dpos_w")
    _close(bias._ts_w.grad, c["dts_w"], 2e-3, 1e-4, "dts_w")


@pytest.mark.parametrize("dtype,H,A,Ld,n,with_ts", [(torch.float32, 1, 50, 50, 60, True), (torch.bfloat16, 4, 64, 64, 211, True),
                                                    (torch.float32, 2, 32, 32, 40, False), (torch.bfloat16, 2, 16, 32, 61, True),
                                                    (torch.float32, 2, 32, 32, 90, "ms"),
                                                    # LDS-tight shapes: 128-wide heads at N = 200 (the K/V block fills the
                                                    # LDS: fewer privatised histogram copies) and N = 420 (several key
                                                    # blocks: fp32 dq accumulation + bias histograms together)
                                                    (torch.bfloat16, 2, 128, 128, 200, True), (torch.bfloat16, 1, 128, 128, 420, True),
                                                    (torch.float32, 1, 64, 64, 300, True)])
def test_rel_bias_attention_vs_oracle(dtype, H, A, Ld, n, with_ts):
    """ML-1M-like (1 head, d=50 -> padded), ML-20M-like (4 x 64, N = 211), position-only bias,
    Amazon-Books-like short sequences (N = 61, long-tail lengths)."""
    m = _mods()
    torch.manual_seed(n + H)                           # module initialisation draws from torch's generator: fix it
    rng = np.random.default_rng(n + H)
    B = 6
    lengths = rng.integers(1, n + 1, size=B)
    lengths[0] = n
    lengths[1] = max(1, n // 20)
    off = O.complete_cumsum(lengths.astype(np.int64))
    Lt = int(off[-1])
    ts = np.sort(rng.integers(0, 10**8, size=(B, n)), axis=1).astype(np.int64)
    if with_ts == "ms":
        # millisecond timestamps spread over years: offsets beyond 30 bits -> the kernels' 64-bit time arithmetic
        # (rows within 2^30 of their first timestamp take the 32-bit path); one user stays small to mix both
        ts[1:] = ts[1:] * 40_000 + 1_600_000_000_000
        assert (ts[1:, -1] - ts[1:, 0]).min() > 2**31
    mk = lambda d: torch.from_numpy(rng.standard_normal((Lt, H * d)) * 0.3).to(dtype)
    q, k, v = mk(A), mk(A), mk(Ld)
    g = torch.from_numpy(rng.standard_normal((Lt, H * Ld))).to(dtype)
    bias = (m.RelativeBucketedTimeAndPositionBasedBias(n, 128) if with_ts else m.RelativePositionalBias(n)).to(DEV)
    pos_w, ts_w, _, _ = bias.bias_params()
    qd, kd, vd = (t.to(DEV).requires_grad_() for t in (q, k, v))
    # (the position-only module ignores the timestamps but the caller still passes them: without timestamps the
    # reference adds no bias at all, hstu.py:205-206)
    out = m.hstu_rel_bias_attention(H, A, Ld, qd, kd, vd, torch.from_numpy(off).to(DEV), torch.from_numpy(ts).to(DEV), n, bias)
    out.backward(g.to(DEV))
    pw = pos_w.detach().double().cpu().numpy()
    tw = None if ts_w is None else ts_w.detach().double().cpu().numpy()
    q3, k3, v3 = (t.double().numpy().reshape(Lt, H, -1) for t in (q, k, v))
    ref = O.rel_bias_attention_fwd(n, q3, k3, v3, off, ts if with_ts else None, pw, tw)
    rq, rk, rv, rpos, rts = O.rel_bias_attention_bwd(n, g.double().numpy().reshape(Lt, H, Ld), q3, k3, v3, off,
                                                     ts if with_ts else None, pw, tw)
    tol = (1e-3, 1e-5) if dtype == torch.float32 else (3e-2, 6e-3)
    tag = str(dtype).replace("torch.", "")
    _close(out, ref.reshape(Lt, -1), *tol, "out")
    _close(qd.grad, rq.reshape(Lt, -1), *tol, "dq")
    _close(kd.grad, rk.reshape(Lt, -1), *tol, "dk")
    _close(vd.grad, rv.reshape(Lt, -1), *tol, "dv")
    btol = (2e-3, 1e-4)     # fp32 sums of dS' whatever the I/O dtype (+ the Frobenius gate of _close)
    _close(pos_w.grad, rpos, *btol, f"dpos_w[{tag} attention]")
    if with_ts:
        _close(ts_w.grad, rts, *btol, f"dts_w[{tag} attention]")


@pytest.mark.parametrize("dtype,H,n,B", [(torch.bfloat16, 4, 211, 600), (torch.float16, 2, 100, 900), (torch.bfloat16, 3, 224, 300),
                                          (torch.bfloat16, 1, 33, 700),
                                          # 129..160 rows: the forward's SECOND query block has one wave with rows, the first
                                          # four -- its per-user bucket bytes must be sized by the larger block (sized by the
                                          # last one, the first block's bytes ran past the allocation: 1-10 % errors in `out`;
                                          # found by tools/fuzz_attention.py --bias in round 3)
                                          (torch.bfloat16, 4, 146, 60), (torch.float16, 5, 155, 40), (torch.bfloat16, 6, 129, 30)])
def test_folded_bias_backward_many_users_per_workgroup(dtype, H, n, B):
    """The research-path backward on the folded schedule (hstu_attn_bwd_fold_bias_kernel: head dim 64, 16-bit I/O): more
    users than CUs, so every persistent workgroup walks several users (tables restaged, bucket bytes recomputed per user,
    ONE histogram pair per workgroup), every tile count 1..7 incl. the full 224 rows, empty users, odd head counts.
    Against the fp64 oracle, user by user (timestamps kept off the time-bucket boundaries, as in test_configs_gpu.py: the
    table gradients are then exact sums and the fp32 gate applies)."""
    from generative_recommenders_amd.ops import _launch
    from test_configs_gpu import _timestamps_off_bucket_boundaries

    m = _mods()
    d = 64
    assert _launch.attn_bwd_kernel_name(dtype, d, d, n, heads=H, with_bias=True).startswith("hstu_attn_bwd_fold_bias_kernel")
    torch.manual_seed(n + B)
    rng = np.random.default_rng(n + B)
    lengths = rng.integers(0, n + 1, size=B)
    lengths[:8] = [n, 0, 1, min(32, n), min(33, n), n - 1, 0, n]
    off = O.complete_cumsum(lengths.astype(np.int64))
    Lt = int(off[-1])
    ts = _timestamps_off_bucket_boundaries(rng, B, n)
    mk = lambda: torch.from_numpy(rng.standard_normal((Lt, H * d)) * 0.3).to(dtype)
    q, k, v = mk(), mk(), mk()
    g = torch.from_numpy(rng.standard_normal((Lt, H * d))).to(dtype)
    bias = m.RelativeBucketedTimeAndPositionBasedBias(n, 128).to(DEV)
    with torch.no_grad():
        bias._ts_w.normal_(0, 0.05)
        bias._pos_w.normal_(0, 0.05)
    pos_w, ts_w, _, _ = bias.bias_params()
    qd, kd, vd = (t.to(DEV).requires_grad_() for t in (q, k, v))
    out = m.hstu_rel_bias_attention(H, d, d, qd, kd, vd, torch.from_numpy(off).to(DEV), torch.from_numpy(ts).to(DEV), n, bias)
    out.backward(g.to(DEV))
    pw, tw = pos_w.detach().double().cpu().numpy(), ts_w.detach().double().cpu().numpy()
    q3, k3, v3 = (t.double().numpy().reshape(Lt, H, d) for t in (q, k, v))
    ref = O.rel_bias_attention_fwd(n, q3, k3, v3, off, ts, pw, tw)
    rq, rk, rv, rpos, rts = O.rel_bias_attention_bwd(n, g.double().numpy().reshape(Lt, H, d), q3, k3, v3, off, ts, pw, tw)
    tol = (3e-2, 6e-3)
    tag = str(dtype).replace("torch.", "")
    _close(out, ref.reshape(Lt, -1), *tol, "out")
    _close(qd.grad, rq.reshape(Lt, -1), *tol, "dq")
    _close(kd.grad, rk.reshape(Lt, -1), *tol, "dk")
    _close(vd.grad, rv.reshape(Lt, -1), *tol, "dv")
    _close(pos_w.grad, rpos, 2e-3, 1e-4, f"dpos_w[{tag} folded]")
    _close(ts_w.grad, rts, 2e-3, 1e-4, f"dts_w[{tag} folded]")


@pytest.mark.parametrize("d,n,B", [(64, 211, 1500), (16, 61, 3000)])
def test_results_do_not_depend_on_the_launch_order_or_the_hand_out(d, n, B, monkeypatch):
    """Round 6: the research attention launches heavy users first (from 512 users on) and its persistent backward kernels hand users
    out from a counter / in two launches by length class -- who computes a user may differ from run to run, what is computed may not:
    out, dq, dk, dv bit-identical with and without the order and run to run; the table gradients (float atomics into histograms,
    summed per workgroup) to 1e-5 of their norm."""
    m = _mods()
    H, dtype = 4, torch.bfloat16
    rng = np.random.default_rng(B + n)
    lengths = rng.integers(0, n + 1, size=B)
    lengths[rng.integers(0, B, size=B // 20)] = n
    off = O.complete_cumsum(lengths.astype(np.int64))
    Lt = int(off[-1])
    ts = np.sort(rng.integers(0, 10 ** 8, size=(B, n)), axis=1)
    mk = lambda: torch.from_numpy(rng.standard_normal((Lt, H * d)) * 0.3).to(dtype).to(DEV)
    q, k, v, g = mk(), mk(), mk(), mk()
    bias = m.RelativeBucketedTimeAndPositionBasedBias(n, 128).to(DEV)
    with torch.no_grad():
        bias._ts_w.normal_(0, 0.05)
        bias._pos_w.normal_(0, 0.05)
    offd, tsd = torch.from_numpy(off).to(DEV), torch.from_numpy(ts).to(DEV)

    def run():
        qd, kd, vd = (t.clone().requires_grad_() for t in (q, k, v))
        bias.zero_grad()
        out = m.hstu_rel_bias_attention(H, d, d, qd, kd, vd, offd, tsd, n, bias)
        out.backward(g)
        return [out.detach(), qd.grad, kd.grad, vd.grad], [bias._pos_w.grad.clone(), bias._ts_w.grad.clone()]

    a, ta = run()
    b, tb = run()
    monkeypatch.setattr(m, "_ORDER_MIN_USERS", 10 ** 9)       # batch order
    c, tc = run()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    for x, y, z in zip(ta, tb, tc):
        den = float(x.double().norm())
        assert float((x.double() - y.double()).norm()) <= 1e-5 * den and float((x.double() - z.double()).norm()) <= 1e-5 * den


@pytest.mark.parametrize("dtype,H,d,n,B,with_ts", [(torch.bfloat16, 4, 16, 61, 700, True), (torch.float16, 6, 32, 64, 300, True),
                                                    (torch.bfloat16, 1, 8, 17, 500, True), (torch.bfloat16, 3, 24, 33, 400, False),
                                                    (torch.bfloat16, 2, 16, 61, 3, True)])
def test_short_sequence_bias_kernels(dtype, H, d, n, B, with_ts):
    """The research path at the Amazon-Books shapes (N <= 64, head dims <= 32, 16-bit): hstu_attn_{fwd,bwd}_solo_bias_kernel --
    a workgroup per user at a time, its four waves the heads (more heads than waves, one head, fewer users than CUs), tables
    restaged per user, ONE histogram pair per persistent workgroup.  Long-tail lengths with empty users and full-length ones;
    position + time tables and position-only.  Against the fp64 oracle."""
    from generative_recommenders_amd.ops import _launch
    from test_configs_gpu import _timestamps_off_bucket_boundaries

    m = _mods()
    assert _launch.attn_bwd_kernel_name(dtype, d, d, n, heads=H, with_bias=True).startswith("hstu_attn_bwd_solo_bias_kernel")
    assert _launch.attn_fwd_kernel_name(dtype, d, d, n, heads=H, with_bias=True).startswith("hstu_attn_fwd_solo_bias_kernel")
    torch.manual_seed(n + B)
    rng = np.random.default_rng(n + B)
    lengths = rng.integers(0, max(n // 2, 2), size=B)
    lengths[rng.random(B) < 0.05] = n
    lengths[:3] = [n, 0, 1]
    off = O.complete_cumsum(lengths.astype(np.int64))
    Lt = int(off[-1])
    ts = _timestamps_off_bucket_boundaries(rng, B, n)
    mk = lambda: torch.from_numpy(rng.standard_normal((Lt, H * d)) * 0.5).to(dtype)
    q, k, v = mk(), mk(), mk()
    g = torch.from_numpy(rng.standard_normal((Lt, H * d))).to(dtype)
    bias = (m.RelativeBucketedTimeAndPositionBasedBias(n, 128) if with_ts else m.RelativePositionalBias(n)).to(DEV)
    with torch.no_grad():
        for prm in bias.parameters():
            prm.normal_(0, 0.05)
    pos_w, ts_w, _, _ = bias.bias_params()
    qd, kd, vd = (t.to(DEV).requires_grad_() for t in (q, k, v))
    out = m.hstu_rel_bias_attention(H, d, d, qd, kd, vd, torch.from_numpy(off).to(DEV), torch.from_numpy(ts).to(DEV), n, bias)
    out.backward(g.to(DEV))
    pw = pos_w.detach().double().cpu().numpy()
    tw = None if ts_w is None else ts_w.detach().double().cpu().numpy()
    q3, k3, v3 = (t.double().numpy().reshape(Lt, H, d) for t in (q, k, v))
    ref = O.rel_bias_attention_fwd(n, q3, k3, v3, off, ts if with_ts else None, pw, tw)
    rq, rk, rv, rpos, rts = O.rel_bias_attention_bwd(n, g.double().numpy().reshape(Lt, H, d), q3, k3, v3, off,
                                                     ts if with_ts else None, pw, tw)
    tol = (3e-2, 6e-3)
    tag = str(dtype).replace("torch.", "")
    _close(out, ref.reshape(Lt, -1), *tol, "out")
    _close(qd.grad, rq.reshape(Lt, -1), *tol, "dq")
    _close(kd.grad, rk.reshape(Lt, -1), *tol, "dk")
    _close(vd.grad, rv.reshape(Lt, -1), *tol, "dv")
    _close(pos_w.grad, rpos, 2e-3, 1e-4, f"dpos_w[{tag} solo]")
    if with_ts:
        _close(ts_w.grad, rts, 2e-3, 1e-4, f"dts_w[{tag} solo]")


_GUARD = 4 << 20


@pytest.mark.parametrize("dtype,d,n,B,H,bias,det,name", [
    (torch.bfloat16, 16, 61, 8, 4, True, 0, "hstu_attn_bwd_solo_bias_kernel<bf16>"),
    # one head: both length classes write a partial row per user (130 + 130 rows) -- more than users x heads rounded up
    (torch.bfloat16, 16, 61, 130, 1, True, 0, "hstu_attn_bwd_solo_bias_kernel<bf16>"),
    (torch.bfloat16, 64, 100, 3, 2, True, 0, "hstu_attn_bwd_fold_bias_kernel<bf16,64>"),
    (torch.bfloat16, 32, 100, 3, 2, True, 0, "hstu_attn_bwd_kernel<bf16,32,32,bias>"),
    (torch.float32, 128, 256, 3, 2, False, 0, "hstu_attn_bwd_kernel<f32,128,128>"),
    (torch.float32, 128, 256, 3, 2, False, 1, "hstu_attn_bwd_kernel<f32,128,128>")])
def test_backward_stays_inside_its_workspace(dtype, d, n, B, H, bias, det, name):
    """Every schedule that writes a workspace, called through the C ABI with hstu_attn_bwd_workspace_bytes() bytes at the
    head of ONE allocation and 4 MiB of a byte pattern behind them: the pattern survives the backward (memsets, partial
    rows, the user counter, the reduce's chunk sums and the dq accumulator all lie inside the reported size), the
    gradients match the fp64 oracle, and the kernel is the one the case is about."""
    import ctypes as C

    from generative_recommenders_amd import _lib as L
    from generative_recommenders_amd.ops import _launch
    from test_configs_gpu import _timestamps_off_bucket_boundaries

    m = _mods()
    torch.manual_seed(n + B)
    rng = np.random.default_rng(n + B + H)
    lengths = rng.integers(0, n + 1, size=B)
    lengths[:3] = [n, 1, min(32, n)]                       # (both sides of 32: the length classes of the short-sequence kernels)
    lengths[B - 1] = min(33, n)
    off = O.complete_cumsum(lengths.astype(np.int64))
    Lt = int(off[-1])
    mk = lambda s: torch.from_numpy(rng.standard_normal((Lt, H, d)) * s).to(dtype)
    q, k, v, g = mk(0.3), mk(0.3), mk(0.3), mk(1.0)
    qd, kd, vd, gd = (t.to(DEV) for t in (q, k, v, g))
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    offd = _launch._idx(torch.from_numpy(off).to(DEV))
    bp = L.HstuAttnBwdParams()
    _launch._fill_attn_params(bp.fwd, qd, kd, vd, None, offd, None, n, 1.0, 1.0 / n, 0, 0, 0, 0)
    if bias:
        ts = _timestamps_off_bucket_boundaries(rng, B, n)
        mod = m.RelativeBucketedTimeAndPositionBasedBias(n, 128).to(DEV)
        with torch.no_grad():
            for prm in mod.parameters():
                prm.normal_(0, 0.05)
        pos_w, ts_w, num_buckets, bucket_div = mod.bias_params()
        pos32, ts32 = pos_w.detach().float().contiguous(), ts_w.detach().float().contiguous()
        tsd = torch.from_numpy(ts).to(DEV)
        m._fill_bias(bp.fwd, pos32, ts32, tsd, num_buckets, bucket_div)
        dpos, dts = torch.zeros_like(pos32), torch.zeros_like(ts32)
        bp.dpos_w, bp.dts_w = dpos.data_ptr(), dts.data_ptr()
    bp.dout, bp.dq, bp.dk, bp.dv = gd.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    bp.do_row_stride, bp.do_head_stride = gd.stride(0), gd.stride(1)
    bp.dq_row_stride, bp.dq_head_stride = dq.stride(0), dq.stride(1)
    bp.dk_row_stride, bp.dk_head_stride = dk.stride(0), dk.stride(1)
    bp.dv_row_stride, bp.dv_head_stride = dv.stride(0), dv.stride(1)
    bp.total_rows = Lt
    bp.deterministic = det
    lib = L.lib()
    buf = C.create_string_buffer(128)
    L.check(lib.hstu_attn_bwd_kernel_name(C.byref(bp), buf, 128))
    assert buf.value.decode() == name
    ws_bytes = lib.hstu_attn_bwd_workspace_bytes(C.byref(bp))
    assert ws_bytes > 0
    ws = torch.full((ws_bytes + _GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    bp.workspace = ws.data_ptr()
    with torch.cuda.device(qd.device):
        L.check(lib.hstu_attn_bwd(C.byref(bp), L.current_stream_ptr(qd.device)))
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == 0xA5).all()), "the backward wrote past hstu_attn_bwd_workspace_bytes()"
    q3, k3, v3, g3 = (t.double().numpy() for t in (q, k, v, g))
    tol = (1e-3, 1e-5) if dtype == torch.float32 else (3e-2, 6e-3)
    if bias:
        pw, tw = pos32.double().cpu().numpy(), ts32.double().cpu().numpy()
        rq, rk, rv, rpos, rts = O.rel_bias_attention_bwd(n, g3, q3, k3, v3, off, ts, pw, tw)
        tag = f"{str(dtype).replace('torch.', '')} guard band"
        _close(dpos, rpos, 2e-3, 1e-4, f"dpos_w[{tag}]")
        _close(dts, rts, 2e-3, 1e-4, f"dts_w[{tag}]")
    else:
        rq, rk, rv = O.hstu_mha_bwd(n, 1.0, g3, q3, k3, v3, off)
    _close(dq, rq, *tol, "dq")
    _close(dk, rk, *tol, "dk")
    _close(dv, rv, *tol, "dv")


def test_research_layer_forward_backward_runs_and_matches_composition():
    """SequentialTransductionUnitJagged on the fused kernels == the same math composed from the
    oracle pieces (LN without affine -> uvqk -> SiLU on all -> bias attention -> u * LN(attn) -> Linear + x)."""
    m = _mods()
    torch.manual_seed(0)
    D, H, A, Ld, n, B = 32, 2, 16, 16, 30, 4
    layer = m.SequentialTransductionUnitJagged(D, Ld, A, 0.0, 0.0, H, "silu",
                                               m.RelativeBucketedTimeAndPositionBasedBias(n, 128)).to(DEV)
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, n + 1, size=B)
    off = O.complete_cumsum(lengths.astype(np.int64))
    Lt = int(off[-1])
    ts = np.sort(rng.integers(0, 10**7, size=(B, n)), axis=1).astype(np.int64)
    x = torch.randn(Lt, D, device=DEV, requires_grad=True)
    mask = torch.ones(n, n, device=DEV)
    y, _ = layer(x, torch.from_numpy(off).to(DEV), torch.from_numpy(ts).to(DEV), mask)
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert layer._uvqk.grad is not None and layer._rel_attn_bias._ts_w.grad is not None
    # reference composition in fp64
    xn = x.detach().double().cpu().numpy()
    nx = O.layer_norm_fwd(xn, np.ones(D), np.zeros(D), 1e-6)
    mm = nx @ layer._uvqk.detach().double().cpu().numpy()
    mm = mm / (1 + np.exp(-mm))
    u, v, q, k = np.split(mm, [Ld * H, 2 * Ld * H, 2 * Ld * H + A * H], axis=1)
    pos_w, ts_w, _, _ = layer._rel_attn_bias.bias_params()
    attn = O.rel_bias_attention_fwd(n, q.reshape(Lt, H, A), k.reshape(Lt, H, A), v.reshape(Lt, H, Ld), off, ts,
                                    pos_w.detach().double().cpu().numpy(), ts_w.detach().double().cpu().numpy())
    a = O.layer_norm_fwd(attn.reshape(Lt, -1), np.ones(Ld * H), np.zeros(Ld * H), 1e-6)
    ref = (u * a) @ layer._o.weight.detach().double().cpu().numpy().T + layer._o.bias.detach().double().cpu().numpy() + xn
    _close(y, ref, 1e-3, 1e-4, "layer out")
    sd_keys = sorted(layer.state_dict())
    assert sd_keys == ["_o.bias", "_o.weight", "_rel_attn_bias._pos_w", "_rel_attn_bias._ts_w", "_uvqk"]


# ------------------------------------------------------------------ the layer stack against the reference itself
def _load_research_stack(c):
    """HSTUJagged of two SequentialTransductionUnitJagged layers with the golden case's parameters"""
    m = _mods()
    n, D, H, A, Ld = (int(c[k]) for k in ("n", "D", "H", "A", "Ld"))
    layers = [m.SequentialTransductionUnitJagged(
        embedding_dim=D, linear_hidden_dim=Ld, attention_dim=A, dropout_ratio=0.0, attn_dropout_ratio=0.0, num_heads=H,
        linear_activation="silu", relative_attention_bias_module=m.RelativeBucketedTimeAndPositionBasedBias(n, 128),
        normalization="rel_bias", linear_config="uvqk", concat_ua=bool(int(c["concat_ua"])), epsilon=1e-6) for _ in range(2)]
    model = m.HSTUJagged(layers, autocast_dtype=None)
    sd = {k[2:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("p:")}
    model.load_state_dict(sd, strict=True)          # the reference's state_dict keys, unchanged
    return model.to(DEV)


@pytest.mark.parametrize("idx", range(2))
def test_research_layer_stack_golden_fwd_bwd(idx):
    """HSTUJagged.jagged_forward + backward vs the reference's (research/modeling/sequential/hstu.py:226-540), fp32:
    output, input gradient, EVERY parameter gradient (incl. both bias tables of both layers) and the cache states."""
    c = load_cases("research_layer.npz")[idx]
    model = _load_research_stack(c)
    n = int(c["n"])
    off = torch.from_numpy(c["offsets"]).to(DEV)
    ts = torch.from_numpy(c["ts"]).to(DEV)
    mask = 1.0 - torch.triu(torch.ones(n, n, device=DEV), diagonal=1)
    x = torch.from_numpy(c["x"]).to(DEV).requires_grad_()
    y, cache = model.jagged_forward(x=x, x_offsets=off, all_timestamps=ts, invalid_attn_mask=mask, return_cache_states=True)
    _close(y, c["y"], 1e-3, 1e-5, "y")
    y.backward(torch.from_numpy(c["g"]).to(DEV))
    _close(x.grad, c["dx"], 1e-3, 1e-5, "dx")
    for name, prm in model.named_parameters():
        _close(prm.grad, c["g:" + name], 2e-3, 2e-5, "grad " + name)
    for li, (cv, cq, ck, co) in enumerate(cache):
        _close(cv, c[f"cache{li}:v"], 1e-3, 1e-5, f"cache{li} v")
        _close(cq, c[f"cache{li}:q"], 1e-3, 1e-5, f"cache{li} padded q")
        _close(ck, c[f"cache{li}:k"], 1e-3, 1e-5, f"cache{li} padded k")
        _close(co, c[f"cache{li}:out"], 1e-3, 1e-5, f"cache{li} outputs")
    # dense (B, N, D) entry point: pads with zeros
    B = off.numel() - 1
    dense = torch.zeros(B, n, x.shape[1], device=DEV)
    for b in range(B):
        dense[b, : int(off[b + 1] - off[b])] = x.detach()[int(off[b]) : int(off[b + 1])]
    yd, _ = model(x=dense, x_offsets=off, all_timestamps=ts, invalid_attn_mask=mask)
    for b in range(B):
        lb = int(off[b + 1] - off[b])
        assert torch.equal(yd[b, :lb], y.detach()[int(off[b]) : int(off[b + 1])]) and bool((yd[b, lb:] == 0).all())


@pytest.mark.parametrize("idx", range(2))
def test_research_layer_stack_incremental_and_no_timestamps(idx):
    """delta_x_offsets / cache (one new last row per user; hstu.py:160-191, 318-336, 421-429) and all_timestamps=None
    (no relative bias at all, :205-206), both against the reference's outputs."""
    c = load_cases("research_layer.npz")[idx]
    model = _load_research_stack(c)
    n = int(c["n"])
    off = torch.from_numpy(c["offsets"]).to(DEV)
    ts = torch.from_numpy(c["ts"]).to(DEV)
    mask = 1.0 - torch.triu(torch.ones(n, n, device=DEV), diagonal=1)
    with torch.no_grad():
        x = torch.from_numpy(c["x"]).to(DEV)
        _, cache = model.jagged_forward(x=x, x_offsets=off, all_timestamps=ts, invalid_attn_mask=mask, return_cache_states=True)
        rows, cols = torch.from_numpy(c["delta_rows"]).to(DEV), torch.from_numpy(c["delta_cols"]).to(DEV)
        x2 = torch.from_numpy(c["x2"]).to(DEV)
        y2, cache2 = model.jagged_forward(x=x2, x_offsets=off, all_timestamps=ts, invalid_attn_mask=mask,
                                          delta_x_offsets=(rows, cols), cache=cache, return_cache_states=True)
        _close(y2, c["y2"], 1e-3, 1e-5, "incremental y")
        for li, (cv, cq, ck, co) in enumerate(cache2):
            _close(cv, c[f"cache2_{li}:v"], 1e-3, 1e-5, f"cache2_{li} v")
            _close(cq, c[f"cache2_{li}:q"], 1e-3, 1e-5, f"cache2_{li} padded q")
            _close(ck, c[f"cache2_{li}:k"], 1e-3, 1e-5, f"cache2_{li} padded k")
            _close(co, c[f"cache2_{li}:out"], 1e-3, 1e-5, f"cache2_{li} outputs")
        # the same rows through the full path on x2
        y_full, _ = model.jagged_forward(x=x2, x_offsets=off, all_timestamps=ts, invalid_attn_mask=mask)
        _close(y_full, c["y2_full"], 1e-3, 1e-5, "full y on the updated input")
        # a new row that is NOT the user's last one: keys / values are cut at its position.  Reference semantics by
        # construction: equal to the full path's output at that row when nothing after it changed.
        _, cache3 = model.jagged_forward(x=x2, x_offsets=off, all_timestamps=ts, invalid_attn_mask=mask, return_cache_states=True)
        mid_cols = torch.clamp(cols - 1, min=0)
        mid_rows = off[:-1] + mid_cols
        y3, _ = model.jagged_forward(x=x2, x_offsets=off, all_timestamps=ts, invalid_attn_mask=mask,
                                     delta_x_offsets=(mid_rows, mid_cols), cache=cache3)
        _close(y3[mid_rows], y_full[mid_rows].cpu().numpy(), 1e-3, 1e-5, "incremental y at an inner position")
        y_nb, _ = model.jagged_forward(x=x, x_offsets=off, all_timestamps=None, invalid_attn_mask=mask)
        _close(y_nb, c["y_nobias"], 1e-3, 1e-5, "y without timestamps")
    # gradients flow and the bias tables get none when there are no timestamps
    xg = x.clone().requires_grad_()
    yg, _ = model.jagged_forward(x=xg, x_offsets=off, all_timestamps=None, invalid_attn_mask=mask)
    yg.sum().backward()
    assert torch.isfinite(xg.grad).all()
    assert all(layer._rel_attn_bias._pos_w.grad is None and layer._rel_attn_bias._ts_w.grad is None for layer in model._attention_layers)


class _StubEmb(torch.nn.Module):          # the stand-in modules of tests/golden/make_golden.py::hstu_model_cases, restated
    item_embedding_dim = 32

    def __init__(self, n_items=50, dim=32):
        super().__init__()
        self._item_emb = torch.nn.Embedding(n_items, dim)

    def get_item_embeddings(self, ids):
        return self._item_emb(ids)


class _StubPre(torch.nn.Module):
    def __init__(self, n, dim):
        super().__init__()
        self._pos = torch.nn.Parameter(torch.zeros(n, dim))

    def forward(self, past_lengths, past_ids, past_embeddings, past_payloads):
        B, N, D = past_embeddings.shape
        x = past_embeddings * (D ** 0.5) + self._pos[:N].unsqueeze(0)
        valid = (past_ids != 0).unsqueeze(-1).to(x.dtype)
        return past_lengths, x * valid, valid


class _StubPost(torch.nn.Module):
    def forward(self, x):
        return x / torch.clamp(torch.linalg.norm(x, ord=None, dim=-1, keepdim=True), min=1e-6)


class _StubSim(torch.nn.Module):
    def forward(self, query_embeddings, item_embeddings, item_ids=None, **kw):
        return (query_embeddings.unsqueeze(1) * item_embeddings).sum(-1), {}


@pytest.mark.parametrize("idx", range(2))
def test_hstu_model_golden_forward_encode_backward(idx):
    """The top-level research model (research/modeling/sequential/hstu.py:543-809) against reference-minted vectors:
    ``forward`` (B, N, D), ``encode`` (B, D) and EVERY parameter gradient (embedding table, preprocessor, both layers incl.
    their bias tables) of a loss on both outputs; fp32."""
    m = _mods()
    c = load_cases("hstu_model.npz")[idx]
    N, out_len, D = int(c["N"]), int(c["out_len"]), int(c["D"])
    model = m.HSTU(max_sequence_len=N, max_output_len=out_len, embedding_dim=D, num_blocks=2, num_heads=int(c["H"]),
                   linear_dim=int(c["Ld"]), attention_dim=int(c["A"]), normalization="rel_bias", linear_config="uvqk",
                   linear_activation="silu", linear_dropout_rate=0.0, attn_dropout_rate=0.0, embedding_module=_StubEmb(50, D),
                   similarity_module=_StubSim(), input_features_preproc_module=_StubPre(N + out_len, D),
                   output_postproc_module=_StubPost(), concat_ua=bool(int(c["concat_ua"])), verbose=False)
    params = dict(model.named_parameters())
    names = sorted(k[2:] for k in c if k.startswith("p:"))
    assert sorted(params) == names, "parameter names = the reference's"
    with torch.no_grad():
        for k in names:
            params[k].copy_(torch.from_numpy(c["p:" + k]))
    model = model.to(DEV)
    lengths = torch.from_numpy(c["lengths"]).to(DEV)
    ids = torch.from_numpy(c["ids"]).to(DEV)
    ts = torch.from_numpy(c["ts"]).to(DEV)
    emb = model.get_item_embeddings(ids)
    y = model(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads={"timestamps": ts})
    cur = model.encode(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads={"timestamps": ts})
    _close(y, c["y"], 1e-3, 1e-5, "HSTU.forward")
    _close(cur, c["cur"], 1e-3, 1e-5, "HSTU.encode")
    ((y * torch.from_numpy(c["gy"]).to(DEV)).sum() + (cur * torch.from_numpy(c["gc"]).to(DEV)).sum()).backward()
    for name, prm in model.named_parameters():
        _close(prm.grad, c["g:" + name], 2e-3, 2e-5, "HSTU grad " + name)


def test_hstu_model_mirror_runs_with_duck_typed_modules():
    """HSTU (hstu.py:543-809): constructor arguments, state_dict names and the encode / forward methods, with stand-in
    embedding / preprocessor / postprocessor / similarity modules."""
    m = _mods()

    class Emb(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._item_emb = torch.nn.Embedding(50, 32)
        item_embedding_dim = 32
        def get_item_embeddings(self, ids):
            return self._item_emb(ids)

    class Pre(torch.nn.Module):
        def forward(self, past_lengths, past_ids, past_embeddings, past_payloads):
            return past_lengths, past_embeddings, None

    torch.manual_seed(0)
    model = m.HSTU(max_sequence_len=20, max_output_len=4, embedding_dim=32, num_blocks=2, num_heads=2, linear_dim=16,
                   attention_dim=16, normalization="rel_bias", linear_config="uvqk", linear_activation="silu",
                   linear_dropout_rate=0.0, attn_dropout_rate=0.0, embedding_module=Emb(),
                   similarity_module=lambda query_embeddings, item_embeddings, item_ids, **kw: (query_embeddings.unsqueeze(1) * item_embeddings).sum(-1),
                   input_features_preproc_module=Pre(), output_postproc_module=torch.nn.Identity(), verbose=False).to(DEV)
    keys = set(model.state_dict())
    assert {"_attn_mask", "_hstu._attention_layers.0._uvqk", "_hstu._attention_layers.1._o.weight",
            "_hstu._attention_layers.0._rel_attn_bias._ts_w", "_embedding_module._item_emb.weight"} <= keys
    assert model._hstu._attention_layers[0]._rel_attn_bias._pos_w.numel() == 2 * 24 - 1
    assert model.debug_str() == "HSTU-b2-h2-dqk16-dv16-lsilud0.0-ad0.0"
    B, N = 3, 24
    lengths = torch.tensor([24, 7, 13], device=DEV)
    ids = torch.randint(1, 50, (B, N), device=DEV)
    emb = model.get_item_embeddings(ids)
    ts = torch.sort(torch.randint(0, 10**7, (B, N), device=DEV), dim=1).values
    y = model(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads={"timestamps": ts})
    assert y.shape == (B, N, 32) and bool((y[1, 7:] == 0).all())
    cur = model.encode(past_lengths=lengths, past_ids=ids, past_embeddings=emb, past_payloads={"timestamps": ts})
    assert torch.equal(cur, torch.stack([y[b, int(lengths[b]) - 1] for b in range(B)]))
    sim = model.similarity_fn(cur, ids[:, :5])
    assert sim.shape == (B, 5)
    y.sum().backward()
    assert model._hstu._attention_layers[0]._uvqk.grad is not None
