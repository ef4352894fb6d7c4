"""GPU checks of the two launch-time decisions that left the attention kernels' prologues (docs/EXPERIMENTS.md R21):

* attn_scale by pointer: the device value is read by a scalar load in every launch -- same bits as the host scale when it
  holds 1/N, exactly doubled results when the caller doubles it between two launches (nothing is cached on the host);
* the fast-addressing predicate of the folded backward comes from the host (csrc/attn_dma_addr.h): a k whose rows lie
  2^24 bytes apart takes the 64-bit address path, forward and backward, and gives the bits of a compact k."""
import ctypes as C

import numpy as np
import pytest
import torch

from generative_recommenders_amd import _lib as L
from generative_recommenders_amd.ops import _launch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 200
LENGTHS = (1, 33, 200)


def _case(dtype, d, H, bias):
    """params + tensors of one forward / backward pair through the C ABI; `keep` holds everything the pointers refer to"""
    g = torch.Generator().manual_seed(1234 + d + H)
    off = torch.zeros(len(LENGTHS) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(LENGTHS), 0)
    Lt = int(off[-1])
    # Inputs in [0.5, 1): every term of every result is positive, so no element comes out near zero.  "Twice the scale gives
    # exactly twice the result" holds for the fp32 product (a power of two) and survives the rounding to 16 bits only for
    # NORMAL numbers: an f16 result below 2^-14 is rounded on the subnormals' fixed grid and its double on a finer one.
    # (The smallest results here, the one-row user's, are ~0.02; the largest ~5.)
    mk = lambda: (0.5 + 0.5 * torch.rand(Lt, H, d, generator=g)).to(dtype).to(DEV)
    q, k, v, do = mk(), mk(), mk(), mk()
    out, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    offd = off.to(DEV)
    bp = L.HstuAttnBwdParams()
    _launch._fill_attn_params(bp.fwd, q, k, v, out, offd, None, N, d ** -0.5, 1.0 / N, 0, 0, 0, 0)
    keep = [q, k, v, do, out, dq, dk, dv, offd]
    if bias:
        from generative_recommenders_amd.research.modeling.sequential import hstu as m

        rng = np.random.default_rng(7)
        mod = m.RelativeBucketedTimeAndPositionBasedBias(N, 128).to(DEV)
        with torch.no_grad():
            for prm in mod.parameters():
                prm.normal_(0, 0.05)
        pos_w, ts_w, num_buckets, bucket_div = mod.bias_params()
        pos32, ts32 = pos_w.detach().float().contiguous(), ts_w.detach().float().contiguous()
        tsd = torch.from_numpy(np.sort(rng.integers(0, 10 ** 7, size=(len(LENGTHS), N)), axis=1).astype(np.int64)).to(DEV)
        m._fill_bias(bp.fwd, pos32, ts32, tsd, num_buckets, bucket_div)
        dpos, dts = torch.zeros_like(pos32), torch.zeros_like(ts32)
        bp.dpos_w, bp.dts_w = dpos.data_ptr(), dts.data_ptr()
        keep += [pos32, ts32, tsd, dpos, dts]
    bp.dout, bp.dq, bp.dk, bp.dv = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    bp.do_row_stride, bp.do_head_stride = do.stride(0), do.stride(1)
    for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        setattr(bp, n + "_row_stride", t.stride(0))
        setattr(bp, n + "_head_stride", t.stride(1))
    bp.total_rows = Lt
    ws_bytes = L.lib().hstu_attn_bwd_workspace_bytes(C.byref(bp))
    if ws_bytes:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        bp.workspace = ws.data_ptr()
        keep.append(ws)
    return bp, (out, dq, dk, dv), keep


def _run(bp, results):
    for t in results:
        t.fill_(float("nan"))
    st = L.current_stream_ptr(results[0].device)
    L.check(L.lib().hstu_attn_fwd(C.byref(bp.fwd), st))
    L.check(L.lib().hstu_attn_bwd(C.byref(bp), st))
    torch.cuda.synchronize()
    return [t.clone() for t in results]


@pytest.mark.parametrize("dtype,d,bias,kernel", [
    (torch.bfloat16, 128, False, "hstu_attn_bwd_fold_kernel<bf16,128,128>"),
    (torch.float16, 128, False, "hstu_attn_bwd_fold_kernel<f16,128,128>"),
    (torch.bfloat16, 64, False, "hstu_attn_bwd_quad_kernel<bf16,64>"),
    (torch.bfloat16, 64, True, "hstu_attn_bwd_fold_bias_kernel<bf16,64>")])
def test_attn_scale_is_read_on_the_device_in_every_launch(dtype, d, bias, kernel):
    bp, results, keep = _case(dtype, d, 2, bias)
    buf = C.create_string_buffer(128)
    L.check(L.lib().hstu_attn_bwd_kernel_name(C.byref(bp), buf, 128))
    assert buf.value.decode() == kernel
    names = ("out", "dq", "dk", "dv")
    host = _run(bp, results)                       # attn_scale = NULL: the host's 1/N
    for n, t in zip(names, host):
        assert bool(torch.isfinite(t.float()).all()) and float(t.float().abs().max()) > 0, n
    scale = torch.full((1,), 1.0 / N, dtype=torch.float32, device=DEV)
    bp.fwd.attn_scale = scale.data_ptr()
    by_pointer = _run(bp, results)
    for n, a, b in zip(names, by_pointer, host):
        assert torch.equal(a, b), f"{n}: the device-side 1/N gives other bits than the host scale"
    scale.mul_(2.0)                                # rewritten on the device between two launches of the same parameters
    doubled = _run(bp, results)
    for n, a, b in zip(names, doubled, host):
        assert torch.equal(a, 2 * b), f"{n}: twice the device scale is not exactly twice the result"


def _strided_k(k):
    """the rows of k (L, 1, d) 2^24 bytes apart in ONE allocation (as_strided view), everything else as it was"""
    rows, _, d = k.shape
    step = (1 << 24) // k.element_size()
    store = torch.empty((rows - 1) * step + d, dtype=k.dtype, device=k.device)
    view = store.as_strided((rows, 1, d), (step, d, 1))
    view.copy_(k)
    assert view.stride(0) * view.element_size() == 1 << 24 and store.numel() * store.element_size() < 0.7 * 2 ** 30
    return view


@pytest.fixture(scope="module")
def slow_path_inputs():
    g = torch.Generator().manual_seed(99)
    rows, d = 40, 128
    mk = lambda s: (s * torch.randn(rows, 1, d, generator=g)).bfloat16().to(DEV)
    q, k, v, do = mk(0.3), mk(0.3), mk(0.3), mk(1.0)
    off = torch.tensor([0, rows], dtype=torch.int64, device=DEV)
    return q, k, v, do, off, _strided_k(k)


def test_forward_with_k_rows_16_mib_apart(slow_path_inputs):
    q, k, v, do, off, k_far = slow_path_inputs
    rows, d = q.shape[0], q.shape[2]
    ref = _launch.attn_fwd(q, k, v, off, None, rows, d ** -0.5, 1.0 / rows)
    got = _launch.attn_fwd(q, k_far, v, off, None, rows, d ** -0.5, 1.0 / rows)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref.float()).all()) and float(ref.float().abs().max()) > 0
    assert torch.equal(got, ref)


def test_backward_with_k_rows_16_mib_apart(slow_path_inputs):
    q, k, v, do, off, k_far = slow_path_inputs
    rows, d = q.shape[0], q.shape[2]
    assert _launch.attn_bwd_kernel_name(torch.bfloat16, d, d, rows) == "hstu_attn_bwd_fold_kernel<bf16,128,128>"
    ref = _launch.attn_bwd(do, q, k, v, off, None, rows, d ** -0.5, 1.0 / rows)
    dk = torch.empty_like(k)
    got = _launch.attn_bwd(do, q, k_far, v, off, None, rows, d ** -0.5, 1.0 / rows, dk=dk)
    torch.cuda.synchronize()
    for n, a, b in zip(("dq", "dk", "dv"), got, ref):
        assert bool(torch.isfinite(b.float()).all()) and float(b.float().abs().max()) > 0, n
        assert torch.equal(a, b), f"{n}: the 64-bit address path gives other bits than the compact layout"
