"""GPU tests of the timestamp postprocessor: hstu_time_features against the reference's features, the op and the module
against the reference-minted fixtures (tests/golden/timestamp_ln/) under the relative gate of the fused row passes
(e_hip <= m * e_ref, both relative Frobenius errors against the fp64 truth; m from multitask_ref.gate_multiplier), the fused
path against the composition on this package's ops, empty inputs, run-to-run identical reductions and strided inputs."""

import numpy as np
import pytest
import torch

import timestamp_ln_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = R.case_files()
CASE_TAGS = [(p, tag) for p in CASES for tag in R.load_case(p)["tags"] if tag != "f64"]


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _periods(c):
    p = np.asarray(c["periods"], dtype=np.float32)
    return _t(p[:, 0]).view(1, -1), _t(p[:, 1]).view(1, -1)


def _module(c, dtype=None):
    from generative_recommenders_amd.modules.postprocessors import TimestampLayerNormPostprocessor

    m = TimestampLayerNormPostprocessor(embedding_dim=c["x"].shape[1], time_duration_features=c["periods"], eps=c["eps"])
    sd = {k: torch.from_numpy(np.ascontiguousarray(c["sd:" + k])) for k in m.state_dict()}
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _op_args(c):
    """fp32 leaf parameters of one case, in the op's argument order"""
    p = {k: _t(c["params"][k]).requires_grad_() for k in R.PARAMS}
    return p


def _run_op(c, tag, fn, x=None):
    p = _op_args(c)
    x = (_t(c["x"], R.TORCH_DTYPES[tag]) if x is None else x).requires_grad_()
    pu, upp = _periods(c)
    out = fn(x, _t(c["timestamps"]), p[R.COMBINER_W], p["_time_feature_combiner.bias"], p["_layer_norm.weight"],
             p["_layer_norm.bias"], pu, upp, c["eps"])
    assert out.dtype == x.dtype and out.shape == x.shape
    (out.float() * _t(c["r"])).sum().backward()
    torch.cuda.synchronize()
    return R.results_of(c, out, x, p)


@pytest.mark.parametrize("path", CASES, ids=R.case_id)
def test_time_features_against_the_fixture(path):
    """bound 1e-4: the smallest bucket step of the fixtures is 2 * 3.14 / 365 = 0.017 in the angle, fp32 libm noise is ~1e-7
    -- two orders from each, so a timestamp in another bucket fails and cos / sin of another libm passes"""
    from generative_recommenders_amd.ops import _launch

    c = R.load_case(path)
    pu, upp = _periods(c)
    got = _launch.time_features(_t(c["timestamps"]), pu, upp)
    assert got.dtype == torch.float32 and got.shape == c["time_features"].shape
    diff = float(np.abs(got.cpu().numpy() - c["time_features"]).max())
    print(f"time_features {c['name']}: max abs difference {diff:.3e}")
    assert diff <= 1e-4


def test_time_features_of_many_timestamps():
    """one block's worth and a grid-stride's worth of rows against the numpy restatement: boundaries +-1, +-64, +128 around
    hour marks near 1.7e9, draws over [0, 2e9) and the four periods of the fixtures"""
    from generative_recommenders_amd.ops import _launch

    g = torch.Generator().manual_seed(5)
    k = torch.randint(470000, 490000, (3000,), generator=g) * 3600
    t = torch.cat([k + d for d in (-64, -1, 0, 1, 64, 128)] + [torch.randint(0, 2_000_000_000, (12001,), generator=g)])
    periods = [(3600, 24), (86400, 7), (86400, 365), (60, 60)]
    p = np.asarray(periods, dtype=np.float32)
    got = _launch.time_features(t.to(DEV), _t(p[:, 0]), _t(p[:, 1])).cpu().numpy()
    assert np.abs(got - R.time_features(t.numpy(), periods)).max() <= 1e-4


@pytest.mark.parametrize("path,tag", CASE_TAGS, ids=lambda v: R.case_id(v) if v.endswith(".npz") else v)
def test_op_against_the_fixture(path, tag):
    from generative_recommenders_amd.ops import _launch
    from generative_recommenders_amd.ops.timestamp_layer_norm import timestamp_layer_norm

    c = R.load_case(path)
    assert _launch.time_ln_supported(c["x"].shape[1], len(c["periods"]), R.TORCH_DTYPES[tag])      # the fused path, not the composition
    R.check_gate(c, tag, _run_op(c, tag, timestamp_layer_norm), "op")


@pytest.mark.parametrize("path,tag", CASE_TAGS, ids=lambda v: R.case_id(v) if v.endswith(".npz") else v)
def test_composition_against_the_fixture(path, tag):
    """the fallback (time features -> cat -> addmm -> layer_norm on this package's ops) passes the same gate: the fused path
    and the composition agree within it"""
    from generative_recommenders_amd.ops.timestamp_layer_norm import timestamp_layer_norm_composed

    c = R.load_case(path)
    R.check_gate(c, tag, _run_op(c, tag, timestamp_layer_norm_composed), "composition")


@pytest.mark.parametrize("path,tag", CASE_TAGS, ids=lambda v: R.case_id(v) if v.endswith(".npz") else v)
def test_module_against_the_fixture(path, tag):
    c = R.load_case(path)
    m = _module(c)
    x = _t(c["x"], R.TORCH_DTYPES[tag]).requires_grad_()
    out = m(seq_embeddings=x, seq_timestamps=_t(c["timestamps"]), seq_payloads={})
    assert out.dtype == x.dtype
    (out.float() * _t(c["r"])).sum().backward()
    R.check_gate(c, tag, R.results_of(c, out, x, dict(m.named_parameters())), "module")


def test_module_flattens_the_3d_input():
    c = R.load_case(CASES[0])
    m = _module(c)
    x, t = _t(c["x"][:22], torch.bfloat16), _t(c["timestamps"][:22])
    flat = m(seq_embeddings=x, seq_timestamps=t, seq_payloads={})
    cube = m(seq_embeddings=x.view(2, 11, -1), seq_timestamps=t.view(2, 11), seq_payloads={})
    assert cube.shape == (2, 11, x.shape[1]) and torch.equal(cube.view(22, -1), flat)


def test_more_than_four_periods_run_the_composition():
    from generative_recommenders_amd.modules.postprocessors import TimestampLayerNormPostprocessor
    from generative_recommenders_amd.ops import _launch

    periods = [(60, 60), (3600, 24), (86400, 7), (86400, 30), (86400, 365)]
    assert not _launch.time_ln_supported(40, 5, torch.float32) and _launch.time_ln_supported(40, 4, torch.float32)
    m = TimestampLayerNormPostprocessor(embedding_dim=40, time_duration_features=periods).to(DEV)
    c = R.load_case(CASES[0])
    x, t = _t(c["x"]).requires_grad_(), _t(c["timestamps"])
    out = m(seq_embeddings=x, seq_timestamps=t, seq_payloads={})
    out.sum().backward()
    # against torch on the restatement's features (fp32: summation order only)
    tf = _t(R.time_features(c["timestamps"], periods))
    ref = torch.nn.functional.layer_norm(torch.nn.functional.linear(torch.cat([x.detach(), tf], -1), m._time_feature_combiner.weight,
                                                                    m._time_feature_combiner.bias), [40], m._layer_norm.weight,
                                         m._layer_norm.bias, 1e-5)
    assert torch.allclose(out, ref, rtol=1e-4, atol=1e-4) and m._time_feature_combiner.weight.grad.shape == (40, 50)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_no_rows_give_an_empty_output_and_zero_gradients(dtype):
    c = R.load_case(CASES[0])
    m = _module(c)
    x = torch.empty(0, 40, dtype=dtype, device=DEV, requires_grad=True)
    out = m(seq_embeddings=x, seq_timestamps=torch.empty(0, dtype=torch.int64, device=DEV), seq_payloads={})
    assert out.shape == (0, 40) and out.dtype == dtype
    out.sum().backward()
    assert x.grad.shape == (0, 40)
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and float(p.grad.abs().max()) == 0.0, k


@pytest.mark.parametrize("path", [CASES[2], CASES[3], CASES[1]], ids=R.case_id)
def test_two_backward_calls_give_bit_identical_reductions(path):
    """more rows than one workgroup walks (the fixture's rows tiled to 3000): registers, LDS, partials and the finish kernel"""
    from generative_recommenders_amd.ops import _launch

    c = R.load_case(path)
    reps = -(-3000 // c["x"].shape[0])
    dt = torch.bfloat16 if "bf16" in c["tags"] else torch.float32
    z0, dy = _t(np.tile(c["x"], (reps, 1)), dt), _t(np.tile(c["r"], (reps, 1)), dt)
    t = _t(np.tile(c["timestamps"], reps))
    pu, upp = _periods(c)
    p = c["params"]
    dim = z0.shape[1]
    b, wt, g, h = _t(p["_time_feature_combiner.bias"]), _t(p[R.COMBINER_W][:, dim:].T), _t(p["_layer_norm.weight"]), _t(p["_layer_norm.bias"])
    _, mean, rstd = _launch.time_ln_fwd(z0, t, pu, upp, b, wt, g, h, 1e-5)
    first = _launch.time_ln_bwd(dy, z0, t, pu, upp, b, wt, g, mean, rstd)
    second = _launch.time_ln_bwd(dy, z0, t, pu, upp, b, wt, g, mean, rstd)
    for a, bb in zip(first, second):
        assert torch.isfinite(a.float()).all() and torch.equal(a, bb)


def test_finish_kernel_adds_the_partial_rows_in_the_documented_order():
    """The backward through the C ABI with a workspace this test owns: the workgroups' partial rows, read back from it and
    added in numpy fp32 in the finish kernel's order, give the returned column sums bit for bit.  150 rows = 38 workgroups of
    4 rows (below any grid cap): thread r < 6 adds three partial rows, the others two.  Partial row of dim 72, 2 periods:
    [dln_w 72 | dln_b 72 | db 72 | dwt 4 x 72] = 504 floats, the last block of 16 columns half full."""
    from generative_recommenders_amd import _lib as L
    from generative_recommenders_amd.ops import _launch

    rows, dim, nf = 150, 72, 4
    g = torch.Generator().manual_seed(72)
    z0, dy = torch.randn(rows, dim, generator=g).to(DEV), torch.randn(rows, dim, generator=g).to(DEV)
    t = torch.randint(0, 2_000_000_000, (rows,), generator=g).to(DEV)
    pu, upp = _t(np.asarray([3600, 86400], dtype=np.float32)), _t(np.asarray([24, 7], dtype=np.float32))
    b, wt = (0.1 * torch.randn(dim, generator=g)).to(DEV), (0.1 * torch.randn(nf, dim, generator=g)).to(DEV)
    lw, lb = (1 + 0.1 * torch.randn(dim, generator=g)).to(DEV), (0.1 * torch.randn(dim, generator=g)).to(DEV)
    _, mean, rstd = _launch.time_ln_fwd(z0, t, pu, upp, b, wt, lw, lb, 1e-5)
    lib = L.lib()
    nbytes = lib.hstu_time_ln_workspace_bytes(dim, nf // 2)
    nparts, pstride = -(-rows // 4), (3 + nf) * dim
    assert (nparts, pstride) == (38, 504) and nbytes >= nparts * pstride * 4
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    dz = torch.empty_like(z0)
    dln_w, dln_b, db = (torch.empty(dim, device=DEV) for _ in range(3))
    dwt = torch.empty(nf, dim, device=DEV)
    L.check(lib.hstu_time_ln_bwd(dy.data_ptr(), z0.data_ptr(), t.data_ptr(), pu.data_ptr(), upp.data_ptr(), nf // 2, b.data_ptr(),
                                 wt.data_ptr(), lw.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dz.data_ptr(), dln_w.data_ptr(),
                                 dln_b.data_ptr(), db.data_ptr(), dwt.data_ptr(), ws.data_ptr(), rows, dim,
                                 L.torch_dtype_code(torch.float32), L.current_stream_ptr(z0.device)))
    torch.cuda.synchronize()
    partial = ws[:nparts * pstride].view(nparts, pstride).cpu().numpy()
    assert np.isfinite(partial).all() and np.isnan(ws[nparts * pstride:].cpu().numpy()).all()     # exactly 38 partial rows
    shares = np.zeros((16, pstride), dtype=np.float32)
    for i in range(nparts):               # thread (r, cc): rows r, r + 16, .. in order into one running sum
        shares[i % 16] += partial[i]
    total = np.zeros(pstride, dtype=np.float32)
    for k in range(16):                   # then the 16 sums in index order
        total += shares[k]
    assert total.dtype == np.float32
    for name, got, lo, n in (("dln_w", dln_w, 0, dim), ("dln_b", dln_b, dim, dim), ("db", db, 2 * dim, dim), ("dwt", dwt, 3 * dim, nf * dim)):
        v = got.cpu().numpy().reshape(-1)
        assert v.size == n and np.count_nonzero(v) > 0, name
        assert np.array_equal(v.view(np.uint32), total[lo:lo + n].view(np.uint32)), name


def test_a_strided_input_is_handled():
    """x as a column slice of a wider buffer and as every other row: the same values as from a contiguous copy"""
    from generative_recommenders_amd.ops.timestamp_layer_norm import timestamp_layer_norm

    c = R.load_case(CASES[0])
    x = _t(c["x"], torch.bfloat16)
    wide = torch.full((23, 56), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:, 8:48] = x
    rows2 = torch.full((46, 40), float("nan"), dtype=torch.bfloat16, device=DEV)
    rows2[::2] = x
    want = _run_op(c, "bf16", timestamp_layer_norm)
    for view in (wide[:, 8:48], rows2[::2], wide[:, 8:48].detach()[:, :]):
        assert not view.is_contiguous()
        got = _run_op(c, "bf16", timestamp_layer_norm, x=view.detach())
        for k in R.result_names():
            assert np.array_equal(got[k], want[k]), k
