"""GPU parity and properties of the multitask prediction head (hstu_multitask_head_fwd / _bwd, ops/multitask.py,
modules/multitask_module.py).  Two references, neither read from the reference tree at run time:

* the reference-minted fixtures (tests/golden/multitask/): per tensor e_hip <= m * e_ref, e = relative Frobenius error
  against the fixture's fp64 truth (gate_multiplier of tests/multitask_ref.py); the measured ratios are printed and, when
  HSTU_PARITY_OUT names a directory, written to parity_multitask.json there;
* the fp64 restatement fed the same rounded inputs, for the shapes the fixtures do not reach.  Its bounds come from the
  number formats: everything the kernel returns in fp32 went through a chain of fp32 operations (unit round-off
  u = 2^-24, the two hardware transcendentals of the gate 1 ulp) and sums of n <= 4096 columns or rows, whose error grows
  like sqrt(n) u at worst: 64 * 2^-24 = 3.8e-6, taken as 4e-6.  dx is rounded once more to x's dtype: its unit round-off
  (2^-8 for bf16, 2^-11 for fp16) is added."""

import json
import os

import numpy as np
import pytest
import torch

import multitask_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_TOL = 4e-6
DX_ROUND = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPE_NAME = {torch.float32: "float32", torch.bfloat16: "bfloat16", torch.float16: "float16"}
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    out = os.environ.get("HSTU_PARITY_OUT")
    if _RATIOS and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_multitask.json"), "w") as f:
            json.dump(_RATIOS, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a kernel fault surfaces at the next synchronisation: end the session there instead of launching the remaining tests"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, no further tests are started: {e}", returncode=70)


def _launch_constants():
    from generative_recommenders_amd.ops import _launch

    return _launch.MULTITASK_MAX_BLOCKS, _launch.MULTITASK_ROWS_PER_BLOCK


def _prediction_fn(in_dim, num_tasks):
    from generative_recommenders_amd.ops.layer_norm import SwishLayerNorm

    return torch.nn.Sequential(torch.nn.Linear(in_dim, 512), SwishLayerNorm(512), torch.nn.Linear(512, num_tasks))


def _module(case, dtype, is_inference=False, prediction_fn=_prediction_fn):
    from generative_recommenders_amd.modules.multitask_module import DefaultMultitaskModule, MultitaskTaskType, TaskConfig

    configs = [TaskConfig(task_name=n, task_weight=1, task_type=MultitaskTaskType(t))
               for n, t in zip(case["task_names"], case["task_types"])]
    m = DefaultMultitaskModule(task_configs=configs, embedding_dim=case["u"].shape[1], prediction_fn=prediction_fn,
                               causal_multitask_weights=case["cmw"], is_inference=is_inference)
    m.set_training_dtype(dtype)
    return m.to(DEV)


def _supervision(case):
    labels = {n: torch.from_numpy(case["label:" + n]).to(DEV) for n in case["task_names"]}
    weights = {n: torch.from_numpy(case["weight:" + n]).to(DEV) for n in case["weighted_tasks"]}
    return labels, weights


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("path", R.case_files(), ids=lambda p: os.path.basename(p)[5:-4])
def test_module_against_the_reference_fixtures(path, dtype):
    c = R.load_case(path)
    tag = "f32" if dtype == torch.float32 else "bf16"
    m = _module(c, dtype)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c["params"].items()}, strict=True)
    u = torch.from_numpy(c["u"]).to(DEV, dtype).requires_grad_()
    i = torch.from_numpy(c["i"]).to(DEV, dtype).requires_grad_()
    labels, weights = _supervision(c)
    preds, mt_labels, mt_weights, losses = m(u, i, labels, weights)
    T, L = len(c["task_names"]), c["u"].shape[0]
    assert preds.shape == (T, L) and preds.dtype == dtype and losses.shape == (T,) and losses.dtype == torch.float32
    assert mt_labels.shape == (T, L) and torch.equal(mt_labels.cpu(), torch.from_numpy(c["labels_tl"]))
    assert mt_weights.shape == (T, L) and torch.equal(mt_weights.cpu(), torch.from_numpy(c["weights_tl"]))
    (losses.sum() + (preds * torch.from_numpy(c["r"]).to(DEV)).sum()).backward()
    got = dict(preds=preds, losses=losses, gu=u.grad, gi=i.grad)
    for k, p in m.named_parameters():
        got["gp:" + k] = p.grad
    bad = []
    for k in R.result_names():
        truth = c["f64:" + k]
        e_hip = R.rel_fro(got[k].detach().double().cpu().numpy(), truth)
        e_ref = R.rel_fro(c[f"{tag}:{k}"], truth)
        _RATIOS[f"{c['name']}/{DTYPE_NAME[dtype]}/{k}"] = dict(e_hip=e_hip, e_ref=e_ref, ratio=e_hip / e_ref)
        print(f"{c['name']} {tag} {k}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {e_hip / e_ref:.3f}")
        mult = R.gate_multiplier(DTYPE_NAME[dtype], truth.size)
        if not e_hip <= mult * e_ref:
            bad.append((k, e_hip, e_ref, mult))
    assert not bad, f"(tensor, e_hip, e_ref, m) with e_hip > m * e_ref: {bad}"


# ------------------------------------------------------------------------------------------------------------ op level
def _big_rows():
    blocks, per_block = _launch_constants()
    return blocks * per_block + 37


TASKS = [(1, 0), (0, 1), (3, 0), (0, 2), (3, 2), (5, 3)]      # (binary, regression): 1 binary, 1 regression, 3+0, 0+2, 3+2, 8
# (dtype, dim, tasks, rows, column offset of x inside a wider buffer or None for a contiguous x, weights given)
OP_CASES = [
    (torch.bfloat16, 64, TASKS[0], 1, None, True), (torch.float16, 64, TASKS[1], 37, 8, False), (torch.float32, 64, TASKS[2], "big", None, True),
    (torch.bfloat16, 512, TASKS[4], "big", None, True), (torch.float16, 512, TASKS[5], 1000, None, True), (torch.float32, 512, TASKS[3], 37, 4, True),
    (torch.bfloat16, 512, TASKS[5], 1000, 16, False), (torch.bfloat16, 512, TASKS[1], 37, None, True), (torch.bfloat16, 512, TASKS[2], 1, None, True),
    (torch.bfloat16, 520, TASKS[3], 1000, None, True), (torch.float16, 520, TASKS[4], "big", 8, True), (torch.float32, 520, TASKS[0], 1, None, False),
    (torch.bfloat16, 4096, TASKS[5], 37, None, True), (torch.float16, 4096, TASKS[2], 1000, None, True), (torch.float32, 4096, TASKS[4], 37, None, True),
    (torch.float32, 4096, TASKS[1], 1, 4, True),
    # rows that start off a 16-byte boundary are read element by element: one column group, several, the widest
    (torch.bfloat16, 64, TASKS[4], 37, 1, True), (torch.float16, 520, TASKS[5], "big", 3, True), (torch.bfloat16, 2048, TASKS[3], 37, 1, True),
    (torch.float32, 517, TASKS[0], 1000, None, True),
]


def _op_id(c):
    dtype, dim, (nb, nr), rows, off, wts = c
    return f"{DTYPE_NAME[dtype]}-d{dim}-t{nb}+{nr}-r{rows}" + (f"-off{off}" if off is not None else "") + ("" if wts else "-now")


def _op_inputs(dtype, dim, tasks, rows, off, with_weights, seed=0):
    nb, nr = tasks
    T = nb + nr
    g = torch.Generator().manual_seed(1000 * dim + 10 * T + seed)
    rnd = lambda t: t.to(dtype).to(torch.float32)
    x = rnd(torch.randn(rows, dim, generator=g))
    lw, lb = rnd(1 + 0.1 * torch.randn(dim, generator=g)), rnd(0.1 * torch.randn(dim, generator=g))
    w, cb = torch.randn(T, dim, generator=g) / dim ** 0.5, 0.1 * torch.randn(T, generator=g)
    labels = torch.cat([torch.randint(0, 11, (nb, rows), generator=g).float(), torch.randn(nr, rows, generator=g)], 0)
    weights = 2 * torch.rand(T, rows, generator=g) if with_weights else None
    r = torch.randn(T, rows, generator=g)
    if off is None:
        xd = x.to(DEV, dtype)
    else:
        buf = torch.zeros(rows, dim + off + 24, dtype=dtype, device=DEV)
        xd = buf[:, off:off + dim]
        xd.copy_(x)
    return dict(x=x, lw=lw, lb=lb, w=w, c=cb, labels=labels, weights=weights, r=r, xd=xd, nb=nb, T=T)


def _run_op(inp, dtype, scale=0.3, labels=True, through=("preds", "losses")):
    from generative_recommenders_amd.ops.multitask import multitask_head

    leaf = lambda t: t.to(DEV, torch.float32).requires_grad_()
    xd = inp["xd"].detach().requires_grad_()
    # the norm's parameters are fp32 masters holding values of x's dtype (the launch layer's cast is exact): fp32 gradients
    lw, lb, w, c = leaf(inp["lw"]), leaf(inp["lb"]), leaf(inp["w"]), leaf(inp["c"])
    lab = inp["labels"].to(DEV) if labels else None
    wts = inp["weights"].to(DEV) if (labels and inp["weights"] is not None) else None
    preds, losses = multitask_head(xd, lw, lb, 1e-5, w, c, lab, wts, inp["nb"], scale)
    obj = 0.0
    if "losses" in through and losses is not None:
        obj = obj + losses.sum()
    if "preds" in through:
        obj = obj + (preds * inp["r"].to(DEV)).sum()
    obj.backward()
    return dict(preds=preds.detach(), losses=None if losses is None else losses.detach(), dx=xd.grad, dg=lw.grad, db=lb.grad,
                dw=w.grad, dc=c.grad)


@pytest.mark.parametrize("case", OP_CASES, ids=_op_id)
def test_op_against_the_restatement(case):
    dtype, dim, tasks, rows, off, with_weights = case
    if rows == "big":
        blocks, per_block = _launch_constants()
        rows = _big_rows()
        assert rows > blocks * per_block      # more rows than the largest grid works on at once: every workgroup loops
    inp = _op_inputs(dtype, dim, tasks, rows, off, with_weights)
    if off is not None:
        assert inp["xd"].stride(0) > dim and (rows == 1 or not inp["xd"].is_contiguous())
    got = _run_op(inp, dtype)
    ref = R.head_fp64(inp["x"], inp["lw"], inp["lb"], 1e-5, inp["w"], inp["c"], inp["labels"], inp["weights"], inp["nb"], 0.3, r=inp["r"])
    assert got["preds"].shape == (inp["T"], rows) and got["preds"].dtype == torch.float32 and got["dx"].dtype == dtype
    assert got["dx"].shape == (rows, dim) and got["dw"].shape == (inp["T"], dim)
    bad = []
    for k in ("preds", "losses") + R.HEAD_GRADS:
        g = got[k].double().cpu().numpy()
        assert np.isfinite(g).all(), k
        e = R.rel_fro(g, ref[k])
        tol = F32_TOL + (DX_ROUND[dtype] if k == "dx" else 0.0)
        print(f"{_op_id(case)} {k}: rel_fro {e:.3e} (bound {tol:.3e})")
        if not e <= tol:
            bad.append((k, e, tol))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ properties
def test_two_runs_are_bit_identical():
    inp = _op_inputs(torch.bfloat16, 512, (3, 2), _big_rows(), None, True)
    a, b = _run_op(inp, torch.bfloat16), _run_op(inp, torch.bfloat16)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    inp = _op_inputs(torch.float32, 520, (5, 3), 1000, None, True)     # the wide rows' two backward kernels
    a, b = _run_op(inp, torch.float32), _run_op(inp, torch.float32)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_finish_kernel_adds_the_partial_rows_in_the_documented_order():
    """The backward through the C ABI with a workspace this test owns: the workgroups' partial rows, read back from it and
    added in numpy fp32 in the finish kernel's order, give the returned gradients bit for bit.  150 rows = 38 workgroups of 4
    rows (below any grid cap): thread r < 6 adds three partial rows, the others two.  Partial row of dim 72, 3 tasks:
    [dW 216 | dg 72 | db 72 | dc 3 | 5 unused] = 368 floats, dc ends inside the last block of 16 columns."""
    from generative_recommenders_amd import _lib as L
    from generative_recommenders_amd.ops import _launch

    rows, dim, nb, T = 150, 72, 2, 3
    inp = _op_inputs(torch.float32, dim, (nb, T - nb), rows, None, True)
    x, lw, lb, w = inp["xd"], inp["lw"].to(DEV), inp["lb"].to(DEV), inp["w"].to(DEV)
    labels, weights, r = inp["labels"].to(DEV), inp["weights"].to(DEV), inp["r"].to(DEV)
    logits, _, mean, rstd, _, wsum = _launch.multitask_head_fwd(x, lw, lb, 1e-5, w, inp["c"].to(DEV), labels, weights, nb, 0.3)
    grad_loss = torch.linspace(0.5, 1.5, T, device=DEV)
    lib = L.lib()
    nbytes = lib.hstu_multitask_head_workspace_bytes(dim, T)
    nparts, pstride = -(-rows // 4), (T + 2) * dim + 8
    assert (nparts, pstride) == (38, 368) and nbytes >= nparts * pstride * 4
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    dx = torch.empty_like(x)
    dw, dc = torch.empty(T, dim, device=DEV), torch.empty(T, device=DEV)
    dg, db = torch.empty(dim, device=DEV), torch.empty(dim, device=DEV)
    L.check(lib.hstu_multitask_head_bwd(grad_loss.data_ptr(), r.data_ptr(), x.data_ptr(), x.stride(0), lw.data_ptr(), lb.data_ptr(),
                                        w.data_ptr(), labels.data_ptr(), weights.data_ptr(), logits.data_ptr(), mean.data_ptr(),
                                        rstd.data_ptr(), wsum.data_ptr(), dx.data_ptr(), dx.stride(0), dw.data_ptr(), dc.data_ptr(),
                                        dg.data_ptr(), db.data_ptr(), ws.data_ptr(), rows, dim, T, nb, 0.3,
                                        L.torch_dtype_code(torch.float32), L.current_stream_ptr(x.device)))
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
    for name, got, lo, n in (("dw", dw, 0, T * dim), ("dg", dg, T * dim, dim), ("db", db, (T + 1) * dim, dim), ("dc", dc, (T + 2) * dim, T)):
        g = got.cpu().numpy().reshape(-1)
        assert g.size == n and np.count_nonzero(g) > 0, name
        assert np.array_equal(g.view(np.uint32), total[lo:lo + n].view(np.uint32)), name


def test_no_rows_gives_zero_losses_and_zero_gradients():
    inp = _op_inputs(torch.bfloat16, 512, (3, 2), 0, None, True)
    got = _run_op(inp, torch.bfloat16)
    assert got["preds"].shape == (5, 0) and got["dx"].shape == (0, 512)
    assert torch.equal(got["losses"], torch.zeros(5, device=DEV))
    for k in ("dg", "db", "dw", "dc"):
        assert got[k] is not None and torch.count_nonzero(got[k]) == 0, k


def test_inference_form():
    from generative_recommenders_amd.ops.multitask import multitask_head

    inp = _op_inputs(torch.bfloat16, 512, (3, 2), 1000, None, True)
    train = _run_op(inp, torch.bfloat16)
    with torch.no_grad():
        preds, losses = multitask_head(inp["xd"], inp["lw"].to(DEV), inp["lb"].to(DEV), 1e-5, inp["w"].to(DEV), inp["c"].to(DEV),
                                       None, None, 3, 0.3)
    assert losses is None and torch.equal(preds, train["preds"])
    grads = _run_op(inp, torch.bfloat16, labels=False, through=("preds",))       # gradients still flow from the predictions
    only_preds = _run_op(inp, torch.bfloat16, through=("preds",))
    for k in R.HEAD_GRADS:
        assert torch.equal(grads[k], only_preds[k]), k
    c = R.load_case(R.case_files()[5])
    m = _module(c, torch.float32, is_inference=True)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c["params"].items()}, strict=True)
    u, i = torch.from_numpy(c["u"]).to(DEV), torch.from_numpy(c["i"]).to(DEV)
    with torch.no_grad():
        out = m(u, i, {}, {})
    assert out[1] is None and out[2] is None and out[3] is None and out[0].shape == (5, 200)
    assert R.rel_fro(out[0].double().cpu().numpy(), c["f64:preds"]) <= R.gate_multiplier("float32", 1000) * R.rel_fro(c["f32:preds"], c["f64:preds"])


def test_gradients_through_predictions_and_losses_add_up():
    """fp32 rows: the two partial gradients and the combined one are three results of the same fp32 chain, so their
    mismatch stays within three times its bound"""
    inp = _op_inputs(torch.float32, 512, (3, 2), 1000, None, True)
    both = _run_op(inp, torch.float32)
    p_only, l_only = _run_op(inp, torch.float32, through=("preds",)), _run_op(inp, torch.float32, through=("losses",))
    for k in R.HEAD_GRADS:
        e = R.rel_fro((p_only[k].double() + l_only[k].double()).cpu().numpy(), both[k].double().cpu().numpy())
        assert e <= 3 * F32_TOL, (k, e)
        assert torch.count_nonzero(l_only[k]) > 0 and torch.count_nonzero(p_only[k]) > 0, k


def test_all_zero_weights_give_a_zero_loss_and_no_loss_gradient():
    inp = _op_inputs(torch.bfloat16, 512, (3, 2), 1000, None, True)
    inp["weights"][1] = 0.0       # a binary task ...
    inp["weights"][4] = 0.0       # ... and a regression task
    got = _run_op(inp, torch.bfloat16, through=("losses",))
    assert got["losses"][1] == 0.0 and got["losses"][4] == 0.0 and torch.all(got["losses"][[0, 2, 3]] > 0)
    assert torch.count_nonzero(got["dw"][[1, 4]]) == 0 and torch.count_nonzero(got["dc"][[1, 4]]) == 0
    assert torch.count_nonzero(got["dw"][[0, 2, 3]]) > 0 and torch.all(got["dc"][[0, 2, 3]] != 0)


# ------------------------------------------------------------------------------------------------------------ fallback
def test_single_linear_prediction_module_takes_the_torch_path():
    c = R.load_case(R.case_files()[5])
    m = _module(c, torch.float32, prediction_fn=lambda in_dim, num_tasks: torch.nn.Linear(in_dim, num_tasks))
    assert m._fused_layers(torch.zeros(4, 64, device=DEV)) is None
    u, i = torch.from_numpy(c["u"]).to(DEV), torch.from_numpy(c["i"]).to(DEV)
    labels, weights = _supervision(c)
    preds, mt_labels, mt_weights, losses = m(u, i, labels, weights)
    rp, rl = R.single_linear_fp64(c["u"], c["i"], m._prediction_module.weight, m._prediction_module.bias, c["labels_tl"], c["weights_tl"],
                                  c["num_binary"], c["cmw"])
    assert preds.shape == (5, 200) and torch.equal(mt_weights.cpu(), torch.from_numpy(c["weights_tl"]))
    assert R.rel_fro(preds.detach().double().cpu().numpy(), rp) <= F32_TOL
    assert R.rel_fro(losses.detach().double().cpu().numpy(), rl) <= F32_TOL
    assert losses[1] == 0.0       # the all-zero-weights task of this fixture
