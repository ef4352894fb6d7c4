"""CPU tests of the in-backward sparse Adam and SGD: the fp64 reference helper against a hand-computed example and against
torch.optim.Adam / torch.optim.SGD, its bounds against an fp32 evaluation (inside) and three wrong forms of Adam (outside), the
refusals, the front door, the state-dict keys and round trip, and the entry points' argument checks.  No kernel is launched."""

import ctypes as C

import numpy as np
import pytest
import torch

import embedding_sparse_optim_ref as SR
from generative_recommenders_amd.modules.dlrm_hstu import (EmbeddingCollection, EmbeddingConfig, KeyedJaggedTensor,
                                                          apply_optimizer_in_backward)
from generative_recommenders_amd.ops import embedding as E


def _collection(item_dtype="FP32"):
    return EmbeddingCollection([EmbeddingConfig(10, 8, "item", ["a", "b"], data_type=item_dtype), EmbeddingConfig(6, 8, "user", ["c"])])


def _features():
    return KeyedJaggedTensor(["a", "b", "c"], torch.tensor([1, 2, 2, 2, 3, 5, 0]), torch.tensor([3, 2, 2]))


def test_reference_helper_against_a_hand_computed_three_row_example():
    w = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    m = np.array([[0.0, 0.0], [9.0, 9.0], [1.0, -1.0]])
    v = np.array([[0.0, 0.0], [9.0, 9.0], [4.0, 1.0]])
    idx = np.array([2, 0, 2])
    dout = np.array([[1.0, 3.0], [2.0, 0.0], [1.0, 1.0]])
    r = SR.sparse_sgd_ref(w, idx, dout, lr=0.5)
    assert r["rows"].tolist() == [0, 2]
    np.testing.assert_allclose(r["weight"], [[0.0, 2.0], [3.0, 4.0], [4.0, 4.0]], rtol=0, atol=1e-15)     # G = (2, 0) and (2, 4)
    u = 2.0 ** -24
    np.testing.assert_allclose(r["tol_weight"][1], 0.5 * 8 * u * np.array([2.0, 4.0]) + 4 * u * (np.array([5.0, 6.0]) + 0.5 * np.array([2.0, 4.0])),
                               rtol=1e-12)
    # Adam, b = (0.5, 0.75), step 1 -> t = 2: bc1 = 0.75, bc2 = 7 / 16.  Row 2: m = 0.5 (1, -1) + 0.5 (2, 4) = (1.5, 1.5);
    # v = 0.75 (4, 1) + 0.25 (4, 16) = (4, 4.75); row 0 from zero state: m = (1, 0), v = (1, 0) -> the second column does not move
    r = SR.sparse_adam_ref(w, m, v, idx, dout, lr=0.3, betas=(0.5, 0.75), eps=0.125, step=1)
    np.testing.assert_allclose(r["exp_avg"], [[1.0, 0.0], [9.0, 9.0], [1.5, 1.5]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(r["exp_avg_sq"], [[1.0, 0.0], [9.0, 9.0], [4.0, 4.75]], rtol=0, atol=1e-15)
    s = np.sqrt(7 / 16)
    want = [[1 - 0.4 * 1.0 / (1 / s + 0.125), 2.0], [3.0, 4.0], [5 - 0.4 * 1.5 / (2 / s + 0.125), 6 - 0.4 * 1.5 / (np.sqrt(4.75) / s + 0.125)]]
    np.testing.assert_allclose(r["weight"], want, rtol=0, atol=1e-15)
    # the bounds of row 2, column 0: k = 2, A = 2, G = 2
    tG = 4 * u * 2
    tm = 0.5 * tG + 4 * u * (0.5 * 1 + 0.5 * 2)
    tv = 0.25 * (2 * 2 * tG + tG * tG) + 6 * u * (0.75 * 4 + 0.25 * 4)
    den = 2 / s + 0.125
    tden = min(tv / 2, np.sqrt(tv)) / s + 4 * u * den
    np.testing.assert_allclose(r["tol_exp_avg"][1, 0], tm, rtol=1e-12)
    np.testing.assert_allclose(r["tol_exp_avg_sq"][1, 0], tv, rtol=1e-12)
    np.testing.assert_allclose(r["tol_weight"][1, 0], 0.4 * (tm / den + 1.5 * tden / den ** 2) + 8 * u * (5 + 0.4 * 1.5 / den), rtol=1e-12)
    assert r["tol_weight"][0, 1] == 8 * u * 2.0 and r["tol_exp_avg"][0, 1] == 0 and r["tol_exp_avg_sq"][0, 1] == 0     # zero gradient, zero state
    assert w[0, 0] == 1.0 and m[2, 0] == 1.0 and v[2, 0] == 4.0          # the inputs are not modified
    assert SR.worst(np.array([0.0, 1e-30]), np.array([0.0, 1.0])) == 1e-30 and SR.worst(np.array([1e-30]), np.array([0.0])) == float("inf")


def test_reference_helper_equals_torch_optimizers_in_fp64():
    rng = np.random.default_rng(0)
    rows, dim, lr, betas, eps = 7, 6, 1e-2, (0.9, 0.99), 1e-3
    # three steps that each touch every row: lazy equals dense
    w0 = rng.standard_normal((rows, dim))
    for name in ("Adam", "SGD"):
        p = torch.nn.Parameter(torch.tensor(w0))
        opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps) if name == "Adam" else torch.optim.SGD([p], lr=lr)
        w, m, v = w0, np.zeros((rows, dim)), np.zeros((rows, dim))
        for step in range(3):
            idx = np.concatenate([np.arange(rows), rng.integers(0, rows, 5)])
            dout = rng.standard_normal((len(idx), dim))
            grad = np.zeros((rows, dim))
            np.add.at(grad, idx, dout)
            p.grad = torch.tensor(grad)
            opt.step()
            if name == "Adam":
                r = SR.sparse_adam_ref(w, m, v, idx, dout, lr, betas, eps, step)
                w, m, v = r["weight"], r["exp_avg"], r["exp_avg_sq"]
                st = opt.state[p]
                np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=0, atol=1e-15)
                np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=0, atol=1e-15)
            else:
                w = SR.sparse_sgd_ref(w, idx, dout, lr)["weight"]
            np.testing.assert_allclose(w, p.detach().numpy(), rtol=0, atol=1e-14)
    # one step from zero state on a partly touched table: dense Adam leaves zero-state rows with a zero gradient in place
    idx = np.array([5, 1, 5, 3])
    dout = rng.standard_normal((4, dim))
    grad = np.zeros((rows, dim))
    np.add.at(grad, idx, dout)
    p = torch.nn.Parameter(torch.tensor(w0))
    p.grad = torch.tensor(grad)
    torch.optim.Adam([p], lr=lr, betas=betas, eps=eps).step()
    r = SR.sparse_adam_ref(w0, np.zeros((rows, dim)), np.zeros((rows, dim)), idx, dout, lr, betas, eps, 0)
    assert r["rows"].tolist() == [1, 3, 5]
    np.testing.assert_allclose(r["weight"], p.detach().numpy(), rtol=0, atol=1e-15)
    p = torch.nn.Parameter(torch.tensor(w0))
    p.grad = torch.tensor(grad)
    torch.optim.SGD([p], lr=lr).step()
    np.testing.assert_allclose(SR.sparse_sgd_ref(w0, idx, dout, lr)["weight"], p.detach().numpy(), rtol=0, atol=1e-15)


def _adam_fp32_shuffled(w, m, v, idx, dout, lr, betas, eps, step, rng):
    """the update evaluated in fp32 by numpy, the gradient rows added one by one in a shuffled order"""
    f = np.float32
    order = rng.permutation(len(idx))
    rows, inverse = np.unique(idx, return_inverse=True)
    G = np.zeros((len(rows), w.shape[1]), dtype=f)
    np.add.at(G, inverse[order], dout[order].astype(f))
    b1, b2 = f(betas[0]), f(betas[1])
    t = step + 1
    bc1, bc2 = f(1.0 - float(b1) ** t), f(1.0 - float(b2) ** t)
    m_new = b1 * m[rows] + (f(1) - b1) * G
    v_new = b2 * v[rows] + (f(1) - b2) * G * G
    w_new = w[rows] - (f(lr) / bc1) * m_new / (np.sqrt(v_new) / np.sqrt(bc2) + f(eps))
    assert w_new.dtype == m_new.dtype == v_new.dtype == f
    return rows, G, w_new, m_new, v_new


@pytest.mark.parametrize("n,dim,rows,kind,tag", SR.CASES)
def test_bounds_admit_an_fp32_evaluation_in_shuffled_order(n, dim, rows, kind, tag):
    idx, dout, w, m, v = SR.make_problem(n, dim, rows, kind, tag)
    lr, betas, eps, step = SR.f32(1e-3), (SR.f32(0.95), SR.f32(0.999)), SR.f32(1e-8), 6
    rng = np.random.default_rng(1)
    touched, G, w32, m32, v32 = _adam_fp32_shuffled(w, m, v, idx, dout, lr, betas, eps, step, rng)
    r = SR.sparse_adam_ref(w, m, v, idx, dout, lr, betas, eps, step)
    assert np.array_equal(touched, r["rows"])
    for got, key in ((w32, "weight"), (m32, "exp_avg"), (v32, "exp_avg_sq")):
        over = SR.worst(np.abs(got.astype(np.float64) - r[key][touched]), r["tol_" + key])
        assert over <= 1.0, (key, over)
    s = SR.sparse_sgd_ref(w, idx, dout, lr)
    w_sgd = w[touched] - np.float32(lr) * G
    assert SR.worst(np.abs(w_sgd.astype(np.float64) - s["weight"][touched]), s["tol_weight"]) <= 1.0


@pytest.mark.parametrize("n,dim,rows,kind,zero_state,step", SR.EPS_CASES)
def test_bounds_reject_the_wrong_forms_of_adam_where_eps_matters(n, dim, rows, kind, zero_state, step):
    idx, dout, w, m, v = SR.make_problem(n, dim, rows, kind, "bf16", zero_state)
    lr, betas, eps = SR.f32(1e-3), (SR.f32(0.95), SR.f32(0.999)), SR.f32(1e-2)
    r = SR.sparse_adam_ref(w, m, v, idx, dout, lr, betas, eps, step)
    touched, _, w32, _, _ = _adam_fp32_shuffled(w, m, v, idx, dout, lr, betas, eps, step, np.random.default_rng(2))
    assert SR.worst(np.abs(w32.astype(np.float64) - r["weight"][touched]), r["tol_weight"]) <= 1.0
    for variant in ("no_bias_correction", "sparse_adam_eps", "eps_under_sqrt"):
        wrong = SR.sparse_adam_ref(w, m, v, idx, dout, lr, betas, eps, step, variant=variant)
        over = SR.worst(np.abs(wrong["weight"][touched] - r["weight"][touched]), r["tol_weight"])
        assert over > 100.0, (variant, over)


def test_refusals_name_their_reason():
    for kwargs, match in (({"weight_decay": 1e-4}, "weight_decay"), ({"amsgrad": True}, "amsgrad"), ({"betas": (0.9, 1.0)}, "betas"),
                          ({"betas": (-0.1, 0.5)}, "betas"), ({"betas": (float("nan"), 0.5)}, "betas")):
        with pytest.raises((NotImplementedError, RuntimeError), match=match):
            apply_optimizer_in_backward(_collection(), "Adam", 0.1, **kwargs)
    with pytest.raises(NotImplementedError, match="momentum"):
        _collection().apply_optimizer_in_backward("SGD", 0.1, momentum=0.9)
    with pytest.raises(NotImplementedError, match="weight_decay"):
        _collection().apply_optimizer_in_backward("SGD", 0.1, weight_decay=0.1)
    with pytest.raises(NotImplementedError, match="weight_decay"):
        _collection().apply_optimizer_in_backward("RowWiseAdagrad", 0.1, weight_decay=0.1)
    with pytest.raises(ValueError, match="optimizer_name"):
        _collection().apply_optimizer_in_backward("LAMB", 0.1)
    with pytest.raises(KeyError):
        _collection().apply_optimizer_in_backward("Adam", 0.1, tables=["nope"])
    with pytest.raises(RuntimeError, match="betas"):
        E.SparseAdamConfig(0.1, betas=(1.0, 0.5))


def test_cpu_tensors_and_wrong_state_are_refused():
    w, z = torch.zeros(4, 8), torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.sparse_sgd_update_(w, torch.tensor([1]), torch.zeros(1, 8), 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.sparse_adam_update_(w, z, z.clone(), torch.tensor([1]), torch.zeros(1, 8), 0.1, (0.9, 0.999), 1e-8, 0)
    with pytest.raises(RuntimeError, match="betas"):
        E.sparse_adam_update_(w, z, z.clone(), torch.tensor([1]), torch.zeros(1, 8), 0.1, (0.9, 1.5), 1e-8, 0)
    with pytest.raises(RuntimeError, match="step"):
        E.sparse_adam_update_(w, z, z.clone(), torch.tensor([1]), torch.zeros(1, 8), 0.1, (0.9, 0.999), 1e-8, -1)
    ec = _collection()
    ec.apply_optimizer_in_backward("Adam", 0.1, tables=["item"])
    ec.apply_optimizer_in_backward("SGD", 0.1, tables=["user"])
    out = ec(_features())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sum(x.values().sum() for x in out.values()).backward()
    assert all(e.weight.grad is None for e in ec.embeddings.values())
    assert int(ec.fused_optimizer_state_dict()["item.step"]) == 0           # nothing was applied: nothing was counted


def test_wrong_state_shapes_dtypes_and_seeds_are_refused_before_any_launch(monkeypatch):
    """the argument checks of the update functions past the device check (which is patched out: the tensors live on the CPU
    and no check below lets the call reach the library)"""
    monkeypatch.setattr(E.L, "require_gpu_tensor", lambda t, name: None)
    idx, dout = torch.tensor([1]), torch.zeros(1, 8)
    w, z = torch.zeros(4, 8), torch.zeros(4, 8)
    adam = lambda w=w, m=z, v=z, seed=None, idx=idx, dout=dout: E.sparse_adam_update_(w, m, v, idx, dout, 0.1, (0.9, 0.999), 1e-8, 0, seed=seed)
    with pytest.raises(RuntimeError, match="exp_avg must be"):
        adam(m=torch.zeros(4))
    with pytest.raises(RuntimeError, match="exp_avg_sq must be"):
        adam(v=torch.zeros(4, 8, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="exp_avg must be"):
        adam(m=torch.zeros(8, 4).t())
    with pytest.raises(RuntimeError, match="needs a seed"):
        adam(w=torch.zeros(4, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="pass none"):
        adam(seed=3)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        adam(w=torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        adam(w=torch.zeros(4, 12, dtype=torch.float16), m=torch.zeros(4, 12), v=torch.zeros(4, 12), seed=1, dout=torch.zeros(1, 12))
    with pytest.raises(RuntimeError, match="idx \\(n\\) and dout"):
        adam(dout=torch.zeros(2, 8))
    with pytest.raises(RuntimeError, match="needs a seed"):
        E.sparse_sgd_update_(torch.zeros(4, 8, dtype=torch.float16), idx, dout, 0.1)
    with pytest.raises(RuntimeError, match="pass none"):
        E.sparse_sgd_update_(w, idx, dout, 0.1, seed=0)
    # a 16-bit table or an Adam table without its step counter
    out = E.gather_rows_fused(torch.zeros(4, 8, requires_grad=True), (z, z.clone()), idx, E.SparseAdamConfig(0.1))
    with pytest.raises(RuntimeError, match="needs its step counter"):
        out.sum().backward()
    out = E.gather_rows_fused(torch.zeros(4, 8, dtype=torch.bfloat16, requires_grad=True), None, idx, E.SparseSGDConfig(0.1))
    with pytest.raises(RuntimeError, match="needs its step counter"):
        out.sum().backward()


def test_rowwise_adagrad_through_the_front_door_configures_what_the_old_call_does():
    a, b = _collection("FP16"), _collection("FP16")
    a.apply_rowwise_adagrad_in_backward(lr=0.2, eps=1e-6, rows_dtype=torch.bfloat16, average=False, seed=9)
    b.apply_optimizer_in_backward("RowWiseAdagrad", 0.2, eps=1e-6, rows_dtype=torch.bfloat16, average=False, seed=9)
    assert list(a._fused) == list(b._fused)
    for t in a._fused:
        assert type(a._fused[t]) is type(b._fused[t]) is E.RowWiseAdagradConfig and vars(a._fused[t]) == vars(b._fused[t])
    assert [(n, x.shape, x.dtype) for n, x in a.named_buffers()] == [(n, x.shape, x.dtype) for n, x in b.named_buffers()]
    assert sorted(a.fused_optimizer_state_dict()) == sorted(b.fused_optimizer_state_dict()) == [
        "item.momentum1", "item.rounding_step", "user.momentum1"]


def test_state_dict_keys_mixed_optimizers_and_settings_per_table():
    ec = _collection("BF16")
    keys = sorted(ec.state_dict())
    ec.apply_optimizer_in_backward("Adam", 0.1, betas=(0.8, 0.9), eps=1e-6, tables=["item"], seed=5)
    ec.apply_optimizer_in_backward("SGD", 0.2, rows_dtype=torch.bfloat16, tables=["user"])
    assert sorted(ec.state_dict()) == keys == ["embeddings.item.weight", "embeddings.user.weight"]       # TorchRec's keys
    assert sorted(ec.fused_optimizer_state_dict()) == ["item.exp_avg", "item.exp_avg_sq", "item.step"]
    st = ec.fused_optimizer_state_dict()
    assert st["item.exp_avg"].shape == st["item.exp_avg_sq"].shape == (10, 8) and st["item.exp_avg"].dtype == torch.float32
    assert st["item.step"].dtype == torch.int64 and st["item.step"].device.type == "cpu" and int(st["item.step"]) == 0
    item, user = ec._fused["item"], ec._fused["user"]
    assert type(item) is E.SparseAdamConfig and (item.lr, item.betas, item.eps, item.seed) == (0.1, (0.8, 0.9), 1e-6, 5)
    assert type(user) is E.SparseSGDConfig and (user.lr, user.rows_dtype) == (0.2, torch.bfloat16)
    out = ec(_features())
    assert out["a"].values().dtype == torch.bfloat16 and out["c"].values().dtype == torch.bfloat16
    ec.set_learning_rate(0.5)
    assert item.lr == user.lr == 0.5
    # named again with the same optimizer: the settings are replaced, the state stays; with another one: the state is the new one's
    with torch.no_grad():
        st["item.exp_avg"].fill_(2.0)
    ec.apply_optimizer_in_backward("Adam", 0.3, tables=["item"])
    assert ec._fused["item"] is item and item.lr == 0.3 and item.betas == (0.9, 0.999) and float(st["item.exp_avg"][0, 0]) == 2.0
    ec.apply_optimizer_in_backward("RowWiseAdagrad", 0.3, tables=["item"])
    assert sorted(ec.fused_optimizer_state_dict()) == ["item.momentum1", "item.rounding_step"]
    ec.apply_optimizer_in_backward("SGD", 0.3, tables=["item"])
    assert sorted(ec.fused_optimizer_state_dict()) == ["item.rounding_step"]       # a 16-bit SGD table keeps its rounding step
    assert [n for n, _ in ec.named_buffers()] == ["_rounding_step_item"]


def test_fused_optimizer_state_dict_round_trips_adam_state():
    a, b = _collection("FP16"), _collection("FP16")
    for ec in (a, b):
        ec.apply_optimizer_in_backward("Adam", 0.1)
    state = a.fused_optimizer_state_dict()
    assert sorted(state) == ["item.exp_avg", "item.exp_avg_sq", "item.step", "user.exp_avg", "user.exp_avg_sq", "user.step"]
    with torch.no_grad():
        state["item.exp_avg"].copy_(torch.arange(80.0).reshape(10, 8))
        state["user.exp_avg_sq"].fill_(0.25)
        state["item.step"].fill_(7)
    b.load_fused_optimizer_state_dict({k: v.clone() for k, v in state.items()})
    for k, v in b.fused_optimizer_state_dict().items():
        assert torch.equal(v, state[k]), k
    assert int(b.fused_optimizer_state_dict()["item.step"]) == 7 and int(b.fused_optimizer_state_dict()["user.step"]) == 0
    with pytest.raises(KeyError):
        b.load_fused_optimizer_state_dict({"item.exp_avg": torch.zeros(10, 8)})


def test_entry_point_validation_without_gpu():
    import os

    from generative_recommenders_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    assert lib.hstu_abi_version() == 13
    buf = (C.c_char * 512)()
    a = (C.addressof(buf) + 255) & ~255
    F32, F16, BF16 = _lib.torch_dtype_code(torch.float32), _lib.torch_dtype_code(torch.float16), _lib.torch_dtype_code(torch.bfloat16)

    def adam(dout=a, n=0, dim=8, rows=4, w=a, wdt=F32, m=a, v=a, b1=0.9, b2=0.999, step=0, dt=BF16):
        return lib.hstu_embedding_sparse_adam(dout, a, n, dim, rows, w, wdt, m, v, 0.1, b1, b2, 1e-8, step, 0, a, 0, dt, None)

    def sgd(dout=a, n=0, dim=8, rows=4, w=a, wdt=F32, dt=BF16):
        return lib.hstu_embedding_sparse_sgd(dout, a, n, dim, rows, w, wdt, 0.1, 0, a, 0, dt, None)

    err = lib.hstu_last_error
    assert adam() == 0 and sgd() == 0                                      # n == 0: nothing to do
    for call in (adam, sgd):
        assert call(w=None) == -1 and b"non-NULL" in err()
        assert call(wdt=3) == -1 and b"weight_dtype" in err()
        assert call(dim=12) == -1 and b"16-byte" in err()
        assert call(dim=12, dt=F32, wdt=F16) == -1 and b"multiple of 8" in err()
        assert call(dim=4096) == -2 and b"rows of" in err()
        assert call(dim=1 << 30) == -2 and b"rows of" in err()             # dim * 4 would wrap to 0
        assert call(dim=2048, dt=F32) == 0                                 # fp32 rows of 8 KiB are taken by the same entry
        assert call(dim=2048, dt=F16, wdt=BF16) == 0
        assert call(dim=2056, dt=F32) == -2 and b"rows of" in err()
        assert call(dt=3) == -1 and b"dtype" in err()
        assert call(n=1 << 31) == -1 and b"n out of range" in err()
        assert call(n=4) == -1 and b"workspace too small" in err()
        assert call(dout=a + 4) == -1 and b"16-byte aligned" in err()
    assert adam(m=None) == -1 and b"exp_avg" in err()
    assert adam(v=a + 8) == -1 and b"16-byte aligned" in err()
    assert adam(b1=1.0) == -1 and b"beta" in err()
    assert adam(b2=-0.5) == -1 and b"beta" in err()
    assert adam(b1=float("nan")) == -1 and b"beta" in err()
    assert adam(step=-1) == -1 and b"step" in err()
