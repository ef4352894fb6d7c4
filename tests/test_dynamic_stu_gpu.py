"""modules/dynamic_stu.py over real STU layers on the GPU: L2STU against the same composition done by hand (host-built row
index lists and plain torch indexing, not the package's split / concat ops), the reference test's nested L2STU scaled down,
SDSTU over a real stack (skip, no skip, eval), and a batch of zero rows straight through STUStack.

Everything is compared bit for bit: the rows L2STU hands its inner stack are the rows the hand composition hands it, so the
same kernels see the same bytes.  Gradients are required to be ``torch.equal`` as long as the hand composition itself repeats
bit for bit (it is run twice first); should it not, the gate is 4 x the largest difference between its two runs."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, H, A, HD = 64, 2, 32, 64


def _layers(n, target_aware=True, contextual=0):
    from generative_recommenders_amd.modules.stu import STULayer, STULayerConfig

    return [STULayer(STULayerConfig(embedding_dim=D, num_heads=H, hidden_dim=HD, attention_dim=A, output_dropout_ratio=0.0,
                                    causal=True, target_aware=target_aware, contextual_seq_len=contextual), is_inference=False)
            for _ in range(n)]


def _stack(n, dtype, **kw):
    from generative_recommenders_amd.modules.stu import STUStack

    return STUStack(_layers(n, **kw), is_inference=False).to(DEV).to(dtype).train()


def _offsets(lengths):
    from generative_recommenders_amd.ops.jagged_tensors import asynchronous_complete_cumsum

    return asynchronous_complete_cumsum(lengths)


def _index_lists(lengths, num_targets, max_l2_len, contextual):
    """per user [contextual rows | prefix rows | the rest]: the global row indices of the prefix and of the L2 part, and the
    L2 lengths (built on the host, independently of the package's offset arithmetic)"""
    prefix, l2, l2_lengths, base = [], [], [], 0
    for n, t in zip(lengths, num_targets):
        p = max(n - max_l2_len - t - contextual, 0)
        rows = list(range(base, base + n))
        l2 += rows[:contextual] + rows[contextual + p:]
        prefix += rows[contextual:contextual + p]
        l2_lengths.append(n - p)
        base += n
    return prefix, l2, l2_lengths


def _grads(out, inputs, dout):
    return torch.autograd.grad(out, inputs, dout, allow_unused=True)


def _same(a, b, tol, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    if tol == 0.0:
        assert torch.equal(a, b), f"{what}: max abs diff {(a.float() - b.float()).abs().max().item():.3e}"
    else:
        assert (a.float() - b.float()).abs().max().item() <= tol, what


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("target_aware", [False, True], ids=["no_targets", "targets"])
@pytest.mark.parametrize("contextual", [0, 3], ids=["ctx0", "ctx3"])
def test_l2stu_equals_the_hand_composition(contextual, target_aware, dtype):
    from generative_recommenders_amd.modules.dynamic_stu import L2STU

    max_l2_len = 8
    # lengths without the targets: shorter than the window, exactly the window (prefix 0), one more (prefix 1), 40,
    # contextual rows only, and -- without contextual rows -- a user of 0 rows
    base = [5, max_l2_len + contextual, max_l2_len + contextual + 1, 40, contextual] + ([0] if contextual == 0 else [])
    nt = [1, 2, 3, 1, 2, 3][: len(base)] if target_aware else [0] * len(base)
    lengths = [b + t for b, t in zip(base, nt)]
    stack = _stack(2, dtype, target_aware=target_aware, contextual=contextual)
    l2stu = L2STU(stack, max_l2_len=max_l2_len, is_inference=False, contextual_seq_len=contextual).train()
    params = [p for p in stack.parameters()]
    g = torch.Generator().manual_seed(11)
    total = sum(lengths)
    x = torch.randn(total, D, generator=g).to(dtype).to(DEV).requires_grad_()
    dout = torch.randn(total, D, generator=g).to(dtype).to(DEV)
    len_d = torch.tensor(lengths, device=DEV)
    nt_d = torch.tensor(nt, device=DEV)
    off_d = _offsets(len_d)
    prefix_idx, l2_idx, l2_lengths = _index_lists(lengths, nt, max_l2_len, contextual)
    assert prefix_idx and len(prefix_idx) == 1 + (40 - max_l2_len - contextual)
    pi, li = torch.tensor(prefix_idx, device=DEV), torch.tensor(l2_idx, device=DEV)

    def hand():
        l2_in = x.detach()[li].requires_grad_()
        l2_len = torch.tensor(l2_lengths, device=DEV)
        y = stack(x=l2_in, x_lengths=l2_len, x_offsets=_offsets(l2_len), max_seq_len=max(l2_lengths), num_targets=nt_d)
        return y.detach(), _grads(y, [l2_in] + params, dout[li])

    y1, g1 = hand()
    y2, g2 = hand()
    assert torch.equal(y1, y2)
    spread = max((a.float() - b.float()).abs().max().item() for a, b in zip(g1, g2) if a is not None)
    print(f"hand composition, two runs: largest gradient difference {spread:.3e}")
    tol = 4 * spread

    out = l2stu(x=x, x_lengths=len_d, x_offsets=off_d, max_seq_len=max(lengths), num_targets=nt_d)
    assert l2stu._saved_tensors is None
    assert l2stu._runtime_max_l2_len == max(l2_lengths) and l2stu._runtime_prefix_len == 40 - max_l2_len - contextual
    assert out.shape == x.shape and out.dtype == dtype
    assert torch.equal(out[pi], x.detach()[pi]), "prefix rows must pass through unchanged"
    assert torch.equal(out[li], y1), "L2 rows differ from the hand composition"
    grads = _grads(out, [x] + params, dout)
    assert torch.equal(grads[0][pi], dout[pi]), "prefix rows of x.grad must be dout's rows"
    _same(grads[0][li], g1[0], tol, "x.grad, L2 rows")
    for (name, _), a, b in zip(stack.named_parameters(), grads[1:], g1[1:]):
        assert a is not None
        _same(a, b, tol, name)


def test_nested_l2stu():
    """two plain layers, then L2STU(16) over [two layers, then L2STU(8) over two layers] (modules/tests/dynamic_stu_test.py,
    scaled down): runs forward and backward, and the rows outside the outer window are the first two layers' output"""
    from generative_recommenders_amd.modules.dynamic_stu import L2STU
    from generative_recommenders_amd.modules.stu import STUStack

    dtype = torch.bfloat16
    l3 = L2STU(STUStack(_layers(2), is_inference=False), max_l2_len=8, is_inference=False)
    l2 = L2STU(STUStack(_layers(2) + [l3], is_inference=False), max_l2_len=16, is_inference=False)
    first = _layers(2)
    stu = STUStack(first + [l2], is_inference=False).to(DEV).to(dtype).train()
    lengths = [40, 7, 0, 19, 31, 12]
    nt = [3, 1, 0, 2, 1, 2]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(sum(lengths), D, generator=g).to(dtype).to(DEV).requires_grad_()
    len_d, nt_d = torch.tensor(lengths, device=DEV), torch.tensor(nt, device=DEV)
    off_d = _offsets(len_d)
    out = stu(x=x, x_lengths=len_d, x_offsets=off_d, max_seq_len=40, num_targets=nt_d)
    assert out.shape == x.shape and bool(torch.isfinite(out.float()).all())
    out.backward(torch.randn(out.shape, generator=g).to(dtype).to(DEV))
    assert bool(torch.isfinite(x.grad.float()).all())
    for name, p in stu.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()), name
    assert l2._saved_tensors is None and l3._saved_tensors is None
    with torch.no_grad():
        two = STUStack(first, is_inference=False)(x=x.detach(), x_lengths=len_d, x_offsets=off_d, max_seq_len=40, num_targets=nt_d)
    prefix_idx, _, _ = _index_lists(lengths, nt, 16, 0)
    assert len(prefix_idx) == (40 - 19) + (19 - 18) + (31 - 17)
    pi = torch.tensor(prefix_idx, device=DEV)
    assert torch.equal(out.detach()[pi], two[pi])


def _sd_batch(dtype):
    lengths = [9, 0, 17, 4]
    nt = [1, 0, 2, 1]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(sum(lengths), D, generator=g).to(dtype).to(DEV).requires_grad_()
    dout = torch.randn(sum(lengths), D, generator=g).to(dtype).to(DEV)
    len_d = torch.tensor(lengths, device=DEV)
    return x, dout, dict(x_lengths=len_d, x_offsets=_offsets(len_d), max_seq_len=17, num_targets=torch.tensor(nt, device=DEV))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fuse", [True, False], ids=["one_node", "two_nodes"])
def test_sdstu_skip_over_a_real_stack(fuse, dtype):
    from generative_recommenders_amd.modules.dynamic_stu import SDSTU

    stack = _stack(2, dtype)
    stack.recursive_setattr("fuse_layer", fuse)
    sd = SDSTU(stack, is_inference=False, dropout_ratio=1.0, seed=3).train()
    x, dout, kw = _sd_batch(dtype)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    out = sd(x=x, **kw)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), dev_state)
    assert out is x and sd._iter == 1 and sd._skip_x is None
    out.backward(dout)
    assert torch.equal(x.grad, dout)
    assert all(p.grad is None for p in stack.parameters())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["train_ratio0", "eval_ratio1"])
def test_sdstu_without_a_skip_is_the_plain_stack(mode, dtype):
    from generative_recommenders_amd.modules.dynamic_stu import SDSTU

    stack = _stack(2, dtype)
    plain = copy.deepcopy(stack)
    sd = SDSTU(stack, is_inference=False, dropout_ratio=0.0 if mode == "train_ratio0" else 1.0, seed=3)
    sd.train(mode == "train_ratio0"), plain.train(mode == "train_ratio0")
    x, dout, kw = _sd_batch(dtype)
    x2 = x.detach().clone().requires_grad_()
    dev_state = torch.cuda.get_rng_state()
    out = sd(x=x, **kw)
    assert torch.equal(torch.cuda.get_rng_state(), dev_state)
    ref = plain(x=x2, **kw)
    assert torch.equal(out, ref)
    out.backward(dout), ref.backward(dout)
    assert torch.equal(x.grad, x2.grad)
    for (name, p), q in zip(stack.named_parameters(), plain.parameters()):
        assert torch.equal(p.grad, q.grad), name
    assert sd._iter == (1 if mode == "train_ratio0" else 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fuse", [True, False], ids=["one_node", "two_nodes"])
def test_empty_batch_through_the_stack(fuse, dtype):
    stack = _stack(2, dtype)
    stack.recursive_setattr("fuse_layer", fuse)
    fresh = copy.deepcopy(stack)
    x0 = torch.empty(0, D, dtype=dtype, device=DEV, requires_grad=True)
    zeros4 = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = stack(x=x0, x_lengths=zeros4, x_offsets=torch.zeros(5, dtype=torch.int64, device=DEV), max_seq_len=1, num_targets=zeros4)
    assert out.shape == (0, D) and out.dtype == dtype and out.is_cuda
    out.sum().backward()
    assert x0.grad is None or x0.grad.shape == (0, D)
    for name, p in stack.named_parameters():
        assert p.grad is None or not bool(p.grad.any()), name
    with torch.no_grad():                      # no graph either
        assert stack(x=x0.detach(), x_lengths=zeros4, x_offsets=torch.zeros(5, dtype=torch.int64, device=DEV), max_seq_len=1,
                     num_targets=zeros4).shape == (0, D)
    # the same stack on a non-empty batch afterwards: what a stack that never saw the empty one gives
    x, dout, kw = _sd_batch(dtype)
    x2 = x.detach().clone().requires_grad_()
    stack.zero_grad()
    a, b = stack(x=x, **kw), fresh(x=x2, **kw)
    assert torch.equal(a, b)
    a.backward(dout), b.backward(dout)
    assert torch.equal(x.grad, x2.grad)
    for (name, p), q in zip(stack.named_parameters(), fresh.parameters()):
        assert torch.equal(p.grad, q.grad), name
