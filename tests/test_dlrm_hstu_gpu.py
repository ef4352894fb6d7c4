"""GPU tests of DlrmHSTU against the fixtures minted from the reference model (tests/golden/dlrm_hstu/): main_forward and
forward through the local feature container, with the gradients of the summed losses for every parameter (the embedding
tables included), in fp32 and bf16 under the relative gate of the fused row passes (e_hip <= m * e_ref, both relative
Frobenius errors against the fp64 truth; m from multitask_ref.gate_multiplier); the inference forward; the transducer with
the timestamp postprocessor over full embeddings; run-to-run identical table gradients; one training step."""

import numpy as np
import pytest
import torch

import dlrm_hstu_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": (torch.float32, "float32"), "bf16": (torch.bfloat16, "bfloat16")}


@pytest.fixture(autouse=True)
def _time_bucket_clamp_of_the_fixture(monkeypatch):
    """the fixtures are minted from the reference's PyTorch path, which clamps the positional encoder's time bucket to the
    embedding dim - 1 (ops/position.py: TIME_BUCKET_CLAMP); the package default is the GPU path's"""
    from generative_recommenders_amd.ops import position

    monkeypatch.setattr(position, "TIME_BUCKET_CLAMP", "pytorch_path")


@pytest.fixture(scope="module")
def inputs():
    return R.load("model_small")


@pytest.fixture(scope="module")
def truth():
    return R.load("model_small_f64")


def _model(inputs, tag, is_inference=False):
    dt = DTYPES[tag][0]
    m = R.build(is_inference, inputs).to(DEV).to(dt)
    m.set_training_dtype(dt)
    return m


def _np(t):
    return t.detach().double().cpu().numpy()


def _train_results(m, out):
    user, item, aux, preds, labels, weights = out
    names = [n for n, _, _ in R.TASKS]
    assert list(aux) == names
    torch.stack([aux[n] for n in names]).sum().backward()
    torch.cuda.synchronize()
    res = dict(user_embeddings=_np(user), item_embeddings=_np(item), preds=_np(preds), labels=_np(labels), weights=_np(weights),
               losses=_np(torch.stack([aux[n] for n in names])))
    for k, p in m.named_parameters():
        res["gp:" + k] = _np(p.grad) if p.grad is not None else np.zeros(tuple(p.shape))
    return res


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_main_forward_and_forward_against_the_fixture(inputs, truth, tag):
    ref = R.load("model_small_" + tag)
    gated = [str(k) for k in inputs["gated"]]
    m = _model(inputs, tag)
    uih, cand = R.features(inputs, DEV)
    got = _train_results(m, m.main_forward(*m.preprocess(uih_features=uih, candidates_features=cand)))
    assert np.array_equal(got["labels"], truth["labels"]) and np.array_equal(got["weights"], truth["weights"])
    m2 = _model(inputs, tag)
    again = _train_results(m2, m2(uih_features=uih, candidates_features=cand))
    for k in gated:       # forward is preprocess + main_forward, and every kernel on the way is deterministic
        assert np.array_equal(got[k], again[k]), k
    R.check_gate(gated, got, ref, truth, DTYPES[tag][1], "model")


def test_inference_forward_against_the_fixture(inputs):
    ref, truth = R.load("model_small_f32_infer"), R.load("model_small_f64_infer")
    m = _model(inputs, "f32", is_inference=True).eval()
    uih, cand = R.features(inputs, DEV)
    with torch.no_grad():
        user, item, aux, preds, labels, weights = m(uih_features=uih, candidates_features=cand)
    assert aux == {} and labels is None and weights is None
    got = dict(user_embeddings=_np(user), item_embeddings=_np(item), preds=_np(preds))
    R.check_gate(list(got), got, ref, truth, "float32", "inference")


def test_transducer_with_the_timestamp_postprocessor_over_full_embeddings(inputs, truth):
    """return_full_embeddings=True: the postprocessor runs on every row of the batch and the candidates are split off its
    output -- per row the same arithmetic, so the candidates pass the gate of the fixture's candidate embeddings"""
    from generative_recommenders_amd.modules.postprocessors import TimestampLayerNormPostprocessor

    ref = R.load("model_small_f32")
    m = _model(inputs, "f32")
    t = m._hstu_transducer
    assert isinstance(t._output_postprocessor, TimestampLayerNormPostprocessor)
    t._return_full_embeddings = True
    seen = {}
    inner = t.forward

    def spy(**kw):
        seen["cand"], seen["full"] = inner(**kw)
        return seen["cand"], seen["full"]

    t.forward = spy
    uih, cand = R.features(inputs, DEV)
    user = m(uih_features=uih, candidates_features=cand)[0]
    rows = sum(R.UIH_LENGTHS) + sum(R.CANDIDATES) + len(R.UIH_LENGTHS)        # + one contextual row per user
    assert seen["full"] is not None and seen["full"].shape == (rows, 32) and bool(torch.isfinite(seen["full"]).all())
    got = dict(user_embeddings=_np(user))
    R.check_gate(["user_embeddings"], got, ref, truth, "float32", "transducer(full)")


def test_table_gradients_are_bit_identical_across_two_runs(inputs):
    uih, cand = R.features(inputs, DEV)
    grads = []
    for _ in range(2):
        m = _model(inputs, "bf16")
        _, _, aux, _, _, _ = m(uih_features=uih, candidates_features=cand)
        sum(aux.values()).backward()
        grads.append({k: p.grad.clone() for k, p in m._embedding_collection.named_parameters()})
    assert sorted(grads[0]) == ["embeddings.item_id.weight", "embeddings.user_id.weight"]
    for k in grads[0]:
        assert float(grads[0][k].float().abs().max()) > 0.0 and torch.equal(grads[0][k], grads[1][k]), k


def test_default_configuration_trains_one_step():
    """DlrmHSTU(DlrmHSTUConfig(...), tables, is_inference) with the default postprocessor settings, from this package alone"""
    inputs = R.load("model_small")
    m = R.build(False).to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    uih, cand = R.features(inputs, DEV)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    _, _, aux, preds, _, _ = m(uih_features=uih, candidates_features=cand)
    loss = sum(aux.values())
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss)) and preds.shape == (3, sum(R.CANDIDATES))
    moved = [k for k, p in m.named_parameters() if not torch.equal(p.detach(), before[k])]
    assert "_hstu_transducer._output_postprocessor._time_feature_combiner.weight" in moved
    assert "_embedding_collection.embeddings.item_id.weight" in moved
