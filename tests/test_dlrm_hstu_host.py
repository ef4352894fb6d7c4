"""CPU checks of DlrmHSTU's drop-in surface: state-dict keys, config fields and defaults, constructor and method signatures
against the names recorded from the reference (tests/golden/dlrm_hstu/reference_names.npz), construction without torchrec,
and the local stand-ins for TorchRec's feature container and embedding collection."""

import dataclasses
import inspect
import sys

import numpy as np
import torch

import dlrm_hstu_ref as R


def test_state_dict_keys_and_config_defaults_equal_the_reference():
    from generative_recommenders_amd.modules import dlrm_hstu as M

    names = R.load_names()
    m = R.build(is_inference=False)
    assert list(m.state_dict()) == names["state_dict_keys"]
    fields = dataclasses.fields(M.DlrmHSTUConfig)
    assert [f.name for f in fields] == names["config_fields"]
    cfg = M.DlrmHSTUConfig()
    assert [repr(getattr(cfg, f.name)) for f in fields] == names["config_defaults"]
    assert cfg.enable_postprocessor and not cfg.use_layer_norm_postprocessor
    assert list(inspect.signature(M.DlrmHSTU.__init__).parameters) == names["init_args"]
    methods = ("_construct_payload", "_user_forward", "_item_forward", "preprocess", "main_forward", "forward")
    assert [f"{n}({', '.join(inspect.signature(getattr(M.DlrmHSTU, n)).parameters)})" for n in methods] == names["methods"]
    assert M.SequenceEmbedding._fields == ("lengths", "embedding")


def test_construction_on_cpu_without_torchrec():
    from generative_recommenders_amd.modules.dlrm_hstu import DlrmHSTU, EmbeddingCollection
    from generative_recommenders_amd.modules.hstu_transducer import HSTUTransducer
    from generative_recommenders_amd.modules.multitask_module import DefaultMultitaskModule
    from generative_recommenders_amd.modules.postprocessors import LayerNormPostprocessor, TimestampLayerNormPostprocessor

    assert "torchrec" not in sys.modules
    for inference in (False, True):
        m = R.build(is_inference=inference)
        assert isinstance(m, DlrmHSTU) and m._is_inference == inference
        assert isinstance(m._embedding_collection, EmbeddingCollection) and isinstance(m._multitask_module, DefaultMultitaskModule)
        assert isinstance(m._hstu_transducer, HSTUTransducer) and isinstance(m._item_embedding_mlp, torch.nn.Sequential)
        post = m._hstu_transducer._output_postprocessor         # the default: the timestamp postprocessor with the two DLRM periods
        assert isinstance(post, TimestampLayerNormPostprocessor)
        assert post._period_units.tolist() == [[3600.0, 86400.0]] and post._units_per_period.tolist() == [[24.0, 7.0]]
        assert all(p.device.type == "cpu" for p in m.parameters())
    cfg = R.config()
    cfg.use_layer_norm_postprocessor = True
    assert isinstance(DlrmHSTU(cfg, R.tables(), False)._hstu_transducer._output_postprocessor, LayerNormPostprocessor)
    inputs = R.load("model_small")
    R.build(False, inputs)        # strict load of the reference's state dict


def test_time_buffers_stay_fp32_whatever_the_module_is_cast_to():
    m = R.build(is_inference=False)
    post = m._hstu_transducer._output_postprocessor
    for dt in (torch.bfloat16, torch.float64, torch.float16):
        m = m.to(dt)
        assert post._time_feature_combiner.weight.dtype == dt
        assert post._period_units.dtype == torch.float32 and post._period_units.tolist() == [[3600.0, 86400.0]]
        assert post._units_per_period.dtype == torch.float32 and post._units_per_period.tolist() == [[24.0, 7.0]]


def test_local_feature_container_and_embedding_collection():
    from generative_recommenders_amd.modules.dlrm_hstu import EmbeddingCollection, KeyedJaggedTensor

    inputs = R.load("model_small")
    uih, cand = R.features(inputs, "cpu")
    assert uih.keys()[:2] == ["user_id", "uih_item_id"] and cand.keys()[0] == "cand_item_id"
    assert uih["uih_item_id"].lengths().tolist() == R.UIH_LENGTHS and uih["user_id"].lengths().tolist() == [1] * 6
    assert cand["cand_weight"].lengths().tolist() == R.CANDIDATES and cand["cand_weight"].values().numel() == sum(R.CANDIDATES)
    merged = KeyedJaggedTensor.from_lengths_sync(uih.keys() + cand.keys(), torch.cat([uih.values(), cand.values()]),
                                                 torch.cat([uih.lengths(), cand.lengths()]))
    assert torch.equal(merged["cand_item_id"].values(), cand["cand_item_id"].values())
    ec = EmbeddingCollection(list(R.tables().values()))
    assert list(ec.state_dict()) == ["embeddings.item_id.weight", "embeddings.user_id.weight"]
    out = ec(merged)
    assert sorted(out) == ["cand_item_id", "uih_item_id", "user_id"]      # the features of a table, nothing else
    assert torch.equal(out["uih_item_id"].values(), ec.embeddings["item_id"].weight[uih["uih_item_id"].values()])
    assert out["user_id"].lengths().tolist() == [1] * 6


def test_supervision_labels_follow_the_bitmask():
    from generative_recommenders_amd.modules.dlrm_hstu import _get_supervision_labels_and_weights

    labels, weights = _get_supervision_labels_and_weights(torch.tensor([0, 1, 2, 3, 7]), torch.tensor([5, 0, 1, 2, 3]),
                                                          R.config().multitask_configs)
    assert weights == {} and list(labels) == ["is_click", "is_like", "vvp"]
    assert labels["is_click"].tolist() == [0, 1, 0, 1, 1] and labels["is_like"].tolist() == [0, 0, 1, 1, 1]
    assert labels["vvp"].tolist() == [5, 0, 1, 2, 3] and labels["vvp"].dtype == torch.float32


def test_fixture_files_are_small_and_gated_tensors_are_off_the_truth():
    import os

    truth = R.load("model_small_f64")
    inputs = R.load("model_small")
    gated = [str(k) for k in inputs["gated"]]
    assert {"user_embeddings", "item_embeddings", "preds", "losses"} <= set(gated)
    assert all(("gp:" + str(k)) in gated for k in inputs["param_keys"])           # every parameter, the tables included
    for tag in ("f32", "bf16"):
        run = R.load("model_small_" + tag)
        for k in gated:
            assert R.rel_fro(run[k], truth[k]) > 0.0, (tag, k)
    for f in os.listdir(R.FIXTURES):
        assert os.path.getsize(os.path.join(R.FIXTURES, f)) <= 1 << 20, f
