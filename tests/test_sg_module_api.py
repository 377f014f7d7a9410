"""SuperGlue module API: constructor, config merge, state_dict compatibility, refusals, empty inputs (no GPU needed)."""
import json
import os

import numpy as np
import pytest
import torch

from onepose_amd import SuperGlue, SuperGlueEngine, synthetic  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_default_config_merge():
    m = SuperGlue({"match_threshold": 0.7})
    assert m.config["match_threshold"] == 0.7
    assert m.config["sinkhorn_iterations"] == 100
    assert m.config["GNN_layers"] == ["self", "cross"] * 9
    assert m.n_layers == 18 and m.layer_kinds[:2] == [0, 1]


def test_state_dict_keys_equal_reference_and_strict_round_trip():
    with open(os.path.join(GOLD, "sg_golden_meta.json")) as f:
        keys = json.load(f)["state_dict_keys"]
    m = SuperGlue({})
    assert list(m.state_dict().keys()) == keys
    sd = synthetic.make_superglue_state_dict(0)
    assert list(sd.keys()) == keys
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m2 = SuperGlue({})
    m2.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(m2.gnn.layers[3].attn.proj[1].weight, torch.from_numpy(sd["gnn.layers.3.attn.proj.1.weight"]))


def test_custom_layer_list():
    m = SuperGlue({"GNN_layers": ["cross", "self", "cross"]})
    assert len(m.gnn.layers) == 3 and m.layer_kinds == [1, 0, 1]
    assert len(m._raw_slots) == 29 + 16 * 3


@pytest.mark.parametrize("cfg", [{"descriptor_dim": 128}, {"keypoint_encoder": [32, 64, 128]}, {"GNN_layers": ["self", "other"]},
                                 {"num_heads": 8}, {"sinkhorn_iterations": -1}])
def test_unsupported_configs_refused(cfg):
    with pytest.raises(ValueError):
        SuperGlue(cfg)


def _empty_data(n0, n1):
    return {"keypoints0": torch.zeros(1, n0, 2), "keypoints1": torch.zeros(1, n1, 2), "scores0": torch.zeros(1, n0),
            "scores1": torch.zeros(1, n1), "descriptors0": torch.zeros(1, 256, n0), "descriptors1": torch.zeros(1, 256, n1),
            "image0": torch.zeros(1, 1, 8, 8), "image1": torch.zeros(1, 1, 8, 8)}


def test_training_mode_raises():
    m = SuperGlue({})
    with pytest.raises(RuntimeError, match="inference only"):
        m(_empty_data(0, 3))


@pytest.mark.parametrize("n0,n1", [(0, 5), (4, 0), (0, 0)])
def test_empty_input_matches_reference_contract(n0, n1):
    m = SuperGlue({}).eval()
    out = m(_empty_data(n0, n1))
    assert out["matches0"].dtype == torch.int32 and out["matches1"].dtype == torch.int32
    assert out["matches0"].shape == (1, n0) and out["matches1"].shape == (1, n1)
    assert (out["matches0"] == -1).all() and (out["matches1"] == -1).all()
    assert out["matching_scores0"].dtype == torch.float32 and (out["matching_scores1"] == 0).all()
    assert m._engine is None       # nothing loaded, nothing launched


def test_cpu_inputs_refused_without_fallback():
    m = SuperGlue({}).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(_empty_data(3, 4))
