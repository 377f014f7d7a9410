"""onepose_amd.NearestNeighbour: the reference module's contract (constructor, conf, forward's refusals) without a GPU."""
import pytest
import torch

import onepose_amd
from onepose_amd import NearestNeighbour, NearestNeighbourEngine


def desc(b, n, d=256):
    return torch.zeros(b, d, n)


def test_conf_is_the_reference_default_with_conf_merged_over_it():
    assert NearestNeighbour.default_conf == {"match_threshold": None, "ratio_threshold": None, "distance_threshold": None, "do_mutual_check": True}
    assert NearestNeighbour().conf == NearestNeighbour.default_conf and NearestNeighbour({}).conf == NearestNeighbour.default_conf
    m = NearestNeighbour({"ratio_threshold": 0.8, "match_threshold": 0.3})
    assert m.conf == {"match_threshold": 0.3, "ratio_threshold": 0.8, "distance_threshold": None, "do_mutual_check": True}
    assert NearestNeighbour.default_conf["ratio_threshold"] is None                  # the class default is not written through
    assert m.thresholds() == (0.8, 0.0) and NearestNeighbour({"distance_threshold": 0.7, "ratio_threshold": 0}).thresholds() == (0.0, 0.7)
    assert "NearestNeighbour" in onepose_amd.__all__ and issubclass(NearestNeighbourEngine, onepose_amd._binding.Engine)


def test_the_module_has_no_parameters():
    m = NearestNeighbour({"distance_threshold": 0.7})
    assert len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
    m.load_state_dict({}, strict=True)
    assert m.eval() is m and m.cpu() is m


@pytest.mark.parametrize("conf", [{"ratio_threshold": -0.1}, {"distance_threshold": float("nan")}, {"distance_threshold": float("inf")}])
def test_bad_thresholds_are_refused_at_construction(conf):
    with pytest.raises(ValueError, match="must be a finite number >= 0 or None"):
        NearestNeighbour(conf)


def test_forward_refuses_host_tensors_with_the_projects_wording():
    with pytest.raises(RuntimeError, match=r"onepose_amd.NearestNeighbour runs only on a ROCm GPU \(the inputs are on cpu\); there is no CPU fallback"):
        NearestNeighbour()({"descriptors0": desc(1, 5), "descriptors1": desc(1, 7)})
    with pytest.raises(RuntimeError, match="item 0 is on cpu"):
        NearestNeighbour().match_pairs([{"descriptors0": desc(1, 5), "descriptors1": desc(1, 7)}] * 2)


def test_forward_refuses_what_the_reference_cannot_compute():
    nn = NearestNeighbour()
    with pytest.raises(ValueError, match="descriptor dimension 256 only"):
        nn({"descriptors0": desc(1, 5, 128), "descriptors1": desc(1, 7, 128)})
    for n0, n1 in ((0, 7), (5, 0)):
        with pytest.raises(ValueError, match="no nearest neighbour"):
            nn({"descriptors0": desc(1, n0), "descriptors1": desc(1, n1)})
    with pytest.raises(ValueError, match="with one b"):
        nn({"descriptors0": desc(1, 5), "descriptors1": desc(2, 7)})
    ratio = NearestNeighbour({"ratio_threshold": 0.8})
    for n0, n1 in ((1, 7), (5, 1)):
        with pytest.raises(ValueError, match="second neighbour"):
            ratio({"descriptors0": desc(1, n0), "descriptors1": desc(1, n1)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # one point a side is fine without the ratio test
        NearestNeighbour({"distance_threshold": 0.7})({"descriptors0": desc(1, 1), "descriptors1": desc(1, 1)})


def test_match_pairs_checks_its_items():
    nn = NearestNeighbour()
    with pytest.raises(ValueError, match="item 0: match_pairs takes pairs with batch size 1"):
        nn.match_pairs([{"descriptors0": desc(2, 5), "descriptors1": desc(2, 7)}])
    with pytest.raises(ValueError, match="no nearest neighbour"):
        nn.match_pairs([{"descriptors0": desc(1, 5), "descriptors1": desc(1, 0)}])
    assert nn.match_pairs([]) == []
    with pytest.raises(ValueError, match="max_items"):
        nn.match_pairs([], max_items=65)
