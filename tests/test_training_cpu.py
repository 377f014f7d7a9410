"""onepose_amd.training on the CPU: the stock-torch paths (impl="eager", matching_descriptors, SparseTarget.dense) against what the
unmodified reference gives under autograd (tests/golden/train_*.npz), and the refusals of impl="hip".  No GPU.

Bounds (the reference's own fp32 deviation from its fp64 run is recorded per case in train_golden_meta.json): loss, relative:
max(1e-6, 4 x deviation); a gradient tensor, max|d| / max|golden|: max(2e-6, 4 x deviation).  The factor 4 covers another summation
order, 1e-6 / 2e-6 are 16 / 32 fp32 ulps."""
import numpy as np
import pytest
import torch

import onepose_amd
from onepose_amd import synthetic
from onepose_amd.training import MatchingLoss, SparseTarget, matching_descriptors, training_loss
from conftest import load_golden
from test_train_oracle_golden import HEAD_CASES, META, head_case


def loss_bound(dev):
    return max(1e-6, 4 * dev)


def grad_bound(dev):
    return max(2e-6, 4 * dev)


def test_exports():
    assert {"MatchingLoss", "SparseTarget", "matching_descriptors", "training_loss"} <= set(onepose_amd.__all__)
    assert onepose_amd.MatchingLoss is MatchingLoss and "oracle" not in open(onepose_amd.training.__file__).read().replace("torch_oracle", "")


def eager(name, target_of=lambda pairs, target, meta: torch.from_numpy(target)):
    x, y, pairs, target, focal, g, meta = head_case(name)
    crit = MatchingLoss(alpha=focal["alpha"], gamma=focal["gamma"], pos_weights=focal["pos_w"], neg_weights=focal["neg_w"],
                        scale_factor=focal["scale"], impl="eager")
    tx, ty = torch.from_numpy(x).requires_grad_(), torch.from_numpy(y).requires_grad_()
    loss = crit(tx, ty, target_of(pairs, target, meta))
    loss.backward()
    return loss.item(), tx.grad.numpy(), ty.grad.numpy(), crit, g, meta, target


@pytest.mark.parametrize("name", HEAD_CASES)
def test_eager_head_equals_the_reference(name):
    loss, dx, dy, crit, g, meta, target = eager(name)
    dev = meta["fp32_deviation"]
    assert abs(loss - float(g["loss"])) <= loss_bound(dev["loss"]) * abs(float(g["loss"]))
    assert np.abs(dx - g["dx"]).max() <= grad_bound(dev["dx"]) * np.abs(g["dx"]).max()
    assert np.abs(dy - g["dy"]).max() <= grad_bound(dev["dy"]) * np.abs(g["dy"]).max()
    assert crit.last_counts.tolist() == [(target == 1).sum(), (target == 0).sum(), ((target != 0) & (target != 1)).sum()]


@pytest.mark.parametrize("name", ["edge", "pad0"])
def test_eager_head_takes_a_sparse_target(name):
    def sparse(pairs, target, meta):
        i = meta["inputs"]
        return SparseTarget([torch.from_numpy(p) for p in pairs], i["n_orig"], i["m_orig"], pad_val=i["pad_val"])
    loss, dx, _, _, _, _, _ = eager(name, sparse)
    loss_d, dx_d, _, _, _, _, _ = eager(name)
    assert loss == loss_d and np.array_equal(dx, dx_d)


def test_neither_positive_nor_negative_is_zero_with_zero_gradients():
    x = torch.nn.functional.normalize(torch.randn(1, 256, 6, generator=torch.Generator().manual_seed(0)), dim=1).requires_grad_()
    y = torch.nn.functional.normalize(torch.randn(1, 256, 9, generator=torch.Generator().manual_seed(1)), dim=1).requires_grad_()
    crit = MatchingLoss(impl="eager")
    loss = crit(x, y, torch.full((1, 6, 9), -1, dtype=torch.int16))
    loss.backward()
    assert loss.item() == 0.0 and not x.grad.any() and not y.grad.any() and crit.last_counts.tolist() == [0, 0, 54]


@pytest.mark.parametrize("name", sorted(META["assign"]))
def test_sparse_target_dense_equals_reshape_assign_matrix(name):
    g, s = load_golden("train_assign"), META["assign"][name]
    pairs = torch.from_numpy(g[name + ".pairs"])
    t = SparseTarget([pairs, pairs[:, :7]], [s["n_orig"], s["n"]], [s["m_orig"], s["m"]], pad_val=s["pad_val"]).dense(s["n"], s["m"])
    assert t.dtype is torch.int16 and tuple(t.shape) == (2, s["n"], s["m"])
    np.testing.assert_array_equal(t[0].numpy(), g[name + ".target"])
    assert int(t[1].sum()) == len({(int(i), int(j)) for i, j in pairs[:, :7].T.tolist() if i < s["n"] and j < s["m"]})   # no pad band at all
    with_negative = torch.cat([pairs, torch.tensor([[-1], [0]], dtype=pairs.dtype)], dim=1)
    np.testing.assert_array_equal(SparseTarget([with_negative], s["n_orig"], s["m_orig"], s["pad_val"]).dense(s["n"], s["m"])[0].numpy(),
                                  g[name + ".target"])


def test_sparse_target_refusals():
    p = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="pad_val = 1"):
        SparseTarget([p], 4, 4, pad_val=1)
    with pytest.raises(TypeError, match="integers"):
        SparseTarget([p.float()], 4, 4)
    with pytest.raises(ValueError, match="one non-negative int per sample"):
        SparseTarget([p, p], [4], [4, 4])
    with pytest.raises(ValueError, match=r"\[b, 2, k\]"):
        SparseTarget(torch.zeros(2, 3, 4, dtype=torch.int32), 4, 4)
    assert len(SparseTarget(torch.zeros(3, 2, 5, dtype=torch.int64), 4, 4)) == 3


def test_matching_loss_refusals():
    x, y = torch.zeros(2, 256, 5), torch.zeros(2, 256, 7)
    t = torch.zeros(2, 5, 7, dtype=torch.int16)
    with pytest.raises(ValueError, match="impl must be one of"):
        MatchingLoss(impl="triton")
    with pytest.raises(RuntimeError, match=r"tensor 'mdesc0' is on cpu\); there is no CPU fallback"):
        MatchingLoss()(x, y, t)                                       # impl="hip" is never swapped for eager silently
    crit = MatchingLoss(impl="eager")
    for bad in (t[:, :4], t.float(), t[:1], None):
        with pytest.raises(ValueError, match="target must be"):
            crit(x, y, bad)
    with pytest.raises(ValueError, match=r"\[b, 256, n\]"):
        crit(x[:, :128], y[:, :128], t)
    with pytest.raises(ValueError, match="the target has 1 samples"):
        crit(x, y, SparseTarget([torch.zeros(2, 1, dtype=torch.int32)], 5, 7))
    assert "impl='eager'" in repr(crit)


@pytest.fixture(scope="module")
def network():
    """The whole-network golden's module (reference state_dict names, loaded strict), inputs and target, on the CPU."""
    meta = META["network"]
    model = onepose_amd.GATsSuperGlue(dict(meta["hparams"]))
    kind, seed = meta["weights"]
    assert kind == "random"
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(seed).items()}, strict=True)
    inputs = dict(meta["inputs"], noise=tuple(meta["inputs"]["noise"]))
    data = {k: torch.from_numpy(v) for k, v in synthetic.make_inputs(**inputs).items()}
    return model, data, load_golden("train_network"), meta


def test_matching_descriptors_equal_the_reference(network):
    model, data, g, meta = network
    with torch.no_grad():
        m0, m1 = matching_descriptors(model, data)
    for ours, key in ((m0, "mdesc0"), (m1, "mdesc1")):
        assert tuple(ours.shape) == g[key].shape
        assert np.abs(ours.numpy() - g[key]).max() <= grad_bound(meta["fp32_deviation"][key]) * np.abs(g[key]).max(), key


def test_training_loss_parameter_gradients_equal_the_reference(network):
    model, data, g, meta = network
    model.zero_grad()
    loss = training_loss(model, data, torch.from_numpy(g["target"]), MatchingLoss(impl="eager", scale_factor=meta["hparams"]["scale_factor"]))
    loss.backward()
    assert abs(loss.item() - float(g["loss"])) <= loss_bound(meta["fp32_deviation"]["loss"]) * abs(float(g["loss"]))
    devs = meta["fp32_deviation"]["grads"]
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(got) == set(devs) and len(devs) == 4 * 2 + 8 * 12 + 2    # kenc_* and bin_score never reach the forward
    for k, d in devs.items():
        grad = got[k].numpy().astype(np.float64)
        if d["zero"]:       # no gradient by construction (a bias in front of an InstanceNorm ...): noise of the size of the reference's own
            assert np.abs(grad).max() <= 4 * d["fp32_absmax"] + 1e-30, k
            continue
        norm, top, pos, val = float(g["norm::" + k]), float(g["max::" + k]), g["pos::" + k], g["val::" + k]
        bound = grad_bound(d["deviation"])
        assert np.abs(grad.reshape(-1)[pos] - val).max() <= bound * top, k
        assert abs(np.linalg.norm(grad) - norm) <= bound * top * np.sqrt(grad.size), k     # what max|d| <= bound * top implies for the norm
