"""The training-set builder on the GPU against tests/trainset_oracle.py, bit for bit: every stage entry and gts_build_batch at the
edges of the 64-column gather tile, with b of 1 and 3, every shape2d of tests/trainset_cases.py, images with no keypoints and with
fewer, as many and more than shape2d, N below, at and above shape3d, a point without observations; then the sample rules (the same
image twice, two epochs, another slot) and two calls from a NaN-filled workspace.  Every buffer a call writes holds 0xFF (NaN / -1)
before it.  Integer arithmetic and copies only: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import trainset_cases as tc
import trainset_oracle as oracle
from arena import Memory, bitwise_equal

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def run(body):
    """the body on plain buffers that hold 0xFF; outputs as numpy"""
    got = body(Memory(DEV, 0xFF, tc.ROLES))
    full = got[0] if isinstance(got, tuple) else got
    return {k: v.cpu().numpy() for k, v in full.items()}


def same(got, want, keys=None):
    for k in keys or got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), f"{k}: {int((got[k] != want[k]).sum())} entries differ"


@pytest.mark.parametrize("L", [1, 5, 8])
def test_assign_pairs(L):
    c = tc.case(L)
    got = run(tc.body_assign(c))
    offs, kpt, point, ignored = oracle.assign_pairs(c["point_offsets"], c["obs_image"], c["obs_kpt"], c["kpt_offsets"])
    assert np.array_equal(got["pair_offsets"], offs) and int(got["ignored"][0]) == ignored == 4
    assert np.array_equal(got["pair_kpt"][:offs[-1]], kpt) and np.array_equal(got["pair_point"][:offs[-1]], point)
    assert (got["pair_kpt"][offs[-1]:] == -1).all()                     # not written
    assert offs[1] == 0 and offs[-1] > 0                                # the image without keypoints has no pair


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("shape3d,L", tc.TILES)
def test_stage_entries(shape3d, L, b):
    """select, gather, pad_points at every tile edge: 1, 63, 64, 65 and 264 leaf columns.  A mishandled last partial tile of the gather
    shows at 7 x 9, 13 x 5 and 33 x 8."""
    c = tc.case(L)
    images, epochs = tc.samples(b, shape3d)
    leaf = run(tc.body_select(c, images, epochs, shape3d, L))["leaf_src"]
    want = oracle.select_leaves(c["point_offsets"], images, epochs, shape3d, L, tc.SEED)
    same(dict(leaf_src=leaf), dict(leaf_src=want))
    for s in range(b):
        oracle.check_leaves(leaf[s], np.diff(c["point_offsets"]), L, shape3d)
    same(run(tc.body_gather(c, leaf, shape3d, L)), dict(descriptors2d_db=oracle.gather_leaves(c["collect"], want)))
    k3, d3 = oracle.pad_points(c["points3d"], c["mean_desc"], images, epochs, shape3d, tc.SEED)
    same(run(tc.body_pad_points(c, images, epochs, shape3d)), dict(keypoints3d=k3, descriptors3d_db=d3))
    assert (np.abs(k3[:, tc.N_POINTS:]) <= 0.5).all()


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("shape2d", tc.SHAPES2D)
def test_pad_query(shape2d, b):
    c = tc.case(8)
    images, epochs = tc.samples(b, shape2d)
    dq, kq, sq = oracle.pad_query(c["features"], c["image_hw"], images, epochs, shape2d, tc.SEED)
    same(run(tc.body_pad_query(c, images, epochs, shape2d)), dict(descriptors2d_query=dq, keypoints2d=kq, scores_query=sq))


def test_pad_query_with_no_fewer_as_many_and_more_keypoints_than_shape2d():
    """images of 0, 40, 64 and 200 keypoints at shape2d = 64.  Epoch 5 is one at which two first draws of the 40-keypoint image land on
    a keypoint of the 24 x 32 image (a condition on the oracle, asserted): a redraw happens, and no pad equals a keypoint of its image"""
    c, shape2d = tc.case(8), 64
    images, epochs = np.array([0, 1, 3, 6], np.int32), np.array([5, 5, 5, 5], np.int32)
    dq, kq, sq = oracle.pad_query(c["features"], c["image_hw"], images, epochs, shape2d, tc.SEED)
    got = run(tc.body_pad_query(c, images, epochs, shape2d))
    same(got, dict(descriptors2d_query=dq, keypoints2d=kq, scores_query=sq))
    first = np.array([[oracle.draw_index(oracle.stream_key(tc.SEED, oracle.TAG_PAD2D, 5, 1, j), k, n) for k, n in ((0, 24), (1, 32))] for j in range(40, 64)])
    assert int((first != kq[1, 40:]).any(axis=1).sum()) == 2            # two first draws were rejected
    own = set(map(tuple, c["features"][1]["keypoints"].tolist()))
    assert not any(tuple(p) in own for p in got["keypoints2d"][1, 40:].tolist())
    assert (got["keypoints2d"][0, :, 0] < 24).all() and (got["keypoints2d"][0, :, 1] < 32).all() and got["keypoints2d"][0, :, 1].max() >= 24


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("shape3d,L", tc.TILES)
def test_build_batch(shape3d, L, b):
    c = tc.case(L)
    shape2d = tc.SHAPES2D[tc.TILES.index((shape3d, L))]
    images, epochs = tc.samples(b, shape3d)
    want = oracle.build_batch(c, images, epochs, shape2d, shape3d, L, tc.SEED)
    same(run(tc.body_build(c, images, epochs, shape2d, shape3d, L)), want, ["descriptors2d_query", "keypoints2d", "scores_query", "keypoints3d",
                                                                           "descriptors3d_db", "descriptors2d_db"])


@pytest.mark.parametrize("shape2d", tc.SHAPES2D)
def test_build_batch_at_every_shape2d(shape2d):
    c, shape3d, L = tc.case(8), 13, 8
    images, epochs = tc.samples(3, shape2d)
    want = oracle.build_batch(c, images, epochs, shape2d, shape3d, L, tc.SEED)
    got = run(tc.body_build(c, images, epochs, shape2d, shape3d, L))
    same(got, {k: want[k] for k in got})


def test_a_sample_depends_on_seed_epoch_and_image_alone():
    c, shape2d, shape3d, L = tc.case(8), 65, 13, 8
    build = lambda images, epochs: run(tc.body_build(c, np.array(images, np.int32), np.array(epochs, np.int32), shape2d, shape3d, L))  # noqa: E731
    a = build([2, 2, 5], [0, 0, 0])
    for k, v in a.items():
        assert v[0].tobytes() == v[1].tobytes(), k                      # the same image twice: identical rows
    e = build([2, 5], [1, 0])
    assert e["descriptors2d_db"][0].tobytes() != a["descriptors2d_db"][0].tobytes()      # another epoch: other leaves
    assert e["keypoints2d"][0].tobytes() != a["keypoints2d"][0].tobytes() and e["keypoints3d"][0].tobytes() != a["keypoints3d"][0].tobytes()
    assert e["descriptors3d_db"][0].tobytes() == a["descriptors3d_db"][0].tobytes()
    for k in a:
        assert e[k][1].tobytes() == a[k][2].tobytes(), k                # the same (epoch, image) in another slot, beside other samples


def test_two_calls_from_a_nan_filled_workspace_are_bitwise_equal():
    c, shape2d, shape3d, L = tc.case(8), 130, 33, 8
    images, epochs = tc.samples(3, 1)
    once = tc.body_build(c, images, epochs, shape2d, shape3d, L)(Memory(DEV, 0xFF, tc.ROLES))
    twice = tc.body_build(c, images, epochs, shape2d, shape3d, L, calls=2)(Memory(DEV, 0xFF, tc.ROLES))
    zeros = tc.body_build(c, images, epochs, shape2d, shape3d, L)(Memory(DEV, 0x00, tc.ROLES))
    for k in once:
        assert bitwise_equal(once[k], twice[k]) and bitwise_equal(once[k], zeros[k]), k
        assert not torch.isnan(once[k]).any(), k
