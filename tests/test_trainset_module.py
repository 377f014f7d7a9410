"""onepose_amd.TrainingSet end to end on the GPU: a planted scan (300 points, 12 views of 96 x 128) through
ObjectMapper.build_from_matches, ``training_set``, ``batch`` and ``training_loss``; the batch against tests/trainset_oracle.py bit for
bit; the pair lists against the oracle's rule; batches across objects; the reference's files written and read back."""
import numpy as np
import pytest
import torch

import trainset_oracle as oracle
from onepose_amd import GATsSuperGlue, MatchingLoss, ObjectMapper, SparseTarget, TrainingSet, synthetic, training_loss

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HP = {"descriptor_dim": 256, "keypoints_encoder": [32, 64, 128], "match_type": "softmax", "scale_factor": 0.07,
      "match_threshold": 0.2, "include_self": True, "additional": False, "with_linear_transform": False}
SHAPE = dict(shape2d=160, shape3d=320, num_leaf=4)


@pytest.fixture(scope="module")
def built():
    scene = synthetic.make_map_scene(n_points=300, n_views=12, hw=(96, 128), seed=1)
    mapper = ObjectMapper(leaf_seed=5, device=DEV)
    db = mapper.build_from_matches(scene["features"], scene["pair_matches"], scene["poses"], scene["Ks"], scene["box"])
    keys = set(mapper.last)
    ts = mapper.training_set(scene["features"], image_size=scene["hw"])
    assert set(mapper.last) == keys and set(db) == {"keypoints3d", "descriptors3d_db", "descriptors2d_db"}
    return scene, mapper, ts


def case_of(scene, mapper):
    """the build's results as a case of the oracle"""
    last = mapper.last
    n_kpts = [len(f["keypoints"]) for f in scene["features"]]
    return dict(point_offsets=last["point_offsets"], obs_image=last["gather_image"], obs_kpt=last["gather_kpt"],
                collect=np.ascontiguousarray(last["anno"]["collect"]["descriptors3d"].T.astype(np.float32)),
                points3d=last["merged_xyz"].astype(np.float32), mean_desc=last["anno"]["average"]["descriptors3d"].astype(np.float32),
                features=scene["features"], image_hw=np.array([scene["hw"]] * len(n_kpts), np.int32),
                kpt_offsets=np.concatenate([[0], np.cumsum(n_kpts)]).astype(np.int32))


def test_pairs_are_the_oracle_rule_and_name_planted_points(built):
    scene, mapper, ts = built
    c = case_of(scene, mapper)
    offs, kpt, point, ignored = oracle.assign_pairs(c["point_offsets"], c["obs_image"], c["obs_kpt"], c["kpt_offsets"])
    assert int(ts.ignored.item()) == ignored == 0 and len(ts) == len(ts.image_ids) == 12 and ts.image_ids == list(range(12))
    assert ts.pair_counts == np.diff(offs).tolist() and min(ts.pair_counts) > 50
    for v in range(ts.V):
        p = ts.pairs(v)
        assert p.dtype == torch.int32 and p.is_cuda and tuple(p.shape) == (2, ts.pair_counts[v])
        assert np.array_equal(p.cpu().numpy(), np.stack([kpt[offs[v]:offs[v + 1]], point[offs[v]:offs[v + 1]]]))
        planted = scene["kp_point"][v][p[0].cpu().numpy()]
        assert (planted >= 0).all() and len(set(planted.tolist())) == len(planted)       # matched keypoints see distinct planted points


def test_batch_equals_the_oracle_and_feeds_training_loss(built):
    scene, mapper, ts = built
    ids = [ts.image_ids[0], ts.image_ids[5], ts.image_ids[11]]
    data, target = ts.batch(ids, epoch=3, seed=17, **SHAPE)
    assert set(data) == {"keypoints2d", "descriptors2d_query", "keypoints3d", "descriptors3d_db", "descriptors2d_db", "image_size"}
    want = oracle.build_batch(case_of(scene, mapper), ids, [3, 3, 3], SHAPE["shape2d"], SHAPE["shape3d"], SHAPE["num_leaf"], 17)
    for k in ("keypoints2d", "descriptors2d_query", "keypoints3d", "descriptors3d_db", "descriptors2d_db"):
        got = data[k].cpu().numpy()
        assert got.shape == want[k].shape and got.dtype == np.float32 and got.tobytes() == want[k].tobytes(), k
    assert data["image_size"].tolist() == [[96.0, 128.0]] * 3
    assert isinstance(target, SparseTarget) and target.n_orig == [min(ts.n_kpts[v], 160) for v in ids] and target.m_orig == [min(ts.N, 320)] * 3
    assert all(p.data_ptr() == ts.pairs(v).data_ptr() for p, v in zip(target.pairs, ids))          # views of the resident lists
    model = GATsSuperGlue(HP).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(0).items()}, strict=True)
    crit = MatchingLoss()
    loss = training_loss(model, data, target, crit)
    loss.backward()
    inside = sum(int(((ts.pairs(v)[0] < 160) & (ts.pairs(v)[1] < 320)).sum()) for v in ids)
    total = sum(ts.pair_counts[v] for v in ids)
    print(f"{total} pairs in the three images, {inside} of them inside {SHAPE['shape2d']} x {SHAPE['shape3d']}")
    assert crit.last_counts[0].item() == inside and 0 < inside <= total    # reshape_assign_matrix drops a pair beyond the padded shape
    assert np.isfinite(loss.item())
    for name, p in model.named_parameters():
        if p.grad is None:
            assert name.startswith(("kenc_", "bin_score")), name       # what the reference's training forward does not run either
        else:
            assert bool(torch.isfinite(p.grad).all()), name
    assert sum(p.grad is not None for p in model.parameters()) > 50


def test_ten_adam_steps_on_fresh_epochs_lower_the_loss(built):
    scene, mapper, ts = built
    model = GATsSuperGlue(HP).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(0).items()}, strict=True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = MatchingLoss()
    losses = []
    for epoch in range(10):
        data, target = ts.batch(ts.image_ids[:3], epoch=epoch, **SHAPE)
        loss = training_loss(model, data, target, crit)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_from_arrays_and_batches_across_objects(built):
    scene, mapper, ts = built
    c = case_of(scene, mapper)
    other = TrainingSet.from_arrays(c["point_offsets"], c["collect"], c["points3d"], c["mean_desc"], scene["features"], obs_image=c["obs_image"],
                                    obs_kpt=c["obs_kpt"], image_size=scene["hw"], device=DEV)
    assert other.pair_counts == ts.pair_counts and all(torch.equal(other.pairs(v), ts.pairs(v)) for v in range(ts.V))
    data, target = TrainingSet.batch_of([(ts, [4, 7]), (other, [2])], epoch=[1, 1, 6], **SHAPE)
    a, _ = ts.batch([4, 7], 1, **SHAPE)
    b, tb = other.batch([2], 6, **SHAPE)
    for k in data:
        assert torch.equal(data[k][:2], a[k]) and torch.equal(data[k][2:], b[k]), k
    assert len(target) == 3 and target.pairs[2].data_ptr() == tb.pairs[0].data_ptr()
    with pytest.raises(ValueError, match=r"image 12 is outside \[0, 12\)"):
        ts.batch([12], 0, **SHAPE)


def test_written_annotations_read_back_to_identical_tensors(built, tmp_path):
    scene, mapper, ts = built
    path = ts.write_training_annotations(str(tmp_path))
    from onepose_amd.mapping import write_annotation_files
    write_annotation_files(str(tmp_path), mapper.last["anno"])
    back = TrainingSet.from_reference_files(path, str(tmp_path / "anno"), image_size=scene["hw"], device=DEV)
    assert len(back) == len(ts) == back.V                              # every image has a pair: the list holds them all, in order
    for name in ("point_offsets", "collect", "points3d", "mean_desc", "kpts2d", "scores2d", "desc2d", "kpt_offsets", "image_hw"):
        a, b = getattr(ts, name), getattr(back, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert all(torch.equal(ts.pairs(v), back.pairs(v)) for v in range(ts.V))
    d0, _ = ts.batch([1, 2], 0, **SHAPE)
    d1, _ = back.batch([1, 2], 0, **SHAPE)
    assert all(torch.equal(d0[k], d1[k]) for k in d0)
