"""The oracle of the object database builder's post-processing (tests/mapping_oracle.py) and the host-side pair selection
(onepose_amd.mapping.covis_pairs) against outputs of the REFERENCE itself (tests/golden/map_post.npz, written by
tests/golden/make_map_golden.py from the reference's covis_from_pose, get_tkl, filter_3d, merge and get_kpt_ann): array_equal,
same dtypes.  The synthetic model is regenerated from its seed; no GPU needed."""
import os

import numpy as np
import pytest

import mapping_oracle as mo
from onepose_amd import database_io, mapping, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_post.npz")
SEED = 7


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def model():
    return synthetic.make_map_model(SEED)


@pytest.fixture(scope="module")
def post(model):
    lengths = np.diff(model["track_offsets"]).astype(np.int32)
    return mo.post_process(model["xyz"], lengths, model["track_offsets"], model["obs_image"], model["obs_kpt"],
                           np.ones(len(model["obs_image"]), np.int32), model["features"], model["box"], model["max_num_kp3d"])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_covisible_pairs(golden, model):
    pairs = np.array(mapping.covis_pairs(model["poses"], model["seq_ids"], 10, max_rotation=50), np.int64)
    assert same(pairs, golden["pairs"])
    assert len({tuple(sorted(p)) for p in pairs.tolist()}) < len(pairs)                  # both orientations occur: unique_pairs matters
    uniq = mapping.unique_pairs(pairs.tolist())
    assert len({tuple(sorted(p)) for p in uniq}) == len(uniq) == len({tuple(sorted(p)) for p in pairs.tolist()})


def test_track_length_threshold_lands_on_a_middle_bin(golden, model, post):
    assert post["threshold"] == int(golden["track_length"])
    lengths = np.diff(model["track_offsets"])
    assert lengths.min() < post["threshold"] < lengths.max()


def test_kept_ids_and_coordinates(golden, model, post):
    assert np.array_equal(post["kept_ids"], golden["kept_ids"]) and same(post["kept_xyz"], golden["kept_xyz"])
    lengths = np.diff(model["track_offsets"])
    long_enough = lengths >= post["threshold"]
    assert len(post["kept_ids"]) < long_enough.sum()                                       # the box rejects points too


def test_merged_points_and_members(golden, post):
    assert same(post["merged_xyz"].astype(np.float64), golden["merged_xyz"])
    assert np.array_equal(post["member_offsets"], golden["member_offsets"])
    assert np.array_equal(post["kept_ids"][post["members"]], golden["members"])
    sizes = np.diff(golden["member_offsets"])
    assert sizes.max() == 3 and (sizes == 2).any()                                         # a triple and a pair inside 1 mm
    assert golden["members"].shape[0] < golden["kept_ids"].shape[0]                       # the chain's end is dropped, as in the reference


def test_annotation_arrays(golden, post):
    anno = post["anno"]
    assert same(anno["idxs"], golden["idxs"])
    for ours, ref in (("average", "avg"), ("collect", "clt")):
        for key in ("keypoints3d", "descriptors3d", "scores3d"):
            assert same(anno[ours][key], golden[f"{ref}_{key}"]), (ours, key)


def test_written_files_load_through_database_io(tmp_path, golden, post):
    paths = mapping.write_annotation_files(str(tmp_path), post["anno"])
    assert [os.path.basename(p) for p in paths] == ["anno_3d_average.npz", "anno_3d_collect.npz", "idxs.npy"]
    assert os.path.basename(os.path.dirname(paths[0])) == "anno"
    db = database_io.load_object_database(*paths, num_leaf=8, seed=3, device="cpu")
    n = len(golden["idxs"])
    assert db["keypoints3d"].shape == (1, n, 3) and db["descriptors3d_db"].shape == (1, 16, n) and db["descriptors2d_db"].shape == (1, 16, 8 * n)
    assert np.array_equal(db["keypoints3d"][0].numpy(), golden["clt_keypoints3d"].astype(np.float32))
    again = mapping.database_from_annotation(post["anno"], num_leaf=8, seed=3, device="cpu")
    assert all(np.array_equal(db[k].numpy(), again[k].numpy()) for k in db)
