"""The numpy oracle of the training-set builder (tests/trainset_oracle.py) against the reference's own outputs
(tests/golden/trainset_golden.npz and tests/golden/trainset_ref/, written by tests/golden/make_trainset_golden.py): pairs, leaf
selections under one property checker, pads; the uniformity of the oracle's draw; and the reader and writer of the reference's
annotation files.  No GPU."""
import json
import os

import numpy as np
import pytest

import trainset_oracle as oracle
from conftest import GOLDEN_DIR, load_golden
from onepose_amd import mapping, synthetic, trainset

REF_DIR = os.path.join(GOLDEN_DIR, "trainset_ref")
MODEL_SEED, MODEL = 11, dict(n_images=6, n_points=30, dim=16)        # of tests/golden/make_trainset_golden.py
SHAPES3D, SHAPES2D = [3, 5, 8], [6, 10, 25]
UNIFORM_SEED = 2024


@pytest.fixture(scope="module")
def golden():
    return load_golden("trainset_golden")


@pytest.fixture(scope="module")
def model_pairs(golden):
    """the golden's model again from its seed, its observations grouped by merged point (mapping.point_observations with the
    reference's own filter and merge results), and the oracle's pairs"""
    model = synthetic.make_map_model(MODEL_SEED, **MODEL)
    mask = np.ones(len(model["obs_image"]), np.int32)
    where = {int(t): i for i, t in enumerate(golden["kept_ids"])}       # the reference names a member by its track, the builder by its position
    members = np.array([where[int(t)] for t in golden["members"]], np.int64)
    offs, img, kpt = mapping.point_observations(model["track_offsets"], model["obs_image"], model["obs_kpt"], mask, golden["kept_ids"],
                                                golden["member_offsets"], members)
    n_kpts = [len(f["keypoints"]) for f in model["features"]]
    kpt_offsets = np.concatenate([[0], np.cumsum(n_kpts)]).astype(np.int32)
    return model, (offs, img, kpt), kpt_offsets, oracle.assign_pairs(offs, img, kpt, kpt_offsets)


def test_oracle_pairs_equal_the_reference_assign_matrices(golden, model_pairs):
    model, (offs, img, kpt), kpt_offsets, (pair_offsets, pair_kpt, pair_point, ignored) = model_pairs
    assert ignored == 0 and np.array_equal(np.diff(offs), golden["idxs"]) and len(offs) - 1 == int(golden["n_merged"])
    listed = golden["listed_images"].tolist()
    assert len(listed) >= 5
    for v in range(len(model["features"])):
        mine = np.stack([pair_kpt[pair_offsets[v]:pair_offsets[v + 1]], pair_point[pair_offsets[v]:pair_offsets[v + 1]]]).astype(np.int64)
        if v not in listed:
            assert mine.shape[1] == 0                                   # images with no pair are left out of the list
            continue
        ref = golden[f"assign_{v}"]
        ref = ref[:, np.argsort(ref[0], kind="stable")]                 # the reference lists them in dictionary order
        assert len(set(ref[0].tolist())) == ref.shape[1] and np.array_equal(mine, ref), v
    assert pair_offsets[-1] == sum(golden[f"assign_{v}"].shape[1] for v in listed) > 60
    host = trainset.pairs_from_observations(offs, img, kpt, np.diff(kpt_offsets))           # the module's own host restatement
    assert all(np.array_equal(host[v], np.stack([pair_kpt[pair_offsets[v]:pair_offsets[v + 1]], pair_point[pair_offsets[v]:pair_offsets[v + 1]]]))
               for v in range(len(host)))


def reference_selection(leaves, K):
    """the reference's leaves hold column values j + 2 (1: the dustbin): back to rows of collect, the dustbin as K"""
    assert (leaves == leaves[0]).all()
    return np.where(leaves[0] == 1, K, leaves[0] - 2).astype(np.int64)


@pytest.mark.parametrize("shape3d", SHAPES3D)
def test_check_leaves_passes_on_the_reference_selections_and_on_the_oracle(golden, shape3d):
    idxs, L = golden["in_idxs"], int(golden["num_leaf"])
    assert idxs.tolist() == [1, L - 1, L, L + 1, 3 * L] and min(SHAPES3D) < len(idxs) < max(SHAPES3D) and len(idxs) in SHAPES3D
    offsets = np.concatenate([[0], np.cumsum(idxs)]).astype(np.int32)
    seen = set()
    for rep in range(4):
        sel = reference_selection(golden[f"leaves_{shape3d}_{rep}"], int(idxs.sum()))
        assert sel.shape == (shape3d * L,)
        assert oracle.check_leaves(sel, idxs[:shape3d], L, shape3d)    # truncated to shape3d points: the later points' rows never show
        seen.add(sel.tobytes())
    assert len(seen) > 1
    mine = oracle.select_leaves(offsets, [0, 3, 3], [0, 0, 1], shape3d, L, seed=5)
    for s in range(3):
        assert oracle.check_leaves(mine[s], idxs[:shape3d], L, shape3d)
    assert mine[1].tobytes() != mine[2].tobytes() and mine[0].tobytes() != mine[1].tobytes()
    assert mine.dtype == np.int32 and mine.shape == (3, shape3d * L)
    repeated, foreign, pad = mine[0].copy(), mine[0].copy(), mine[0].copy()
    repeated[2 * L:3 * L] = repeated[2 * L]                             # the checker checks: a repeated row,
    foreign[2 * L] = offsets[2] - 1                                     # a row of another point,
    pad[-1] = 0                                                         # a row in a pad point (or one too many in the last point)
    for bad in (repeated, foreign, pad):
        with pytest.raises(AssertionError):
            oracle.check_leaves(bad, idxs[:shape3d], L, shape3d)
    # the gathered descriptors of the oracle, read back like the reference's
    got = oracle.gather_leaves(np.ascontiguousarray(golden["in_collect"].T), mine[:1])
    assert np.array_equal(reference_selection(np.where(mine[0] < 0, 1, got[0]), int(idxs.sum())), np.where(mine[0] < 0, idxs.sum(), mine[0]))


@pytest.mark.parametrize("shape3d", SHAPES3D)
def test_pad_points_agrees_with_the_reference_in_everything_but_the_random_values(golden, shape3d):
    kp3, avg = golden["in_kp3"], golden["in_avg"]
    ref_k, ref_d = golden[f"kp3_{shape3d}"], golden[f"avg_{shape3d}"]
    pad = np.zeros((256 - avg.shape[0], avg.shape[1]), np.float32)      # the oracle is dimension 256 only: the golden's 4 channels on top
    k3, d3 = oracle.pad_points(kp3, np.concatenate([avg, pad]), [2], [7], shape3d, seed=3)
    k3, d3 = k3[0], d3[0][:avg.shape[0]]
    n = min(len(kp3), shape3d)
    assert k3.shape == ref_k.shape and k3.dtype == ref_k.dtype and d3.shape == ref_d.shape and d3.dtype == ref_d.dtype
    assert np.array_equal(k3[:n], ref_k[:n]) and np.array_equal(d3, ref_d)              # copied part; the pad descriptors are ones in both
    assert (d3[:, n:] == 1).all()
    for pads in (k3[n:], ref_k[n:]):
        assert ((pads >= -0.5) & (pads < 0.5)).all()
        assert not any((p == kp3).all(axis=1).any() for p in pads)                      # no pad equals an original
    assert np.array_equal(k3[n:] * 2.0 ** 24, np.round(k3[n:] * 2.0 ** 24))             # on the 2^-24 grid: exact in fp32


@pytest.mark.parametrize("shape2d", SHAPES2D)
def test_pad_query_agrees_with_the_reference_in_everything_but_the_random_values(golden, shape2d):
    kp2, d2, s2, (h, w) = golden["in_kp2"], golden["in_d2"], golden["in_s2"], golden["image_hw"]
    ref_k, ref_d, ref_s = golden[f"kp2_{shape2d}"], golden[f"d2_{shape2d}"], golden[f"s2_{shape2d}"]
    feature = {"keypoints": kp2, "descriptors": np.concatenate([d2, np.zeros((256 - d2.shape[0], d2.shape[1]), np.float32)]), "scores": s2[:, 0]}
    dq, kq, sq = oracle.pad_query([feature], [(h, w)], [0], [1], shape2d, seed=3)
    dq, kq, sq = dq[0][:d2.shape[0]], kq[0], sq[0][:, None]
    n = min(len(kp2), shape2d)
    for mine, ref in ((kq, ref_k), (dq, ref_d), (sq, ref_s)):
        assert mine.shape == ref.shape and mine.dtype == ref.dtype
    assert np.array_equal(kq[:n], ref_k[:n]) and np.array_equal(dq, ref_d) and np.array_equal(sq, ref_s)
    assert (dq[:, n:] == 1).all() and (sq[n:] == 0).all()
    own = set(map(tuple, kp2.tolist()))
    for pads in (kq[n:], ref_k[n:]):
        assert np.array_equal(pads, np.round(pads))                                     # integers stored as floats
        assert ((pads[:, 0] >= 0) & (pads[:, 0] < h)).all() and ((pads[:, 1] >= 0) & (pads[:, 1] < w)).all()      # the reference's (y, x) order
        assert not any(tuple(p) in own for p in pads.tolist())                          # no pad equals an original
    if shape2d > n:     # a rejected draw: 10 of the 64 pixels are keypoints, and among the oracle's first draws one meets one
        first = [(oracle.draw_index(oracle.stream_key(3, oracle.TAG_PAD2D, 1, 0, j), 0, h), oracle.draw_index(oracle.stream_key(3, oracle.TAG_PAD2D, 1, 0, j), 1, w))
                 for j in range(n, shape2d)]
        assert any(tuple(map(float, f)) in own for f in first)


def frequencies(cnt, L, points, seed):
    offsets = (np.arange(points + 1) * cnt).astype(np.int64)
    sel = oracle.select_leaves(offsets, [0], [0], points, L, seed)[0].reshape(points, L)
    local = np.where(sel >= 0, sel - offsets[:-1, None], -1)
    return local


def within(count, n, p, sigmas=5):
    return abs(count - n * p) <= sigmas * np.sqrt(n * p * (1 - p))


def test_the_draw_is_uniform():
    """cnt = 12, L = 8, 20 000 points at a fixed seed: every candidate is selected with frequency 8/12 and shows in every slot with
    frequency 1/12; at cnt = 3 every slot is the dustbin with frequency 5/8 and holds each observation with frequency 1/8.  All within
    5 binomial standard deviations: a condition of the seed, found by running this test, not a measurement."""
    n, L = 20000, 8
    local = frequencies(12, L, n, UNIFORM_SEED)
    assert (local >= 0).all()
    for c in range(12):
        assert within(int((local == c).sum()), n, 8 / 12), c
        for slot in range(L):
            assert within(int((local[:, slot] == c).sum()), n, 1 / 12), (c, slot)
    local = frequencies(3, L, n, UNIFORM_SEED)
    for slot in range(L):
        assert within(int((local[:, slot] < 0).sum()), n, 5 / 8), slot
        for j in range(3):
            assert within(int((local[:, slot] == j).sum()), n, 1 / 8), (slot, j)
    assert ((local >= 0).sum(axis=1) == 3).all()


def test_the_reader_round_trips_the_reference_files(golden):
    features, pairs, records = trainset.read_annotation_json(os.path.join(REF_DIR, "anno_2d.json"), relocate=REF_DIR)
    model = synthetic.make_map_model(MODEL_SEED, **MODEL)
    listed = golden["listed_images"].tolist()
    assert [r["anno_id"] for r in records] == list(range(1, len(listed) + 1)) and len(features) == len(pairs) == len(listed)
    for f, a, v in zip(features, pairs, listed):
        want = model["features"][v]
        assert f["keypoints"].dtype == f["descriptors"].dtype == f["scores"].dtype == np.float32 and a.dtype == np.int64
        assert np.array_equal(f["keypoints"], want["keypoints"]) and np.array_equal(f["descriptors"], want["descriptors"])
        assert np.array_equal(f["scores"], want["scores"]) and np.array_equal(a, golden[f"assign_{v}"])
    a3 = trainset.read_annotation_3d(REF_DIR)
    assert np.array_equal(a3["idxs"], golden["idxs"]) and a3["collect"].shape == (int(golden["idxs"].sum()), MODEL["dim"])
    assert a3["points3d"].shape == (len(a3["idxs"]), 3) and a3["mean_desc"].shape == (MODEL["dim"], len(a3["idxs"]))
    assert all(a3[k].dtype == np.float32 for k in ("collect", "points3d", "mean_desc"))
    # the mean of a point's collected rows is its mean descriptor (float64 in the files)
    np.testing.assert_allclose(a3["collect"][:a3["idxs"][0]].astype(np.float64).mean(axis=0), a3["mean_desc"][:, 0], rtol=0, atol=1e-6)


def test_the_writer_writes_what_the_reference_writes_and_the_reader_reads_it_back(golden, model_pairs, tmp_path):
    model, (offs, img, kpt), kpt_offsets, _ = model_pairs
    mine = trainset.pairs_from_observations(offs, img, kpt, np.diff(kpt_offsets))
    path = trainset.write_annotation_json(str(tmp_path), model["features"], mine, image_names=[f"color/{v}.png" for v in range(len(mine))])
    features, pairs, records = trainset.read_annotation_json(path)
    ref_features, ref_pairs, ref_records = trainset.read_annotation_json(os.path.join(REF_DIR, "anno_2d.json"), relocate=REF_DIR)
    assert len(records) == len(ref_records) and [set(r) for r in records] == [set(r) for r in ref_records]
    for f, a, rf, ra, r, rr in zip(features, pairs, ref_features, ref_pairs, records, ref_records):
        assert all(np.array_equal(f[k], rf[k]) and f[k].dtype == rf[k].dtype for k in f)        # identical arrays
        assert np.array_equal(a, ra[:, np.argsort(ra[0], kind="stable")]) and r["anno_id"] == rr["anno_id"]
        with open(r["anno_file"]) as fh, open(os.path.join(REF_DIR, os.path.basename(rr["anno_file"]))) as rh:
            d, rd = json.load(fh), json.load(rh)
        assert set(d) == set(rd) == {"keypoints2d", "descriptors2d", "scores2d", "assign_matrix", "num_matches"}
        assert d["num_matches"] == rd["num_matches"] and all(np.asarray(d[k]).shape == np.asarray(rd[k]).shape for k in d)
        assert d["keypoints2d"] == rd["keypoints2d"] and d["descriptors2d"] == rd["descriptors2d"] and d["scores2d"] == rd["scores2d"]
    # an image without a pair is left out
    fewer = list(mine)
    fewer[2] = np.zeros((2, 0), np.int64)
    _, _, left = trainset.read_annotation_json(trainset.write_annotation_json(str(tmp_path / "fewer"), model["features"], fewer))
    assert len(left) == len(records) - 1 and [r["anno_id"] for r in left] == list(range(1, len(records)))
    assert all(os.path.basename(r["anno_file"]) != "2.json" for r in left)


def test_the_oracle_chain_on_a_small_case():
    """the sample rules on the oracle alone: same image twice, another epoch, another slot"""
    case = oracle.make_case(8, (1, 3, 4, 5, 12, 0, 2, 5), [0, 10, 20], seed=1)
    a = oracle.build_batch(case, [1, 1, 2], [0, 0, 0], 16, 13, 4, seed=9)
    e = oracle.build_batch(case, [2, 1], [0, 1], 16, 13, 4, seed=9)
    for k in a:
        assert np.array_equal(a[k][0], a[k][1]) and np.array_equal(a[k][2], e[k][0]), k
    assert not np.array_equal(a["leaf_src"][0], e["leaf_src"][1])
    for s in range(3):
        oracle.check_leaves(a["leaf_src"][s], np.diff(case["point_offsets"]), 4, 13)
    assert a["descriptors2d_db"].shape == (3, 256, 52) and (a["descriptors2d_db"][:, :, 8 * 4:] == 1).all()
    assert (a["descriptors2d_db"][0, 0] == np.where(a["leaf_src"][0] < 0, 1, a["leaf_src"][0])).all()      # channel 0 of a row is its index
