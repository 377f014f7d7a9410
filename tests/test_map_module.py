"""onepose_amd.ObjectMapper.build_from_matches on a planted object (about 300 points, 12 views of 96 x 128, fp32 keypoints)
against the whole oracle chain (tests/mapping_oracle.run_chain): one noise-free scene and one with 0.3 px noise and 10 % wrong
matches.  The scenes meet the exactness conditions of tests/map_cases.py (asserted in tests/test_map_cases.py)."""
import functools
import os

import numpy as np
import pytest
import torch

import map_cases as mc
import mapping_oracle as mo
from onepose_amd import GATsSuperGlue, ObjectMapper, database_io, synthetic

SCENES = {"clean": dict(noise_px=0.0, wrong_frac=0.0, seed=1), "noisy": dict(noise_px=0.3, wrong_frac=0.1, seed=2)}
HP = {"descriptor_dim": 256, "keypoints_encoder": [32, 64, 128], "match_type": "softmax", "scale_factor": 0.07,
      "match_threshold": 0.2, "include_self": True, "additional": False, "with_linear_transform": False}


@functools.lru_cache(maxsize=None)
def scene_and_reference(name):
    scene = synthetic.make_map_scene(n_points=300, n_views=12, hw=(96, 128), outside_frac=0.05, **SCENES[name])
    return scene, mo.run_chain(scene["features"], scene["pair_matches"], scene["poses"], scene["Ks"], scene["box"])


def scene_conditions(scene, ref):
    verify = all(mc.verify_conditions(dict(residuals=r, thr2=mo.MAX_EPIPOLAR_ERROR ** 2))[0] for r in ref["verify_residuals"])
    # residual and angle margins for every hypothesis of every track.  The runner-up condition is not asked of whole scenes: a
    # noisy scene always holds a few tracks in which two observation pairs reach the same count with different inlier sets
    # (4 of 234 here).  With the margins above both sides count the same integers, and the tie goes to the lowest index on
    # both; the stage tests keep the condition for their planted tracks.
    tracks = all(all(mc.track_conditions(r)[:2]) for r in ref["tracks"])
    return (verify, tracks) + mc.points_conditions(ref["xyz"], ref["lengths"], scene["box"])


def track_bound(ref, t):
    """The bound of tests/test_map_hip.xyz_bound for track t of a chain result."""
    s, e = ref["track_offsets"][t], ref["track_offsets"][t + 1]
    cams, xy, r = ref["cams"][ref["obs_image"][s:e]], ref["obs_xy"][s:e], ref["tracks"][t]
    ld = mo.refit(cams, xy, r["inliers"], r["start"], dtype=np.longdouble)
    return 4 * float(np.abs(r["xyz"] - ld).max()) + 4 * np.finfo(np.float64).eps * float(np.abs(ld).max())


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    out = {}
    for name in SCENES:
        scene, ref = scene_and_reference(name)
        mapper = ObjectMapper(leaf_seed=5, device="cuda:0")
        out_dir = tmp_path_factory.mktemp(name)
        db = mapper.build_from_matches(scene["features"], scene["pair_matches"], scene["poses"], scene["Ks"], scene["box"], out_dir=str(out_dir))
        out[name] = (scene, ref, mapper, db)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_the_whole_result_equals_the_oracle_chain(built, name):
    scene, ref, mapper, db = built[name]
    got = mapper.last
    assert all(scene_conditions(scene, ref))
    assert np.array_equal(got["counts"], ref["counts"]) and all(np.array_equal(a, b) for a, b in zip(got["survivors"], ref["survivors"]))
    for k in ("track_offsets", "obs_image", "obs_kpt", "info", "inlier_mask", "lengths"):
        assert np.array_equal(got[k], ref[k]), k
    worst = 0.0
    for t in np.nonzero(ref["info"][:, 0])[0]:
        err, bound = float(np.abs(got["xyz"][t] - ref["xyz"][t]).max()), track_bound(ref, t)
        worst = max(worst, err)
        assert err <= bound, (t, err, bound)
    print(f"{name}: {len(ref['info'])} tracks, worst |HIP - oracle| of a point {worst:.3e}")
    assert got["threshold"] == ref["threshold"]
    for k in ("kept_ids", "member_offsets", "members", "point_offsets", "gather_image", "gather_kpt"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["kept_xyz"].tobytes() == ref["kept_xyz"].tobytes() and got["merged_xyz"].tobytes() == ref["merged_xyz"].tobytes()
    for part in ("average", "collect"):
        for key, val in ref["anno"][part].items():
            assert got["anno"][part][key].dtype == val.dtype and got["anno"][part][key].tobytes() == val.tobytes(), (part, key)
    assert np.array_equal(got["anno"]["idxs"], ref["anno"]["idxs"])
    assert 150 < len(ref["merged_xyz"]) <= 300


def rounding_displacement(ref, t, planted):
    """Where rounding the keypoints to fp32 moves the least-squares point of track t, to first order, in longdouble: the scene is
    noise-free, so the residuals r of the planted point are exactly the rounding errors of its keypoints (about 2^-18 px), and
    the minimiser of the reprojection error over the inliers sits at planted - (J^T J)^-1 J^T r.  The second-order remainder is
    smaller by the factor |displacement| / depth times the conditioning of J^T J: about 1e-8 x 1e2 here."""
    ld = np.longdouble
    s, e = ref["track_offsets"][t], ref["track_offsets"][t + 1]
    sel = ref["tracks"][t]["inliers"]
    c, xy, X = ref["cams"][ref["obs_image"][s:e]][sel].astype(ld), ref["obs_xy"][s:e][sel].astype(ld), planted.astype(ld)
    p = np.stack([c[:, 4 * k:4 * k + 3] @ X + c[:, 4 * k + 3] for k in range(3)], axis=1)
    u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    r = np.stack([c[:, 12] * u + c[:, 14] - xy[:, 0], c[:, 13] * v + c[:, 15] - xy[:, 1]], axis=1)
    J0 = (c[:, 12] / p[:, 2])[:, None] * (c[:, 0:3] - u[:, None] * c[:, 8:11])
    J1 = (c[:, 13] / p[:, 2])[:, None] * (c[:, 4:7] - v[:, None] * c[:, 8:11])
    H = J0.T @ J0 + J1.T @ J1
    g = J0.T @ r[:, 0] + J1.T @ r[:, 1]
    return -np.linalg.solve(H.astype(np.float64), g.astype(np.float64))


@pytest.mark.gpu
def test_noise_free_points_are_the_planted_ones(built):
    """The planted point was projected BEFORE the keypoints were rounded to fp32, so it is not the minimiser the kernels are
    asked for: the derived bound of the stage tests (about 5e-16 m) cannot hold against it, and is not asked to.  What is
    asserted instead, per track: xyz - planted equals the first-order displacement that the actual fp32 rounding errors of
    this track's keypoints cause (``rounding_displacement``), within the derived bound of the stage tests plus 1e-6 of that
    displacement for its second-order remainder.  The plain distance to the planted point is printed."""
    scene, ref, mapper, _ = built["clean"]
    ok = np.nonzero(ref["info"][:, 0])[0]
    assert len(ok) >= 280
    worst, worst_rest = 0.0, 0.0
    for t in ok:
        s = ref["track_offsets"][t]
        planted = scene["points"][scene["kp_point"][ref["obs_image"][s]][ref["obs_kpt"][s]]]
        moved = rounding_displacement(ref, t, planted)
        diff = mapper.last["xyz"][t] - planted
        rest = float(np.abs(diff - moved).max())
        worst, worst_rest = max(worst, float(np.abs(diff).max())), max(worst_rest, rest)
        assert rest <= track_bound(ref, t) + 1e-6 * float(np.abs(moved).max()), (t, rest, float(np.abs(moved).max()))
    print(f"worst |xyz - planted| {worst:.3e} m; worst |xyz - planted - first-order fp32 displacement| {worst_rest:.3e} m")


@pytest.mark.gpu
def test_a_planted_wrong_match_is_never_an_inlier_observation(built):
    """A planted wrong match joins two keypoints that lie more than 8 px, twice the reprojection threshold, from where the other's
    point is seen in their image (synthetic.make_map_scene): next to two right observations of a point it cannot be an inlier.  So every point with at least
    three inlier observations observes one planted point.  (Two observations alone cannot tell: a wrong keypoint that happens
    to lie on the epipolar line triangulates with its partner, here as in any two-view geometry.)"""
    scene, ref, mapper, _ = built["noisy"]
    got = mapper.last
    assert len(scene["wrong"]) > 100
    off = np.concatenate([[0], np.cumsum([len(f["keypoints"]) for f in scene["features"]])])
    planted = np.concatenate(scene["kp_point"])
    node = off[got["obs_image"]] + got["obs_kpt"]
    checked = 0
    for t in np.nonzero(got["info"][:, 0])[0]:
        s, e = got["track_offsets"][t], got["track_offsets"][t + 1]
        ids = planted[node[s:e]][got["inlier_mask"][s:e] > 0]
        if len(ids) >= 3:
            checked += 1
            assert len(set(ids.tolist())) == 1 and ids[0] >= 0, (t, ids)
    assert checked > 150
    assert (got["inlier_mask"] == 0).sum() > 0                          # wrong matches did reach the tracks and were dropped


@pytest.mark.gpu
def test_written_files_round_trip_and_feed_the_matcher(built):
    scene, ref, mapper, db = built["clean"]
    loaded = database_io.load_object_database(*mapper.last["paths"], num_leaf=8, seed=5, device="cuda:0")
    assert set(loaded) == set(db) == {"keypoints3d", "descriptors3d_db", "descriptors2d_db"}
    for k in db:
        assert loaded[k].dtype == db[k].dtype and torch.equal(loaded[k], db[k]), k
    n = db["keypoints3d"].shape[1]
    assert db["descriptors3d_db"].shape == (1, 256, n) and db["descriptors2d_db"].shape == (1, 256, 8 * n)
    matcher = GATsSuperGlue(HP).eval()
    matcher.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(0).items()}, strict=True)
    matcher = matcher.to("cuda:0")
    f = scene["features"][0]
    data = dict(db, keypoints2d=torch.from_numpy(f["keypoints"])[None].to("cuda:0"),
                descriptors2d_query=torch.from_numpy(f["descriptors"])[None].to("cuda:0"))
    with torch.no_grad():
        pred, conf = matcher(data)
    torch.cuda.synchronize()
    assert pred["matches0"].shape == (len(f["keypoints"]),) and conf.shape == (1, len(f["keypoints"]), n)


class SceneExtractor(torch.nn.Module):
    """SuperPoint's forward contract: returns the scene's features in call order."""

    def __init__(self, scene):
        super().__init__()
        self.scene, self.calls = scene, 0

    def forward(self, img):
        assert img.is_cuda and img.shape == (1, 1) + tuple(self.scene["hw"])
        f = self.scene["features"][self.calls]
        self.calls += 1
        return {k: [torch.from_numpy(v).to(img.device)] for k, v in f.items()}


class SceneMatcher(torch.nn.Module):
    """SuperGlue's forward(data) contract: recognises the two images by their keypoints and returns the planted matches."""

    def __init__(self, scene):
        super().__init__()
        self.scene, self.pairs = scene, []
        self.index = {f["keypoints"].tobytes(): v for v, f in enumerate(scene["features"])}

    def forward(self, data):
        i, j = (self.index[data[k][0].cpu().numpy().tobytes()] for k in ("keypoints0", "keypoints1"))
        assert data["image0"].shape[-2:] == data["image1"].shape[-2:] == torch.Size(self.scene["hw"]) and data["descriptors0"].shape[1] == 256
        self.pairs.append((i, j))
        where = {int(q): k for k, q in enumerate(self.scene["kp_point"][j]) if q >= 0}
        m0 = np.array([where.get(int(q), -1) if q >= 0 else -1 for q in self.scene["kp_point"][i]], np.int64)
        return {"matches0": torch.from_numpy(m0)[None].to(data["keypoints0"].device)}


@pytest.mark.gpu
def test_build_runs_extractor_pairs_and_matcher_in_front_of_the_same_tail(tmp_path):
    """build(): one extractor call per frame, covis_pairs of the poses, every unordered pair matched once, then the tail --
    the result is the one build_from_matches gives for the matches the matcher returned."""
    from onepose_amd import mapping
    scene, _ = scene_and_reference("clean")
    extractor, matcher = SceneExtractor(scene), SceneMatcher(scene)
    mapper = ObjectMapper(extractor, matcher, leaf_seed=5, device="cuda:0")
    frames = [torch.zeros(1, 1, *scene["hw"]) for _ in scene["features"]]
    db = mapper.build(frames, scene["poses"], scene["Ks"], scene["box"], out_dir=str(tmp_path))
    pairs = mapping.unique_pairs(mapping.covis_pairs(scene["poses"], None, mapping.COVIS_NUM))
    assert extractor.calls == len(frames) and matcher.pairs == pairs and len(pairs) > len(frames)
    assert len({tuple(sorted(p)) for p in pairs}) == len(pairs)
    planted = SceneMatcher(scene)
    feats = [{k: torch.from_numpy(v).to("cuda:0") for k, v in f.items()} for f in scene["features"]]
    pm = [(i, j, planted({"keypoints0": feats[i]["keypoints"][None], "keypoints1": feats[j]["keypoints"][None], "descriptors0": feats[i]["descriptors"][None],
                          "image0": torch.empty(1, 1, *scene["hw"], device="meta"), "image1": torch.empty(1, 1, *scene["hw"], device="meta")})["matches0"][0])
          for i, j in pairs]
    other = ObjectMapper(leaf_seed=5, device="cuda:0")
    db2 = other.build_from_matches(scene["features"], pm, scene["poses"], scene["Ks"], scene["box"])
    assert all(torch.equal(db[k], db2[k]) for k in db) and db["keypoints3d"].shape[1] > 150
    assert all(mapper.last["anno"][p][k].tobytes() == other.last["anno"][p][k].tobytes() for p in ("average", "collect") for k in other.last["anno"][p])
    assert all(os.path.exists(q) for q in mapper.last["paths"])
    with pytest.raises(RuntimeError, match="needs an extractor"):
        other.build(frames, scene["poses"], scene["Ks"], scene["box"])
    with pytest.raises(RuntimeError, match="needs a matcher"):
        other.build_from_features(scene["features"], pairs, scene["poses"], scene["Ks"], scene["box"])


def test_thresholds_are_checked():
    with pytest.raises(TypeError, match="unknown thresholds"):
        ObjectMapper(bogus=1)
