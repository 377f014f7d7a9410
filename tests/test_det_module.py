"""onepose_amd.LocalFeatureObjectDetector on the GPU against the oracle chain (tests/detector_oracle.py): with a stub matcher
that plants matches, with the real HIP SuperGlue on planted descriptor pairs (oracle tail fed with the HIP matcher's own
matches0), with the real extractor in front, previous_pose_detect, and the refusals."""
import numpy as np
import pytest
import torch
from torch import nn

import det_cases as dc
import detector_oracle as do
from onepose_amd import LocalFeatureObjectDetector, SuperGlue, SuperPoint, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = np.array([[1063.2, 0.0, 318.7], [0.0, 1071.9, 243.1], [0.0, 0.0, 1.0]])


class PlantedExtractor(nn.Module):
    """Returns prepared features in call order: the reference views first, then the query for every later call."""

    def __init__(self, feats):
        super().__init__()
        self.feats, self.calls = feats, 0

    def forward(self, img):
        assert img.is_cuda and img.dim() == 4
        f = self.feats[min(self.calls, len(self.feats) - 1)]
        self.calls += 1
        return {k: [torch.from_numpy(np.ascontiguousarray(v)).to(img.device)] for k, v in f.items()}


class PlantedMatcher(nn.Module):
    """SuperGlue's forward(data) contract; returns the planted matches of the views in call order."""

    def __init__(self, matches):
        super().__init__()
        self.matches, self.calls = matches, 0

    def forward(self, data):
        m = self.matches[self.calls % len(self.matches)]
        self.calls += 1
        n0, dev = data["keypoints0"].shape[1], data["keypoints0"].device
        assert len(m) == n0 and data["image0"].shape[-2:] == torch.Size(dc.HW0)
        return {"matches0": torch.from_numpy(m)[None].to(dev), "matching_scores0": torch.ones(1, n0, device=dev)}


def feats_of(kpts, seed):
    rs = np.random.RandomState(seed)
    n = len(kpts)
    d = rs.normal(size=(256, n)).astype(np.float32)
    return {"keypoints": np.asarray(kpts, np.float32), "scores": rs.uniform(0.1, 0.9, n).astype(np.float32),
            "descriptors": d / np.maximum(np.linalg.norm(d, axis=0, keepdims=True), 1e-9)}


def frame(h, w, seed):
    u8 = np.random.RandomState(seed).randint(0, 256, size=(h, w)).astype(np.uint8)
    return u8, torch.from_numpy(u8.astype(np.float32) / np.float32(255))[None, None].to(DEV)


def oracle_chain(kpts0_list, matches0_list, kpts1, hw0_list, u8, crop, rank_by="matches"):
    tail = do.detect_tail(kpts0_list, matches0_list, kpts1, hw0_list, u8.shape, rank_by=rank_by)
    return tail, do.crop_resize(u8, tail["bbox"], crop), do.k_crop(tail["bbox"], K, crop)


@pytest.mark.parametrize("rank_by,crop", [("matches", 512), ("inliers", 256)])
def test_detect_with_planted_matches_equals_the_oracle_chain(rank_by, crop):
    ns = [64, 5, 300, 1024, 300, 7]
    views = [dc.planted_view(n, 900 + i) for i, n in enumerate(ns)]
    assert all(all(v["conditions"]) for v in views)
    emb = dc.embed(views, 5)
    k0 = [emb["kpts0"][i, :emb["n0"][i]] for i in range(len(ns))]
    m0 = [emb["matches0"][i, :emb["n0"][i]] for i in range(len(ns))]
    refs = [torch.zeros(1, 1, *dc.HW0, device=DEV) for _ in ns]
    ext = PlantedExtractor([feats_of(k, i) for i, k in enumerate(k0)] + [feats_of(emb["kpts1"], 99)])
    det = LocalFeatureObjectDetector(ext, PlantedMatcher(m0), ref_images=refs, rank_by=rank_by)
    assert det.V == len(ns) and det.kpts0.is_cuda and det.db_dict[0]["descriptors"].is_cuda
    u8, img = frame(480, 640, 3)
    bbox, crop_t, K_crop = det.detect(img, None, K, crop_size=crop)
    tail, ref_crop, ref_K = oracle_chain(k0, m0, emb["kpts1"], [dc.HW0] * len(ns), u8, crop, rank_by)
    assert isinstance(bbox, np.ndarray) and np.array_equal(bbox, tail["bbox"])
    assert np.array_equal(det.last["info"].cpu().numpy(), tail["info"]) and int(det.last["best_view"]) == tail["best_view"]
    assert np.array_equal(det.last["boxes"].cpu().numpy(), tail["boxes"])
    assert crop_t.is_cuda and crop_t.shape == (1, 1, crop, crop) and crop_t.dtype == torch.float32
    assert crop_t[0, 0].cpu().numpy().tobytes() == ref_crop.tobytes()
    assert isinstance(K_crop, np.ndarray) and K_crop.tobytes() == ref_K.tobytes()
    # rank by matches: 1024 matches win; the reference's helpers keep their return shapes
    res = det.match_worker({**{k: torch.from_numpy(v).to(DEV) for k, v in feats_of(emb["kpts1"], 99).items()}, "size": np.array([480, 640])})
    assert set(res) == set(range(len(ns))) and res[1]["inliers"].shape == (0,) and res[1]["bbox"].tolist() == [0, 0, 480, 640]
    assert res[3]["inliers"].shape == (1024, 1) and int(res[3]["inliers"].sum()) == views[3]["count"]
    assert np.array_equal(det.detect_by_matching({**{k: torch.from_numpy(v).to(DEV) for k, v in feats_of(emb["kpts1"], 99).items()},
                                                  "size": np.array([480, 640])}), tail["bbox"])
    img_crop, K2 = det.crop_img_by_bbox(img, bbox, K, crop_size=crop)
    assert img_crop.dtype == np.uint8 and np.array_equal(img_crop, np.rint(ref_crop * 255).astype(np.uint8)) and np.array_equal(K2, ref_K)


def planted_descriptor_views(rs, q, sizes, planted):
    """Views whose planted keypoints are the query's under a similarity and share its descriptors."""
    out = []
    for (n0, k), seed in zip(zip(sizes, planted), range(len(sizes))):
        f = feats_of(np.stack([rs.uniform(0, 639, n0), rs.uniform(0, 479, n0)], -1), 50 + seed)
        p0, p1 = rs.permutation(n0)[:k], rs.permutation(len(q["keypoints"]))[:k]
        ang, sc, t = rs.uniform(-0.5, 0.5), rs.uniform(0.6, 1.5), rs.uniform(-40, 120, 2)
        R = sc * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        f["keypoints"][p0] = ((q["keypoints"][p1] - t) @ np.linalg.inv(R).T).astype(np.float32)
        f["descriptors"][:, p0] = q["descriptors"][:, p1]
        out.append(f)
    return out


def test_detect_device_with_the_hip_superglue_equals_the_oracle_tail():
    rs = np.random.RandomState(2)
    q = feats_of(np.stack([rs.uniform(0, 639, 400), rs.uniform(0, 479, 400)], -1), 7)
    views = planted_descriptor_views(rs, q, [300, 4, 257, 120], [150, 4, 100, 3])
    sd = synthetic.make_superglue_passthrough_state_dict(6, 4)      # planted pairs (equal descriptors) survive the network
    sg = SuperGlue({"GNN_layers": ["self", "cross"] * 2, "sinkhorn_iterations": 100, "match_threshold": 0.7}).eval()
    sg.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    refs = [torch.zeros(1, 1, *dc.HW0, device=DEV) for _ in views]
    det = LocalFeatureObjectDetector(PlantedExtractor(views + [q]), sg, ref_images=refs)
    u8, img = frame(480, 640, 4)
    bbox, crop_t, K_crop, best = det.detect_device(img, K)
    assert all(t.is_cuda for t in (bbox, crop_t, K_crop, best)) and bbox.dtype == torch.int32 and K_crop.dtype == torch.float64
    torch.cuda.synchronize()
    matches = det.matches0.cpu().numpy()
    m0 = [matches[i, :len(v["keypoints"])] for i, v in enumerate(views)]
    # the padded buffer holds what the module path returns for the same pair
    pred = sg({"keypoints0": torch.from_numpy(views[0]["keypoints"])[None].to(DEV), "scores0": torch.from_numpy(views[0]["scores"])[None].to(DEV),
               "descriptors0": torch.from_numpy(views[0]["descriptors"])[None].to(DEV), "keypoints1": torch.from_numpy(q["keypoints"])[None].to(DEV),
               "scores1": torch.from_numpy(q["scores"])[None].to(DEV), "descriptors1": torch.from_numpy(q["descriptors"])[None].to(DEV),
               "image0": torch.empty(1, 1, *dc.HW0), "image1": torch.empty(1, 1, 480, 640)})
    assert np.array_equal(pred["matches0"][0].cpu().numpy(), m0[0])
    tail, _, _ = oracle_chain([v["keypoints"] for v in views], m0, q["keypoints"], [dc.HW0] * len(views), u8, 512)
    info = det.last["info"].cpu().numpy()
    print("matches per view", info[:, 1].tolist(), "inliers", info[:, 3].tolist(), "bbox", bbox.cpu().numpy().tolist())
    assert np.array_equal(info, tail["info"])
    assert info[1, 0] == 0 and info[1, 1] < 6 and info[3, 0] == 0          # the < 6 branch
    assert info[0, 0] == 1 and info[0, 1] >= 100 and info[0, 3] >= 50       # the planted similarity is found
    assert np.array_equal(det.last["mask"].cpu().numpy()[0, :300], tail["masks"][0])
    assert np.array_equal(bbox.cpu().numpy(), tail["bbox"]) and int(best) == tail["best_view"]
    if int(det.last["crop_info"][0]):
        assert crop_t[0, 0].cpu().numpy().tobytes() == do.crop_resize(u8, tail["bbox"], 512).tobytes()
        assert K_crop.cpu().numpy().tobytes() == do.k_crop(tail["bbox"], K, 512).tobytes()


def test_full_chain_with_the_hip_extractor_and_matcher():
    """SuperPoint -> V x SuperGlue -> tail -> crop on real kernels end to end; the tail equals the oracle on the same matches."""
    ext = SuperPoint({"nms_radius": 3, "max_keypoints": 300}).eval()
    ext.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_spp_state_dict(0).items()}, strict=True)
    sd = synthetic.make_superglue_state_dict(10, 2)
    sg = SuperGlue({"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 10, "match_threshold": 0.0}).eval()
    sg.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    refs = [torch.from_numpy(synthetic.make_image(1, 96, 128, 20 + i)).to(DEV) for i in range(3)]
    det = LocalFeatureObjectDetector(ext, sg, ref_images=refs, iterations=500)
    img = torch.from_numpy(synthetic.make_image(1, 120, 160, 20)).to(DEV)
    bbox, crop_t, K_crop, best = det.detect_device(img, K, crop_size=256)
    torch.cuda.synchronize()
    k0 = [v["keypoints"].cpu().numpy() for v in det.db_dict.values()]
    m0 = [det.matches0[i, :len(k)].cpu().numpy() for i, k in enumerate(k0)]
    tail = do.detect_tail(k0, m0, det.last["keypoints1"].cpu().numpy(), [(96, 128)] * 3, (120, 160), iterations=500)
    assert np.array_equal(det.last["info"].cpu().numpy(), tail["info"]) and np.array_equal(bbox.cpu().numpy(), tail["bbox"])
    u8 = do.to_u8(img[0, 0].cpu().numpy())
    if int(det.last["crop_info"][0]):
        assert crop_t[0, 0].cpu().numpy().tobytes() == do.crop_resize(u8, tail["bbox"], 256).tobytes()
    assert crop_t.shape == (1, 1, 256, 256)


def test_previous_pose_detect_equals_the_oracle():
    det = LocalFeatureObjectDetector(PlantedExtractor([feats_of(np.zeros((3, 2)), 0)]), PlantedMatcher([np.full(3, -1, np.int64)]),
                                     ref_images=[torch.zeros(1, 1, *dc.HW0, device=DEV)])
    u8, img = frame(480, 640, 8)
    pose = np.array([[0.96, -0.1, 0.26, 0.02], [0.12, 0.99, -0.06, -0.01], [-0.25, 0.09, 0.96, 0.6]])
    corners = np.array([[x, y, z] for x in (-0.05, 0.05) for y in (-0.04, 0.04) for z in (-0.03, 0.03)])
    bbox, crop_t, K_crop = det.previous_pose_detect(img, K, pose, corners)
    ref_box = do.pose_box(K, pose, corners)
    assert np.array_equal(bbox, ref_box) and bbox.dtype == np.int32
    assert crop_t[0, 0].cpu().numpy().tobytes() == do.crop_resize(u8, ref_box, 512).tobytes()
    assert K_crop.tobytes() == do.k_crop(ref_box, K, 512).tobytes()
    pose4 = np.concatenate([pose, [[0, 0, 0, 1]]])
    assert np.array_equal(det.previous_pose_detect(img, K, pose4, corners, crop_size=256)[0], ref_box)


def test_refusals():
    det = LocalFeatureObjectDetector(PlantedExtractor([feats_of(np.zeros((3, 2)), 0)]), PlantedMatcher([np.full(3, -1, np.int64)]),
                                     ref_images=[torch.zeros(1, 1, *dc.HW0, device=DEV)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        det.detect(torch.zeros(1, 1, 48, 64), None, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        det.previous_pose_detect(torch.zeros(1, 1, 48, 64), K, np.eye(4)[:3], np.ones((8, 3)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LocalFeatureObjectDetector(PlantedExtractor([]), PlantedMatcher([]), ref_images=[torch.zeros(1, 1, 48, 64)])
    with pytest.raises(Exception, match="power of two"):
        det.detect(torch.zeros(1, 1, 48, 64, device=DEV), None, K, crop_size=300)
    with pytest.raises(ValueError, match="rank_by"):
        LocalFeatureObjectDetector(PlantedExtractor([]), PlantedMatcher([]), ref_images=[], rank_by="votes")
    # all views fail on a 48 x 64 frame: bbox = [0, 0, H, W] as the reference has it
    bbox, crop_t, _ = det.detect(torch.zeros(1, 1, 48, 64, device=DEV), None, K, crop_size=64)
    assert bbox.tolist() == [0, 0, 48, 64]
