"""The users of the nearest-neighbour matcher: LocalFeatureObjectDetector (one ragged call over the live views, which share the query
plane, straight into matches0 / scores0) and ObjectMapper (image pairs through match_pairs) give bitwise what one forward per
view / pair gives.  The SuperGlue paths of both are the branches they were (tests/test_det_ragged.py, tests/test_map_ragged.py)."""
import numpy as np
import pytest
import torch

from onepose_amd import LocalFeatureObjectDetector, NearestNeighbour, ObjectMapper, synthetic
from test_det_module import DEV, K, PlantedExtractor, feats_of, frame, planted_descriptor_views

pytestmark = pytest.mark.gpu
CONF = {"distance_threshold": 0.7}      # a view of one keypoint has no second neighbour: no ratio test here


def detect(views, q, matcher, ragged):
    refs = [torch.zeros(1, 1, 480, 640, device=DEV) for _ in views]
    det = LocalFeatureObjectDetector(PlantedExtractor(views + [q]), matcher, ref_images=refs, iterations=500)
    det.ragged = ragged
    calls = []
    inner = matcher.engine.match_ragged
    matcher.engine.match_ragged = lambda *a, **k: (calls.append(len(a[2])), inner(*a, **k))[1]
    try:
        bbox, crop, K_crop, best = det.detect_device(frame(480, 640, 4)[1], K, crop_size=256)
    finally:
        del matcher.engine.match_ragged
    torch.cuda.synchronize()
    out = {"matches0": det.matches0, "scores0": det.scores0, "bbox": bbox, "crop": crop, "K_crop": K_crop, "best": best,
           **{k: det.last[k] for k in ("affine", "mask", "info", "boxes")}}
    return det, {k: v.clone() for k, v in out.items()}, calls


@pytest.mark.parametrize("n0", [[120, 257, 64, 200, 33], [120, 4, 0, 257, 1, 129]], ids=["all-live", "an-empty-view"])
def test_detector_ragged_views_equal_the_per_view_loop(n0):
    rs = np.random.RandomState(len(n0))
    q = feats_of(np.stack([rs.uniform(0, 639, 200), rs.uniform(0, 479, 200)], -1), 7)
    views = planted_descriptor_views(rs, q, n0, [min(n, 60) for n in n0])
    nn = NearestNeighbour(CONF)
    det_r, ragged, calls_r = detect(views, q, nn, True)
    det_l, loop, calls_l = detect(views, q, nn, False)
    assert calls_r == [sum(1 for n in n0 if n)] and calls_l == []           # one ragged call over the live views / the forward loop
    for k in loop:
        assert ragged[k].dtype == loop[k].dtype and ragged[k].cpu().numpy().tobytes() == loop[k].cpu().numpy().tobytes(), k
    m = ragged["matches0"].cpu().numpy()
    assert all((m[v, n:] == -1).all() for v, n in enumerate(n0))
    # the comparison is not empty: the planted pairs (identical descriptors) are matched, and the detector finds a box
    assert int((m >= 0).sum()) >= sum(min(n, 60) for n in n0 if n >= 33) * 9 // 10
    assert int(ragged["info"][:, 0].sum()) >= 3


COUNTS = [40, 300, 97, 257, 150, 64]
PAIRS = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (2, 4), (3, 4), (3, 5), (4, 5)]


def test_mapper_pair_batches_equal_the_per_pair_loop(tmp_path):
    s = synthetic.make_map_scene(n_points=420, n_views=6, hw=(96, 128), seed=3, dropout=0.1)
    feats = [{"keypoints": f["keypoints"][:n], "scores": f["scores"][:n], "descriptors": np.ascontiguousarray(f["descriptors"][:, :n]),
              "size": s["hw"]} for f, n in zip(s["features"], COUNTS)]
    nn = NearestNeighbour({"ratio_threshold": 0.9, "distance_threshold": 0.7})
    seen = {}
    for pb in (1, 4):
        mapper = ObjectMapper(matcher=nn, leaf_seed=5, device="cuda:0", pair_batch=pb)
        inner, seen[pb] = mapper.build_from_matches, []
        mapper.build_from_matches = lambda f, pm, *a, _inner=inner, _seen=seen[pb], **k: (_seen.extend(pm), _inner(f, pm, *a, **k))[1]
        mapper.build_from_features(feats, PAIRS, s["poses"], s["Ks"], s["box"], out_dir=str(tmp_path / f"pb{pb}"))
        seen[pb] = (mapper, seen[pb])
    (ref, ref_pm), (got, got_pm) = seen[1], seen[4]
    assert [(i, j) for i, j, _ in got_pm] == [(i, j) for i, j, _ in ref_pm] == PAIRS
    for (i, j, m), (_, _, r) in zip(got_pm, ref_pm):
        assert m.dtype == r.dtype == torch.int64 and m.shape == (COUNTS[i],) and torch.equal(m, r), (i, j)
    assert sum(int((m >= 0).sum()) for _, _, m in ref_pm) > 200
    for part in ("average", "collect"):
        for key, val in ref.last["anno"][part].items():
            assert got.last["anno"][part][key].tobytes() == val.tobytes(), (part, key)
