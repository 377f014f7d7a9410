"""LocalFeatureObjectDetector with the native matcher: one ragged batch over the reference views gives bitwise what one
forward per view gives -- the padded matches0 / scores0 buffers and every output of detect_device."""
import numpy as np
import pytest
import torch

from onepose_amd import LocalFeatureObjectDetector, SuperGlue, synthetic
from test_det_module import DEV, K, PlantedExtractor, feats_of, frame, planted_descriptor_views

pytestmark = pytest.mark.gpu


def matcher():
    sd = synthetic.make_superglue_passthrough_state_dict(6, 2)
    sg = SuperGlue({"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "match_threshold": 0.7}).eval()
    sg.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return sg


def run(views, sizes, q, sg, ragged):
    refs = [torch.zeros(1, 1, *hw, device=DEV) for hw in sizes]
    det = LocalFeatureObjectDetector(PlantedExtractor(views + [q]), sg, ref_images=refs, iterations=500)
    det.ragged = ragged
    _, img = frame(480, 640, 4)
    bbox, crop, K_crop, best = det.detect_device(img, K, crop_size=256)
    torch.cuda.synchronize()
    out = {"matches0": det.matches0, "scores0": det.scores0, "bbox": bbox, "crop": crop, "K_crop": K_crop, "best": best,
           **{k: det.last[k] for k in ("affine", "mask", "info", "boxes")}}
    return det, {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("V", [1, 15])
def test_ragged_views_equal_the_per_view_loop(V):
    rs = np.random.RandomState(20 + V)
    q = feats_of(np.stack([rs.uniform(0, 639, 200), rs.uniform(0, 479, 200)], -1), 7)
    n0 = [257] if V == 1 else [120, 4, 0, 257, 64, 65, 1, 129, 200, 33, 257, 90, 128, 17, 250]      # an empty view; two at cap0
    planted = [min(n, 60) for n in n0]
    views = planted_descriptor_views(rs, q, n0, planted)
    sizes = [[(480, 640), (640, 480), (96, 128), (700, 300)][v % 4] for v in range(V)]
    sg = matcher()
    det_r, ragged = run(views, sizes, q, sg, True)
    det_l, loop = run(views, sizes, q, sg, False)
    assert det_r.cap0 == 257 and det_r.live == [v for v in range(V) if n0[v]] and det_r.view_desc.shape == (V, 256, 257)
    for k in loop:
        assert ragged[k].dtype == loop[k].dtype and ragged[k].cpu().numpy().tobytes() == loop[k].cpu().numpy().tobytes(), k
    m = ragged["matches0"].cpu().numpy()
    assert all((m[v, n0[v]:] == -1).all() for v in range(V))
    # the comparison is not empty: at least half of the pairs planted in the larger views are matched
    assert int((m >= 0).sum()) > sum(p for n, p in zip(n0, planted) if n >= 60) // 2
