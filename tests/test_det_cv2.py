"""The oracle of the detector tail against OpenCV itself, where cv2 is importable (it is not where this was developed: these
tests are skipped there, and parity with OpenCV is NOT claimed anywhere).  They RECORD the differences -- printed with -s --
and assert only what the documented differences allow: the same transform up to the inlier noise, grey levels within the
effect of warpAffine's 1/32 px position grid.  tests/golden/make_det_golden.py records the same figures from the unmodified
reference into tests/golden/det_cv2_record.json."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import detector_oracle as do  # noqa: E402
from onepose_amd import detector  # noqa: E402,F401


@pytest.mark.parametrize("n,outliers,seed", [(40, 0.3, 1), (300, 0.5, 2), (2000, 0.6, 3)])
def test_estimate_affine_partial_against_cv2(n, outliers, seed):
    src, dst, A, _ = do.planted_matches(np.random.RandomState(seed), n, outliers)
    ok, est, mask, _, cnt = do.estimate_affine_partial(src, dst)
    ref, ref_mask = cv2.estimateAffinePartial2D(src, dst, ransacReprojThreshold=6)
    corners = np.abs(do.projected_corners(est, (480, 640)) - do.projected_corners(ref, (480, 640))).max()
    print(f"n={n}: inliers oracle {cnt} / cv2 {int(ref_mask.sum())}, masks differ at {int((mask != ref_mask[:, 0].astype(bool)).sum())}, "
          f"max |affine diff| {np.abs(est - ref).max():.3e}, projected corners differ by {corners:.3e} px")
    assert ok and ref_mask.shape == (n, 1)            # the N x 1 mask whose shape[0] the reference's vote ranks by
    assert corners < 6.0


@pytest.mark.parametrize("box", [(100, 80, 400, 330), (-60, 50, 200, 300), (300, 5, 380, 475)])
def test_crop_against_two_cv2_warps(box):
    img = np.random.RandomState(11).randint(0, 256, size=(480, 640)).astype(np.uint8)
    M1, M2 = do.crop_transforms(box, 512)
    w, h = box[2] - box[0], box[3] - box[1]
    stage1 = cv2.warpAffine(img, M1[:2], (w, h), flags=cv2.INTER_LINEAR)
    ref = cv2.warpAffine(stage1, M2[:2], (512, 512), flags=cv2.INTER_LINEAR)
    got = np.rint(do.crop_resize(img, box, 512) * 255)
    d = np.abs(got - ref.astype(np.float64))
    print(f"box {box}: grey levels differ at {int((d > 0).sum())} of {d.size} pixels, max {d.max():.0f}, mean {d.mean():.4f}")
    assert d.mean() < 8.0                              # white-noise image: 1/32 px of position moves a level by up to 255/32


def test_k_crop_against_cv2_get_affine_transform():
    K = np.array([[1063.2, 0.0, 318.7], [0.0, 1071.9, 243.1], [0.0, 0.0, 1.0]])
    worst = 0.0
    for box in [(10, 20, 300, 200), (-35, -8, 77, 401), (601, 333, 1234, 777)]:
        Kc, _, _ = do.k_crop_reference_route(box, K, 512, solve=lambda A, b: cv2.solve(A, b[:, None])[1][:, 0])
        worst = max(worst, float(np.abs(Kc - do.k_crop(box, K, 512)).max() / np.abs(Kc).max()))
    print(f"K_crop: closed form vs cv2.solve route, relative {worst:.3e}")
    assert worst < 1e-9
