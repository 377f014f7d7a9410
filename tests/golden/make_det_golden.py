"""Record what OpenCV and the unmodified reference give on the detector tail's seeded cases, next to the oracle's results.

    python tests/golden/make_det_golden.py --reference /path/to/OnePose     (needs cv2; the reference is imported, not copied)

Writes tests/golden/det_cv2_record.json: per case the inlier counts, the largest difference of the transforms and of the
projected corners, the grey-level differences of the crop and the K_crop difference against the reference's
get_K_crop_resize / get_image_crop_resize.  Nothing here has been run where the detector was developed (no cv2): parity with
OpenCV is unpinned until this file exists.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import detector_oracle as do  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (imported unmodified)")
    a = ap.parse_args()
    import cv2
    sys.path.insert(0, a.reference)
    from src.utils.data_utils import get_image_crop_resize, get_K_crop_resize
    rec = {"cv2": cv2.__version__, "affine": [], "crop": []}
    for n, outliers, seed in [(40, 0.3, 1), (300, 0.5, 2), (2000, 0.6, 3), (4096, 0.7, 4)]:
        src, dst, _, _ = do.planted_matches(np.random.RandomState(seed), n, outliers)
        ok, est, mask, best, cnt = do.estimate_affine_partial(src, dst)
        ref, ref_mask = cv2.estimateAffinePartial2D(src, dst, ransacReprojThreshold=6)
        rec["affine"].append({"n": n, "outliers": outliers, "seed": seed, "oracle_inliers": cnt, "cv2_inliers": int(ref_mask.sum()),
                              "masks_differ": int((mask != ref_mask[:, 0].astype(bool)).sum()),
                              "max_abs_affine_diff": float(np.abs(est - ref).max()),
                              "max_corner_diff_px": float(np.abs(do.projected_corners(est, (480, 640)) -
                                                                 do.projected_corners(ref, (480, 640))).max())})
    img = np.random.RandomState(11).randint(0, 256, size=(480, 640)).astype(np.uint8)
    K = np.array([[1063.2, 0.0, 318.7], [0.0, 1071.9, 243.1], [0.0, 0.0, 1.0]])
    for box in [(100, 80, 400, 330), (-60, 50, 200, 300), (300, 5, 380, 475), (20, 200, 620, 300)]:
        x0, y0, x1, y1 = box
        b = np.array(box)
        K1, _ = get_K_crop_resize(b, K, np.array([y1 - y0, x1 - x0]))
        c1, _ = get_image_crop_resize(img, b, np.array([y1 - y0, x1 - x0]))
        b2 = np.array([0, 0, x1 - x0, y1 - y0])
        K2, _ = get_K_crop_resize(b2, K1, np.array([512, 512]))
        c2, _ = get_image_crop_resize(c1, b2, np.array([512, 512]))
        d = np.abs(np.rint(do.crop_resize(img, box, 512) * 255) - c2.astype(np.float64))
        rec["crop"].append({"box": list(box), "levels_differing": int((d > 0).sum()), "max_level_diff": float(d.max()),
                            "mean_level_diff": float(d.mean()),
                            "k_crop_rel_diff": float(np.abs(K2 - do.k_crop(box, K, 512)).max() / np.abs(K2).max())})
    with open(os.path.join(HERE, "det_cv2_record.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
