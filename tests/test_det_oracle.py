"""The detector tail's numpy oracle (tests/detector_oracle.py) against planted data and against direct restatements of the
reference's constructions; CPU only.  Importing onepose_amd.detector ties these tests to the feature."""
import os

import numpy as np
import pytest

import detector_oracle as do
from onepose_amd import detector  # noqa: F401  (the feature under test; its COLMAP name reader is tested below)


@pytest.mark.parametrize("n,outliers,seed", [(6, 0.2, 1), (7, 0.3, 2), (40, 0.5, 3), (64, 0.7, 4), (300, 0.2, 5), (1025, 0.6, 6),
                                             (4096, 0.7, 7), (4096, 0.45, 8)])
def test_oracle_recovers_planted_similarity_and_box(n, outliers, seed):
    rs = np.random.RandomState(seed)
    hw0 = (480, 640)
    src, dst, A, is_out = do.planted_matches(rs, n, outliers, hw0)
    ok, est, mask, best, cnt = do.estimate_affine_partial(src, dst, seed=seed)
    assert ok and cnt == mask.sum() and best >= 0
    n_in = int((~is_out).sum())
    assert mask[~is_out].sum() >= 0.95 * n_in - 1, (mask[~is_out].sum(), n_in)
    # the refit over >= 4 inliers with 0.5 px noise: corners of the view land within a few pixels of the planted ones
    tol = 12.0 / np.sqrt(max(n_in, 1)) + 0.6 if n_in >= 12 else 8.0
    assert np.abs(do.projected_corners(est, hw0) - do.projected_corners(A, hw0)).max() < tol * max(1.0, np.hypot(A[0, 0], A[1, 0]))
    box, planted = do.view_box(est, True, hw0, (480, 640)), do.view_box(A, True, hw0, (480, 640))
    assert np.abs(box.astype(np.int64) - planted).max() <= np.ceil(tol * max(1.0, np.hypot(A[0, 0], A[1, 0]))) + 1


def test_sampler_gives_distinct_reproducible_pairs():
    p = do.all_samples(3, 500, 2)
    assert set(map(tuple, p.tolist())) == {(0, 1), (1, 0)}
    p = do.all_samples(0, 2000, 4096)
    assert (p[:, 0] != p[:, 1]).all() and p.min() >= 0 and p.max() < 4096
    assert do.sample_indices(0, 17, 4096) == p[17].tolist()
    assert (do.all_samples(1, 2000, 4096) != p).any()


def test_degenerate_samples_are_skipped_and_all_degenerate_fails():
    src = np.array([[5, 5]] * 6 + [[10, 20], [30, 5]], np.float32)
    dst = src * 2 + 3
    ok, A, mask, best, cnt = do.estimate_affine_partial(src, dst, iterations=200)
    assert ok and cnt == 8 and np.allclose(A, [[2, 0, 3], [0, 2, 3]], atol=1e-9)
    pair = do.sample_indices(0, best, 8)
    assert (src[pair[0]] != src[pair[1]]).any()
    ok, A, mask, best, cnt = do.estimate_affine_partial(np.full((8, 2), 5, np.float32), dst)
    assert not ok and best == -1 and cnt == 0 and not mask.any() and (A == 0).all()


def test_refit_is_the_least_squares_fixed_point():
    rs = np.random.RandomState(0)
    src, dst, A, _ = do.planted_matches(rs, 500, 0.0, noise=1.0)
    est = do.refit(src, dst, np.ones(500, bool))
    # normal equations of min sum |a x - b y + tx - x'|^2 + |b x + a y + ty - y'|^2 with numpy.linalg.lstsq
    x, y = src[:, 0].astype(float), src[:, 1].astype(float)
    M = np.concatenate([np.stack([x, -y, np.ones_like(x), np.zeros_like(x)], -1), np.stack([y, x, np.zeros_like(x), np.ones_like(x)], -1)])
    sol = np.linalg.lstsq(M, np.concatenate([dst[:, 0], dst[:, 1]]).astype(float), rcond=None)[0]
    assert np.allclose([est[0, 0], est[1, 0], est[0, 2], est[1, 2]], sol, rtol=1e-9, atol=1e-9)
    ld = do.refit(src, dst, np.ones(500, bool), np.longdouble)
    assert float(np.abs(est - ld).max()) < 1e-11


BOXES = [(10, 20, 300, 200), (0, 0, 640, 480), (-35, -8, 77, 401), (100, 50, 101, 460), (3, 7, 500, 8), (-100, -100, 900, 700),
         (15, 9, 272, 266), (601, 333, 1234, 777), (2, 3, 5, 11)]


def test_closed_form_transforms_against_the_three_point_construction():
    """M1, M2 and K_crop in closed form against get_affine_transform's three-point construction solved with numpy.linalg.solve.
    Bound: 4 x the disagreement of the solve route with itself in longdouble (both relative to the largest entry), taken over
    all boxes and crop sizes below.  Recorded on x86-64: route disagreement 4.19e-14 relative, closed form vs route 4.19e-14
    (the difference is the fp64 solve's own rounding on the 6 x 6 system; the closed form is the more accurate of the two)."""
    K = np.array([[1063.2, 0.0, 318.7], [0.0, 1071.9, 243.1], [0.0, 0.0, 1.0]])
    worst_route, worst_closed = 0.0, 0.0
    for crop in (256, 512):
        for box in BOXES:
            Kc, M1, M2 = do.k_crop_reference_route(box, K, crop)
            Kl, M1l, M2l = do.k_crop_reference_route(box, K, crop, np.longdouble, do.gauss_solve)
            c1, c2 = do.crop_transforms(box, crop)
            for ours, route, ld in ((c1, M1, M1l), (c2, M2, M2l), (do.k_crop(box, K, crop), Kc, Kl)):
                scale = float(np.abs(ld).max())
                worst_route = max(worst_route, float(np.abs(route - ld).max()) / scale)
                worst_closed = max(worst_closed, float(np.abs(ours - route).max()) / scale)
    print(f"three-point route vs itself in longdouble: {worst_route:.3e} relative; closed form vs route: {worst_closed:.3e}")
    assert worst_route > 0
    assert worst_closed <= 4 * worst_route


def test_vote_ranks_by_match_count_and_keeps_the_first_view_on_ties():
    assert do.vote([1, 1, 1], [50, 80, 80], [40, 10, 70]) == 1                      # matches, first among equals
    assert do.vote([1, 1, 1], [50, 80, 80], [40, 10, 70], rank_by="inliers") == 2   # the documented deviation
    assert do.vote([0, 1, 1], [5, 9, 9], [0, 9, 3]) == 1                            # a failed view counts 0
    assert do.vote([0, 0, 0], [5, 0, 3], [0, 0, 0]) == 0                            # all views fail: the first one
    rs = np.random.RandomState(3)
    kpts1 = rs.uniform(0, 600, (50, 2)).astype(np.float32)
    k0 = [rs.uniform(0, 300, (20, 2)).astype(np.float32) for _ in range(3)]
    few = np.full(20, -1, np.int64)
    few[:5] = np.arange(5)
    out = do.detect_tail(k0, [few, few.copy(), few.copy()], kpts1, [(300, 400)] * 3, (480, 640))
    assert out["bbox"].tolist() == [0, 0, 480, 640] and out["best_view"] == 0       # :98 as written: x1 = H, y1 = W
    assert (out["info"][:, 0] == 0).all() and (out["info"][:, 1] == 5).all()
    # one view with a planted transform wins over a failed one that comes first
    src, dst, A, _ = do.planted_matches(rs, 40, 0.2, (300, 400), angle=0.2, scale=1.3, shift=(50, 60))
    m = np.arange(40, dtype=np.int64)
    out = do.detect_tail([k0[0], src], [few, m], dst, [(300, 400)] * 2, (480, 640))
    assert out["best_view"] == 1 and out["info"][1, 0] == 1 and out["info"][1, 1] == 40
    assert out["bbox"].tolist() == do.view_box(out["affine"][1], True, (300, 400), (480, 640)).tolist()
    assert out["masks"][1].sum() == out["info"][1, 3]


def test_integer_crop_equals_fp64_bilinear_except_at_exact_ties():
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, size=(120, 160)).astype(np.uint8)
    ties_total = 0
    for crop in (64, 256):
        for box in [(10, 20, 100, 90), (-20, -10, 200, 150), (30, 5, 31, 110), (5, 40, 150, 41), (0, 0, 160, 120), (8, 8, 72, 72),
                    (100, 60, 228, 188)]:
            got = do.crop_resize(img, box, crop)
            val, ties = do.crop_resize_float(img, box, crop)
            lv = np.rint(got.astype(np.float64) * 255)
            assert np.array_equal(got, (lv.astype(np.float32) / np.float32(255)))
            assert np.array_equal(lv[~ties], np.rint(val[~ties]))
            assert np.array_equal(lv[ties], np.rint(val[ties]))          # numpy's rint is half-to-even as well
            assert (np.abs(lv - val) <= 0.5).all()
            ties_total += int(ties.sum())
    print(f"exact .5 ties met: {ties_total}")
    assert ties_total > 0
    # a 1:1 box is the exact crop; zero outside the image
    got = do.crop_resize(img, (16, 8, 80, 72), 64)
    assert np.array_equal(np.rint(got * 255).astype(np.uint8), img[8:72, 16:80])
    got = do.crop_resize(img, (-32, -32, 32, 32), 64)
    assert (got[:32] == 0).all() and (got[:, :32] == 0).all() and np.array_equal(np.rint(got[32:, 32:] * 255), img[:32, :32])
    assert (do.crop_resize(img, (5, 5, 5, 50), 64) == 0).all()
    with pytest.raises(AssertionError):
        do.crop_resize(img, (0, 0, 10, 10), 300)


def test_letterbox_geometry_of_a_wide_and_a_tall_box():
    img = np.full((100, 200), 200, np.uint8)
    wide = do.crop_resize(img, (0, 25, 200, 75), 64)            # w = 200, h = 50: rows 24..39 hold the object
    assert (wide[:23] == 0).all() and (wide[41:] == 0).all() and np.allclose(wide[26:38], 200 / 255)
    tall = do.crop_resize(img, (75, 0, 125, 100), 64)           # w = 50, h = 100: scale 64/50, rows cut
    assert np.allclose(tall[:, :63], 200 / 255)                  # column 63 samples x = 49.2: blended with the zero border at x = 50
    assert np.allclose(tall[:, 63], np.rint(200 * (1 - 63 * 50 / 64 % 1)) / 255)


def test_colmap_image_names_from_text_and_binary(tmp_path):
    txt = tmp_path / "images.txt"
    txt.write_text("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                   "# Number of images: 3\n"
                   "2 1 0 0 0 0.1 0.2 0.3 1 color/b frame.png\n10.5 20.5 -1 30 40 7\n"
                   "1 1 0 0 0 0 0 0 1 color/a.png\n\n"
                   "3 0.5 0.5 0.5 0.5 1 2 3 1 color/c.png\n1 2 3\n")
    names = detector.read_colmap_image_names(str(tmp_path))
    assert names == {2: "color/b frame.png", 1: "color/a.png", 3: "color/c.png"}
    import struct
    os.remove(txt)
    with open(tmp_path / "images.bin", "wb") as f:
        f.write(struct.pack("<Q", 2))
        for iid, name, npts in ((7, b"x/7.png", 2), (4, b"y.png", 0)):
            f.write(struct.pack("<I7dI", iid, 1, 0, 0, 0, 0, 0, 0, 1) + name + b"\0" + struct.pack("<Q", npts))
            f.write(b"".join(struct.pack("<ddq", 1.0, 2.0, -1) for _ in range(npts)))
    assert detector.read_colmap_image_names(str(tmp_path)) == {7: "x/7.png", 4: "y.png"}
    assert detector.sample_reference_ids({i: str(i) for i in range(1, 31)}, 15) == list(range(1, 30, 2))
    with pytest.raises(FileNotFoundError):
        detector.read_colmap_image_names(str(tmp_path / "nope"))
