"""Numpy fp64 restatement of the 2D object detector's tail (src/local_feature_2D_detector/local_feature_2D_detector.py:85-147,
160-186 and src/utils/data_utils.py:24-57,233-272), written from the math: match selection, partial-affine RANSAC, box vote,
crop and K_crop.  It is the yardstick of the HIP library behind include/detector/detector.h and restates every expression in the
same order (numpy never fuses a multiply with an add), with the same counter-based hash, so hypothesis indices, inlier masks,
boxes and crop bits are comparable exactly.  ``ld`` variants evaluate in numpy.longdouble: they measure this oracle's own error.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import ransac_common
from oracle.ransac_common import lane_tree_sum

F64 = np.float64
MIN_MATCHES = 6            # local_feature_2D_detector.py:93
REPROJ_THRESHOLD = 6.0     # :105
ITERATIONS = 2000          # OpenCV's default maxIters of estimateAffinePartial2D
REFIT_LANES = 256          # the refit's reduction order: lane t sums the inliers t, t + 256, ..., then a binary tree over lanes
# sample_indices(seed, hyp, n): the two matches of hypothesis `hyp` (the pose solver's sampler, for minimal sets of 2)
sample_indices = functools.partial(ransac_common.sample_indices, k=2)


@functools.lru_cache(maxsize=64)
def all_samples(seed, iterations, n):
    return np.array([sample_indices(seed, h, n) for h in range(iterations)], dtype=np.int64).reshape(iterations, 2)


def select_matches(kpts0, kpts1, matches0):
    """:85-90 -> (mkpts0 [m,2], mkpts1 [m,2], index of each match in kpts0); entries >= len(kpts1) count as unmatched."""
    matches0 = np.asarray(matches0)
    valid = (matches0 > -1) & (matches0 < len(kpts1))
    return np.asarray(kpts0)[valid], np.asarray(kpts1).reshape(-1, 2)[matches0[valid]], np.nonzero(valid)[0]


def models_from_pairs(src, dst, pairs, dt=F64):
    """Partial affine through two matches, vectorised over hypotheses -> (a, b, tx, ty, valid)."""
    p, q = pairs[:, 0], pairs[:, 1]
    s, d = src.astype(dt), dst.astype(dt)
    sx, sy = s[q, 0] - s[p, 0], s[q, 1] - s[p, 1]
    dx, dy = d[q, 0] - d[p, 0], d[q, 1] - d[p, 1]
    den = sx * sx + sy * sy
    valid = den > 0
    safe = np.where(valid, den, dt(1))
    a = (dx * sx + dy * sy) / safe
    b = (dy * sx - dx * sy) / safe
    tx = d[p, 0] - (a * s[p, 0] - b * s[p, 1])
    ty = d[p, 1] - (b * s[p, 0] + a * s[p, 1])
    return a, b, tx, ty, valid


def residual2(a, b, tx, ty, src, dst, dt=F64):
    """Squared reprojection error; model parameters broadcast against the points."""
    x, y = src[:, 0].astype(dt), src[:, 1].astype(dt)
    ex = ((a * x - b * y) + tx) - dst[:, 0].astype(dt)
    ey = ((b * x + a * y) + ty) - dst[:, 1].astype(dt)
    return ex * ex + ey * ey


def refit(src, dst, mask, dt=F64):
    """Closed-form least squares of x' = [[a,-b],[b,a]] x + t over the inliers (centroids, two dot-product sums): the fixed
    point of the Levenberg-Marquardt refinement OpenCV runs.  -> 2x3 [[a, -b, tx], [b, a, ty]]."""
    s, d = src.astype(dt), dst.astype(dt)
    m = mask.astype(bool)
    z = dt(0)
    cnt = dt(int(m.sum()))
    csx = lane_tree_sum(np.where(m, s[:, 0], z), REFIT_LANES) / cnt
    csy = lane_tree_sum(np.where(m, s[:, 1], z), REFIT_LANES) / cnt
    cdx = lane_tree_sum(np.where(m, d[:, 0], z), REFIT_LANES) / cnt
    cdy = lane_tree_sum(np.where(m, d[:, 1], z), REFIT_LANES) / cnt
    ux, uy, wx, wy = s[:, 0] - csx, s[:, 1] - csy, d[:, 0] - cdx, d[:, 1] - cdy
    suu = lane_tree_sum(np.where(m, ux * ux + uy * uy, z), REFIT_LANES)
    sdot = lane_tree_sum(np.where(m, ux * wx + uy * wy, z), REFIT_LANES)
    scr = lane_tree_sum(np.where(m, ux * wy - uy * wx, z), REFIT_LANES)
    a, b = sdot / suu, scr / suu
    return np.array([[a, -b, cdx - (a * csx - b * csy)], [b, a, cdy - (b * csx + a * csy)]], dtype=dt)


def estimate_affine_partial(src, dst, thr=REPROJ_THRESHOLD, iterations=ITERATIONS, seed=0, min_matches=2, return_debug=False):
    """cv2.estimateAffinePartial2D restated (see include/detector/detector.h for the three documented differences).
    src, dst [n,2] float32.  -> (ok, affine 2x3 float64, mask [n] bool, best hypothesis index, its inlier count)."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 2), np.asarray(dst, np.float32).reshape(-1, 2)
    n = len(src)
    fail = (False, np.zeros((2, 3)), np.zeros(n, bool), -1, 0) + ((None,) if return_debug else ())
    if n < max(2, min_matches):
        return fail
    pairs = all_samples(seed, iterations, n)
    a, b, tx, ty, valid = models_from_pairs(src, dst, pairs)
    thr2 = F64(thr) * F64(thr)
    counts = np.zeros(iterations, np.int64)
    step = max(1, (1 << 22) // n)
    for h0 in range(0, iterations, step):
        sl = slice(h0, h0 + step)
        r = residual2(a[sl, None], b[sl, None], tx[sl, None], ty[sl, None], src, dst)
        counts[sl] = (r <= thr2).sum(axis=1)
    counts[~valid] = -1
    best = int(np.argmax(counts))               # first arg-max: the lowest hypothesis index on ties
    if counts[best] < 0:
        return fail
    res = residual2(a[best], b[best], tx[best], ty[best], src, dst)
    mask = res <= thr2
    out = (True, refit(src, dst, mask), mask, best, int(mask.sum()))
    if return_debug:
        out += (dict(counts=counts, pairs=pairs, residuals=res, thr2=thr2),)
    return out


def view_box(affine, ok, hw0, query_hw):
    """:96-99 and :108-131 -> [x0, y0, x1, y1] int32."""
    if not ok:
        return np.array([0, 0, query_hw[0], query_hw[1]], dtype=np.int32)       # as written: x1 = H, y1 = W
    h0, w0 = F64(hw0[0]), F64(hw0[1])
    cx, cy = np.array([0, w0, 0, w0], F64), np.array([0, 0, h0, h0], F64)
    A = np.asarray(affine, F64)
    px = (A[0, 0] * cx + A[0, 1] * cy) + A[0, 2]
    py = (A[1, 0] * cx + A[1, 1] * cy) + A[1, 2]
    pts = np.stack([px, py], -1)
    ints = np.clip(pts, -2147483648.0, 2147483647.0).astype(np.int32)          # truncation toward zero
    return np.concatenate([ints.min(axis=0), ints.max(axis=0)]).astype(np.int32)


def projected_corners(affine, hw0):
    h0, w0 = F64(hw0[0]), F64(hw0[1])
    cx, cy = np.array([0, w0, 0, w0], F64), np.array([0, 0, h0, h0], F64)
    A = np.asarray(affine, F64)
    return np.stack([(A[0, 0] * cx + A[0, 1] * cy) + A[0, 2], (A[1, 0] * cx + A[1, 1] * cy) + A[1, 2]], -1)


def vote(oks, n_matches, n_inliers, rank_by="matches"):
    """:139-147 as written: sorted(reverse=True) is stable, the key is inliers.shape[0] of cv2's N x 1 mask = the number of
    MATCHES (0 for a failed view).  rank_by='inliers' is the documented deviation."""
    keys = [(int(nm) if rank_by == "matches" else int(ni)) if ok else 0 for ok, nm, ni in zip(oks, n_matches, n_inliers)]
    order = [k for k, _ in sorted(enumerate(keys), reverse=True, key=lambda item: item[1])]
    return order[0]


def detect_tail(kpts0_list, matches0_list, kpts1, hw0_list, query_hw, thr=REPROJ_THRESHOLD, iterations=ITERATIONS, seed=0,
                rank_by="matches"):
    """match_worker + detect_by_matching for the views given as lists -> dict(bbox, best_view, boxes, affine, info, masks)."""
    V = len(kpts0_list)
    aff, info, boxes, masks = np.zeros((V, 2, 3)), np.zeros((V, 4), np.int32), np.zeros((V, 4), np.int32), []
    for v in range(V):
        m0, m1, idx = select_matches(kpts0_list[v], kpts1, matches0_list[v])
        ok, A, mask, best, cnt = estimate_affine_partial(m0, m1, thr, iterations, seed, MIN_MATCHES)
        full = np.zeros(len(kpts0_list[v]), np.int32)
        full[idx[mask]] = 1
        masks.append(full)
        aff[v], info[v] = A, (int(ok), len(m0), best, cnt)
        boxes[v] = view_box(A, ok, hw0_list[v], query_hw)
    bv = vote(info[:, 0], info[:, 1], info[:, 3], rank_by)
    return dict(bbox=boxes[bv].copy(), best_view=bv, boxes=boxes, affine=aff, info=info, masks=masks)


# ---- crop and K_crop -------------------------------------------------------------------------------------
def crop_transforms(bbox, crop):
    """Closed form of the two get_affine_transform calls of crop_img_by_bbox with rot = 0 -> (M1, M2) 3x3 float64."""
    x0, y0, x1, y1 = (F64(int(t)) for t in bbox)
    w, h = x1 - x0, y1 - y0
    s = F64(crop) / w
    M1 = np.array([[1, 0, -x0], [0, 1, -y0], [0, 0, 1]], F64)
    M2 = np.array([[s, 0, 0], [0, s, F64(0.5) * F64(crop) - s * (F64(0.5) * h)], [0, 0, 1]], F64)
    return M1, M2


def k_crop(bbox, K, crop):
    """K_crop = M2 M1 K in the kernel's closed form and order."""
    x0, y0, x1, y1 = (F64(int(t)) for t in bbox)
    w, h = x1 - x0, y1 - y0
    K = np.asarray(K, F64).reshape(3, 3)
    s = F64(crop) / w
    m02 = -(s * x0)
    m12 = (F64(0.5) * F64(crop) - s * (F64(0.5) * h)) - s * y0
    return np.stack([s * K[0] + m02 * K[2], s * K[1] + m12 * K[2], K[2]])


def get_affine_transform_3pt(center, scale, output_size, dt=F64, solve=None):
    """data_utils.get_affine_transform (:24-57) with rot = 0, shift = 0, inv = 0, restated: its three-point construction in
    float32 and the 6-unknown linear system cv2.getAffineTransform solves, here with numpy.linalg.solve (or `solve`)."""
    src_w, dst_w, dst_h = scale[0], output_size[0], output_size[1]
    src_dir = np.array([0.0, src_w * -0.5])
    dst_dir = np.array([0, dst_w * -0.5], np.float32)
    src, dst = np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32)
    src[0] = center
    src[1] = np.asarray(center) + src_dir
    dst[0] = [dst_w * 0.5, dst_h * 0.5]
    dst[1] = np.array([dst_w * 0.5, dst_h * 0.5], np.float32) + dst_dir
    for pts in (src, dst):
        direct = pts[0] - pts[1]
        pts[2] = pts[1] + np.array([-direct[1], direct[0]], dtype=np.float32)
    A, rhs = np.zeros((6, 6), dt), np.zeros(6, dt)
    for i in range(3):
        A[2 * i, 0:3] = (src[i, 0], src[i, 1], 1)
        A[2 * i + 1, 3:6] = (src[i, 0], src[i, 1], 1)
        rhs[2 * i], rhs[2 * i + 1] = dst[i, 0], dst[i, 1]
    x = (solve or np.linalg.solve)(A, rhs)
    return x.reshape(2, 3)


def gauss_solve(A, b):
    """Gaussian elimination with partial pivoting in the dtype of A (numpy.linalg has no longdouble)."""
    A, b = A.copy(), b.copy()
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] = A[i, k:] - f * A[k, k:]
            b[i] = b[i] - f * b[k]
    x = np.zeros(n, A.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - (A[k, k + 1:] * x[k + 1:]).sum()) / A[k, k]
    return x


def k_crop_reference_route(bbox, K, crop, dt=F64, solve=None):
    """crop_img_by_bbox's two get_K_crop_resize calls (:174-183) through the three-point construction -> (K_crop, M1, M2)."""
    x0, y0, x1, y1 = (int(t) for t in bbox)
    K = np.asarray(K, dt).reshape(3, 3)
    Ms = []
    for box, (rh, rw) in (((x0, y0, x1, y1), (y1 - y0, x1 - x0)), ((0, 0, x1 - x0, y1 - y0), (crop, crop))):
        center = np.array([(box[0] + box[2]) / 2., (box[1] + box[3]) / 2.])
        scale = np.array([box[2] - box[0], box[3] - box[1]])
        T = get_affine_transform_3pt(center, scale, [rw, rh], dt, solve)
        Ms.append(np.concatenate([T, np.array([[0, 0, 1]], dt)], axis=0))
        K = Ms[-1] @ K
    return K, Ms[0], Ms[1]


def to_u8(image):
    """The detector's uint8 plane of an fp32 frame in [0, 1]: rint(x * 255) (exact for frames that were u8 / 255)."""
    return np.clip(np.rint(np.asarray(image, np.float32) * np.float32(255)), 0, 255).astype(np.uint8)


def _crop_samples(img_u8, bbox, crop):
    H, W = img_u8.shape
    x0, y0, x1, y1 = (int(t) for t in bbox)
    w, h = x1 - x0, y1 - y0
    u = np.arange(crop, dtype=np.int64)[None, :]
    v = np.arange(crop, dtype=np.int64)[:, None]
    Xs = np.broadcast_to(u * w, (crop, crop))
    Ys = np.broadcast_to((v - crop // 2) * w + h * (crop // 2), (crop, crop))
    ix, iy = Xs // crop, Ys // crop
    fx, fy = Xs - ix * crop, Ys - iy * crop

    def tap(x, y):
        X, Y = x + x0, y + y0
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h) & (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
        return np.where(inside, img_u8[np.clip(Y, 0, H - 1), np.clip(X, 0, W - 1)].astype(np.int64), 0)

    return fx, fy, (tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1))


def crop_resize(img_u8, bbox, crop):
    """Both warps of crop_img_by_bbox as one exact-integer bilinear resampling -> float32 [crop, crop] = level / 255."""
    assert crop >= 2 and crop & (crop - 1) == 0, "crop_size must be a power of two"
    x0, y0, x1, y1 = (int(t) for t in bbox)
    if x1 - x0 <= 0 or y1 - y0 <= 0:
        return np.zeros((crop, crop), np.float32)
    fx, fy, (p00, p10, p01, p11) = _crop_samples(np.asarray(img_u8), bbox, crop)
    total = (crop - fx) * (crop - fy) * p00 + fx * (crop - fy) * p10 + (crop - fx) * fy * p01 + fx * fy * p11
    c2 = crop * crop
    q, r = total // c2, total % c2
    q = q + ((r > c2 // 2) | ((r == c2 // 2) & (q % 2 == 1)))
    return q.astype(np.float32) / np.float32(255)


def crop_resize_float(img_u8, bbox, crop):
    """The same resampling as a plain fp64 bilinear evaluation (no rounding) -> (levels float64 [crop, crop], ties bool)."""
    fx, fy, (p00, p10, p01, p11) = _crop_samples(np.asarray(img_u8), bbox, crop)
    ax, ay = fx.astype(F64) / crop, fy.astype(F64) / crop
    val = (1 - ax) * (1 - ay) * p00 + ax * (1 - ay) * p10 + (1 - ax) * ay * p01 + ax * ay * p11
    return val, (val - np.floor(val)) == 0.5


def reproj(K, pose, pts_3d):
    """vis_utils.reproj (:209-236): K [3,3], pose [3,4] or [4,4], pts_3d [n,3] -> [n,2]."""
    K, pose = np.asarray(K, F64), np.asarray(pose, F64)
    pts = np.concatenate([np.asarray(pts_3d, F64).reshape(-1, 3), np.ones((len(pts_3d), 1))], axis=1).T
    p = K @ pose[:3] @ pts
    return (p[:2] / p[2:]).T


def pose_box(K, pose, bbox3d_corner):
    """previous_pose_detect (:246-250) -> [x0, y0, x1, y1] int32."""
    p = reproj(K, pose, bbox3d_corner)
    x0, y0 = p.min(axis=0)
    x1, y1 = p.max(axis=0)
    return np.array([x0, y0, x1, y1]).astype(np.int32)


# ---- planted cases ---------------------------------------------------------------------------------------
def planted_matches(rs, n, outlier_frac, hw0=(480, 640), angle=None, scale=None, shift=None, noise=0.5):
    """n matches of a planted similarity: src uniform in the reference view, dst = s R src + t + noise; a fraction replaced by
    uniform outliers.  float32, rounded as the extractor's pixel coordinates are not (sub-pixel noise kept)."""
    angle = rs.uniform(-np.pi, np.pi) if angle is None else angle
    scale = float(np.exp(rs.uniform(np.log(0.3), np.log(3.0)))) if scale is None else scale
    shift = rs.uniform(-200, 400, size=2) if shift is None else np.asarray(shift, F64)
    a, b = scale * np.cos(angle), scale * np.sin(angle)
    A = np.array([[a, -b, shift[0]], [b, a, shift[1]]])
    src = np.stack([rs.uniform(0, hw0[1] - 1, n), rs.uniform(0, hw0[0] - 1, n)], -1)
    dst = src @ A[:, :2].T + A[:, 2] + rs.normal(0, noise, size=(n, 2))
    out = rs.permutation(n)[:int(round(outlier_frac * n))]
    lo, hi = dst.min(axis=0) - 50, dst.max(axis=0) + 50
    dst[out] = rs.uniform(lo, hi, size=(len(out), 2))
    is_outlier = np.zeros(n, bool)
    is_outlier[out] = True
    return src.astype(np.float32), dst.astype(np.float32), A, is_outlier


def exactness_conditions(dbg, best, affine, hw0, margin=1e-6):
    """What keeps an exact comparison with another fp64 implementation honest: (no residual of the winner within `margin` px^2
    of thr^2, the best hypothesis drawn from another pair of matches has strictly fewer inliers, no projected corner within
    `margin` of an integer).  Hypotheses that drew the winner's own pair, in either order, are the same model up to rounding
    (~1e-13 px): with the first condition they count the same inliers in any fp64 arithmetic, and the lowest index wins."""
    res_ok = bool(np.all(np.abs(dbg["residuals"] - dbg["thr2"]) > margin))
    pair = set(dbg["pairs"][best].tolist())
    other = np.array([set(p.tolist()) != pair for p in dbg["pairs"]])
    runner = int(dbg["counts"][other].max()) if other.any() else -1
    runner_ok = runner < int(dbg["counts"][best])
    c = projected_corners(affine, hw0)
    corner_ok = bool(np.all(np.abs(c - np.rint(c)) > margin))
    return res_ok, runner_ok, corner_ok
