"""Numpy restatement of the object database builder (include/mapping/mapping.h; reference: src/sfm/pairs_from_poses.py,
src/sfm/postprocess/filter_tkl.py, filter_points.py, feature_process.py), written from the math.  It is the yardstick of
libmap_hip.so and restates every expression in the kernels' order (numpy never fuses a multiply with an add), with the same
counter-based hash and the same fixed-order sums, so survivors, hypothesis indices, inlier masks, kept ids, merged members and
gathered descriptors are comparable exactly.  ``dtype=np.longdouble`` evaluates the refit in extended precision: it measures
this oracle's own error.  The post-processing stages are pinned on outputs of the reference itself
(tests/golden/map_post.npz); verification and triangulation replace COLMAP and are pinned on nothing.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.ransac_common import lane_tree_sum, sample_indices

F64 = np.float64
MAX_EPIPOLAR_ERROR = 4.0
MIN_PAIR_INLIERS = 15
MAX_REPROJ_ERROR = 4.0
MIN_TRI_ANGLE = 1.5
MAX_HYPOTHESES = 120
REFINE_ITERATIONS = 10
DIST_THRESHOLD = 1e-3
WAVE, WORKGROUP = 64, 256      # threads that share one track: up to 64 observations / more
MAX_TRACK_LENGTH = 448
MAX_LENGTH_BINS = 1024


def make_cams(Ks, poses):
    """[V,16]: [R | t] row-major, fx, fy, cx, cy."""
    Ks, poses = np.asarray(Ks, F64), np.asarray(poses, F64)
    return np.concatenate([poses[:, :3, :4].reshape(-1, 12), Ks[:, 0, 0:1], Ks[:, 1, 1:2], Ks[:, 0, 2:3], Ks[:, 1, 2:3]], axis=1)


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


# ---- covisible pairs (pairs_from_poses.py:6-70) ----------------------------------------------------------------
def covis_pairs(poses, seq_ids, num_matched=10):
    from onepose_amd.mapping import covis_pairs as impl
    return impl(poses, seq_ids, num_matched)


# ---- verification ----------------------------------------------------------------------------------------------------
def verify_pair(kpi, kpj, ci, cj, matches0, max_error=MAX_EPIPOLAR_ERROR, min_inliers=MIN_PAIR_INLIERS, return_debug=False):
    """-> (survivors [n,2] int32 in index order, reported count)."""
    ci, cj = np.asarray(ci, F64), np.asarray(cj, F64)
    Ri, Rj = ci[:12].reshape(3, 4), cj[:12].reshape(3, 4)
    R = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            R[r, c] = dot3(Rj[r, 0], Rj[r, 1], Rj[r, 2], Ri[c, 0], Ri[c, 1], Ri[c, 2])
    t = np.array([Rj[r, 3] - dot3(R[r, 0], R[r, 1], R[r, 2], Ri[0, 3], Ri[1, 3], Ri[2, 3]) for r in range(3)])
    E = np.empty((3, 3))
    for c in range(3):
        E[0, c] = t[1] * R[2, c] - t[2] * R[1, c]
        E[1, c] = t[2] * R[0, c] - t[0] * R[2, c]
        E[2, c] = t[0] * R[1, c] - t[1] * R[0, c]
    m0 = np.asarray(matches0, np.int64)[:len(kpi)]
    a = np.nonzero((m0 > -1) & (m0 < len(kpj)))[0]
    b = m0[a]
    pi, pj = np.asarray(kpi, np.float32)[a].astype(F64), np.asarray(kpj, np.float32)[b].astype(F64)
    xi, yi = (pi[:, 0] - ci[14]) / ci[12], (pi[:, 1] - ci[15]) / ci[13]
    xj, yj = (pj[:, 0] - cj[14]) / cj[12], (pj[:, 1] - cj[15]) / cj[13]
    l0, l1, l2 = (E[0, 0] * xi + E[0, 1] * yi) + E[0, 2], (E[1, 0] * xi + E[1, 1] * yi) + E[1, 2], (E[2, 0] * xi + E[2, 1] * yi) + E[2, 2]
    k0, k1 = (E[0, 0] * xj + E[1, 0] * yj) + E[2, 0], (E[0, 1] * xj + E[1, 1] * yj) + E[2, 1]
    num = (l0 * xj + l1 * yj) + l2
    Aj, Bj, Ai, Bi = l0 / cj[12], l1 / cj[13], k0 / ci[12], k1 / ci[13]
    denj, deni = Aj * Aj + Bj * Bj, Ai * Ai + Bi * Bi
    thr2 = max_error * max_error
    with np.errstate(divide="ignore", invalid="ignore"):
        dj, di = (num * num) / denj, (num * num) / deni
        keep = (denj > 0.0) & (deni > 0.0) & (dj <= thr2) & (di <= thr2)
    surv = np.stack([a[keep], b[keep]], axis=1).astype(np.int32).reshape(-1, 2)
    count = len(surv) if len(surv) >= min_inliers else 0
    if return_debug:
        return surv, count, dict(residuals=np.concatenate([dj, di]), thr2=thr2)
    return surv, count


# ---- triangulation ---------------------------------------------------------------------------------------------------
def stage(cam, xy, dtype=F64):
    """Centre C [m,3] and ray d [m,3] of every observation, as the kernel stages them."""
    c = np.asarray(cam, dtype)
    x, y = np.asarray(xy, np.float32)[:, 0].astype(dtype), np.asarray(xy, np.float32)[:, 1].astype(dtype)
    xn, yn = (x - c[:, 14]) / c[:, 12], (y - c[:, 15]) / c[:, 13]
    C = np.stack([-dot3(c[:, 0], c[:, 4], c[:, 8], c[:, 3], c[:, 7], c[:, 11]), -dot3(c[:, 1], c[:, 5], c[:, 9], c[:, 3], c[:, 7], c[:, 11]),
                  -dot3(c[:, 2], c[:, 6], c[:, 10], c[:, 3], c[:, 7], c[:, 11])], axis=1)
    d = np.stack([(c[:, 0] * xn + c[:, 4] * yn) + c[:, 8], (c[:, 1] * xn + c[:, 5] * yn) + c[:, 9], (c[:, 2] * xn + c[:, 6] * yn) + c[:, 10]],
                 axis=1)
    return C, d


def project(cam, xy, X, dtype=F64):
    """Camera-frame depth and squared reprojection error of X [..., 3] in the observations [m]: -> (pz, err) [..., m]."""
    c = np.asarray(cam, dtype)
    X = np.asarray(X, dtype)[..., None, :]
    px = dot3(c[:, 0], c[:, 1], c[:, 2], X[..., 0], X[..., 1], X[..., 2]) + c[:, 3]
    py = dot3(c[:, 4], c[:, 5], c[:, 6], X[..., 0], X[..., 1], X[..., 2]) + c[:, 7]
    pz = dot3(c[:, 8], c[:, 9], c[:, 10], X[..., 0], X[..., 1], X[..., 2]) + c[:, 11]
    xy = np.asarray(xy, np.float32).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        ex = (c[:, 12] * (px / pz) + c[:, 14]) - xy[:, 0]
        ey = (c[:, 13] * (py / pz) + c[:, 15]) - xy[:, 1]
    return pz, ex * ex + ey * ey


def midpoints(C, d, a, b):
    """-> (valid [H], X [H,3], den / (aa cc) [H]: the squared sine of the angle between the rays) of the hypotheses (a[h], b[h])."""
    Ca, da, Cb, db = C[a], d[a], C[b], d[b]
    w = Ca - Cb
    aa, bb, cc = dot3(*da.T, *da.T), dot3(*da.T, *db.T), dot3(*db.T, *db.T)
    dd, ee = dot3(*da.T, *w.T), dot3(*db.T, *w.T)
    den = aa * cc - bb * bb
    with np.errstate(divide="ignore", invalid="ignore"):
        s, t = (bb * ee - cc * dd) / den, (aa * ee - bb * dd) / den
        X = 0.5 * ((Ca + s[:, None] * da) + (Cb + t[:, None] * db))
    return den > 0.0, X, den / (aa * cc)


def cos_min_of(min_tri_angle):
    return math.cos(min_tri_angle * (math.pi / 180.0))


def angle_terms(Ca, Cb, X):
    """dot and sqrt(na nb) of the rays Ca -> X and Cb -> X (broadcasting)."""
    ra, rb = X - Ca, X - Cb
    na, nb = dot3(ra[..., 0], ra[..., 1], ra[..., 2], ra[..., 0], ra[..., 1], ra[..., 2]), dot3(rb[..., 0], rb[..., 1], rb[..., 2], rb[..., 0], rb[..., 1], rb[..., 2])
    return dot3(ra[..., 0], ra[..., 1], ra[..., 2], rb[..., 0], rb[..., 1], rb[..., 2]), np.sqrt(na * nb)


def hypotheses(m, max_hypotheses=MAX_HYPOTHESES, seed=0):
    """Observation pairs (a [H], b [H]) in hypothesis order."""
    if m * (m - 1) // 2 <= max_hypotheses:
        a, b = np.triu_indices(m, 1)
        return a.astype(np.int64), b.astype(np.int64)
    ab = np.array([sample_indices(seed, h, m, 2) for h in range(max_hypotheses)], np.int64)
    return ab[:, 0], ab[:, 1]


def solve3(S, b):
    c00, c01, c02 = S[3] * S[5] - S[4] * S[4], S[2] * S[4] - S[1] * S[5], S[1] * S[4] - S[2] * S[3]
    c11, c12, c22 = S[0] * S[5] - S[2] * S[2], S[1] * S[2] - S[0] * S[4], S[0] * S[3] - S[1] * S[1]
    det = (S[0] * c00 + S[1] * c01) + S[2] * c02
    if not (det > 0.0) or not (det < np.inf):
        return None
    return np.array([((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det, ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det,
                     ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det], dtype=S.dtype)


def refit(cam, xy, inl, X0, refine_iterations=REFINE_ITERATIONS, dtype=F64):
    """Linear multi-ray least squares over the inliers, then Gauss-Newton on their reprojection error; X0: the winning
    midpoint, kept where the linear system is singular."""
    c = np.asarray(cam, dtype)
    m = len(c)
    lanes = WAVE if m <= WAVE else WORKGROUP
    C, d = stage(cam, xy, dtype)
    sel = np.asarray(inl, bool)[:, None]
    one = dtype(1.0)
    n2 = dot3(*d.T, *d.T)
    qq = dot3(*d.T, *C.T) / n2
    rows = np.stack([one - d[:, 0] * d[:, 0] / n2, -(d[:, 0] * d[:, 1] / n2), -(d[:, 0] * d[:, 2] / n2), one - d[:, 1] * d[:, 1] / n2,
                     -(d[:, 1] * d[:, 2] / n2), one - d[:, 2] * d[:, 2] / n2, C[:, 0] - d[:, 0] * qq, C[:, 1] - d[:, 1] * qq,
                     C[:, 2] - d[:, 2] * qq], axis=1)
    s = lane_tree_sum(np.where(sel, rows, dtype(0.0)), lanes)
    X = np.asarray(X0, dtype).copy()
    lin = solve3(s[:6], s[6:])
    if lin is not None:
        X = lin
    xyd = np.asarray(xy, np.float32).astype(dtype)
    for _ in range(refine_iterations):
        px = dot3(c[:, 0], c[:, 1], c[:, 2], X[0], X[1], X[2]) + c[:, 3]
        py = dot3(c[:, 4], c[:, 5], c[:, 6], X[0], X[1], X[2]) + c[:, 7]
        pz = dot3(c[:, 8], c[:, 9], c[:, 10], X[0], X[1], X[2]) + c[:, 11]
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = px / pz, py / pz
            rx, ry = (c[:, 12] * u + c[:, 14]) - xyd[:, 0], (c[:, 13] * v + c[:, 15]) - xyd[:, 1]
            sx, sy = c[:, 12] / pz, c[:, 13] / pz
            J0 = [sx * (c[:, k] - u * c[:, 8 + k]) for k in range(3)]
            J1 = [sy * (c[:, 4 + k] - v * c[:, 8 + k]) for k in range(3)]
            rows = np.stack([J0[0] * J0[0] + J1[0] * J1[0], J0[0] * J0[1] + J1[0] * J1[1], J0[0] * J0[2] + J1[0] * J1[2],
                             J0[1] * J0[1] + J1[1] * J1[1], J0[1] * J0[2] + J1[1] * J1[2], J0[2] * J0[2] + J1[2] * J1[2],
                             J0[0] * rx + J1[0] * ry, J0[1] * rx + J1[1] * ry, J0[2] * rx + J1[2] * ry], axis=1)
        s = lane_tree_sum(np.where(sel, rows, dtype(0.0)), lanes)
        dx = solve3(s[:6], s[6:])
        if dx is None:
            break
        X = X - dx
    return X


def triangulate_track(cam, xy, max_reproj_error=MAX_REPROJ_ERROR, min_tri_angle=MIN_TRI_ANGLE, max_hypotheses=MAX_HYPOTHESES,
                      refine_iterations=REFINE_ITERATIONS, seed=0, return_debug=False):
    """One track: cam [m,16] (the camera of each observation), xy [m,2] fp32 -> dict(ok, xyz [3], mask [m] bool, info [4],
    length, inliers [m] bool (of the best hypothesis, what the refit used))."""
    cam = np.asarray(cam, F64)
    m = len(cam)
    fail = dict(ok=False, xyz=np.zeros(3), mask=np.zeros(m, bool), info=[0, m, -1, 0], length=0, inliers=np.zeros(m, bool), debug=None)
    if m < 2 or m > MAX_TRACK_LENGTH:
        return fail
    thr2, cos_min = max_reproj_error * max_reproj_error, cos_min_of(min_tri_angle)
    C, d = stage(cam, xy)
    a, b = hypotheses(m, max_hypotheses, seed)
    den_ok, X, den_rel = midpoints(C, d, a, b)
    with np.errstate(invalid="ignore"):
        dots, norms = angle_terms(C[a], C[b], X)
        pz, err = project(cam, xy, X)                     # [H, m]
        inl = (pz > 0.0) & (err <= thr2)
        H = np.arange(len(a))
        valid = den_ok & (dots <= cos_min * norms) & inl[H, a] & inl[H, b]
    counts = np.where(valid, inl.sum(axis=1), 0)
    # what the exactness conditions look at: every residual and depth of the valid hypotheses (they are counted), and of every
    # hypothesis with den > 0 the angle and the residuals and depths of its own two observations (they decide its validity)
    own = np.concatenate([H[den_ok], H[den_ok]]), np.concatenate([a[den_ok], b[den_ok]])
    debug = dict(residuals=np.concatenate([err[valid].ravel(), err[own]]), thr2=thr2, counts=counts, valid=valid, inl=inl, pairs=(a, b),
                 hyp_angles=_angles(dots[den_ok], norms[den_ok]), pz=np.concatenate([pz[valid].ravel(), pz[own]]), den_rel=den_rel)
    if not valid.any() or counts.max() <= 0:
        fail["debug"] = debug
        return fail
    best = int(np.argmax(counts))                         # the first of the largest: lowest index on ties
    inliers = inl[best]
    Xr = refit(cam, xy, inliers, X[best], refine_iterations)
    pz, err = project(cam, xy, Xr)
    with np.errstate(invalid="ignore"):
        keep = inliers & (pz > 0.0) & (err <= thr2)
    k = np.nonzero(keep)[0]
    wide, final_angles = False, np.zeros(0)
    if len(k) >= 2:
        ia, ib = np.triu_indices(len(k), 1)
        dots, norms = angle_terms(C[k[ia]], C[k[ib]], Xr)
        wide = bool((dots <= cos_min * norms).any())
        final_angles = _angles(dots, norms)
    debug.update(final_residuals=err[inliers], final_pz=pz[inliers], final_angles=final_angles)
    ok = len(k) >= 2 and wide and bool(np.isfinite(Xr).all())
    if not ok:
        fail.update(info=[0, m, best, int(counts[best])], inliers=inliers, debug=debug)
        return fail
    return dict(ok=True, xyz=Xr, mask=keep, info=[1, m, best, int(counts[best])], length=len(k), inliers=inliers, debug=debug,
                start=X[best])


def _angles(dots, norms):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.degrees(np.arccos(np.clip(dots / norms, -1.0, 1.0)))


def triangulate(track_offsets, obs_image, obs_xy, cams, **kw):
    """CSR tracks -> (xyz [T,3], mask [M] int32, info [T,4] int32, lengths [T] int32, per-track results)."""
    T = len(track_offsets) - 1
    xyz, info, lengths = np.zeros((T, 3)), np.zeros((T, 4), np.int32), np.zeros(T, np.int32)
    mask = np.zeros(len(obs_image), np.int32)
    res = []
    for t in range(T):
        s, e = track_offsets[t], track_offsets[t + 1]
        r = triangulate_track(cams[obs_image[s:e]], obs_xy[s:e], **kw)
        if r["ok"]:
            xyz[t], lengths[t] = r["xyz"], r["length"]
            mask[s:e] = r["mask"]
        info[t] = r["info"]
        res.append(r)
    return xyz, mask, info, lengths, res


# ---- filters (filter_tkl.py:42-50, filter_points.py) ---------------------------------------------------------------------
def track_length_threshold(lengths, max_num_kp3d):
    lengths = np.asarray(lengths)
    lengths = np.minimum(lengths[lengths > 0], MAX_LENGTH_BINS - 1)
    remaining = len(lengths)
    keys, cnt = np.unique(lengths, return_counts=True)
    for k, c in zip(keys, cnt):
        remaining -= c
        if remaining <= max_num_kp3d:
            return int(k)
    return 0


def box_margins(xyz, box):
    """fp32 (m [n,3], v.v [3]) of the box test."""
    p = np.asarray(xyz, F64).astype(np.float32).reshape(-1, 3)
    c = np.asarray(box, np.float32)
    q = p - c[4]
    ms, vv = [], []
    for corner in (5, 0, 7):
        e = c[corner] - c[4]
        ms.append((q[:, 0] * e[0] + q[:, 1] * e[1]) + q[:, 2] * e[2])
        vv.append((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return np.stack(ms, axis=1), np.array(vv, np.float32)


def filter_points(xyz, lengths, threshold, box):
    """-> (kept ids ascending int32, their fp32 coordinates)."""
    lengths = np.asarray(lengths)
    m, vv = box_margins(xyz, box)
    keep = (lengths > 0) & (lengths >= threshold) & np.all((np.float32(0) < m) & (m < vv), axis=1)
    ids = np.nonzero(keep)[0].astype(np.int32)
    return ids, np.asarray(xyz, F64).astype(np.float32).reshape(-1, 3)[ids]


def pair_distances(xyz32):
    p = np.asarray(xyz32, np.float32).astype(F64)
    dx, dy, dz = (p[:, None, k] - p[None, :, k] for k in range(3))
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def merge_points(xyz32, dist_threshold=DIST_THRESHOLD):
    """-> (merged [n',3] fp32, members: list of ascending position arrays)."""
    xyz32 = np.asarray(xyz32, np.float32)
    close = pair_distances(xyz32) < dist_threshold
    taken = np.zeros(len(xyz32), bool)
    merged, members = [], []
    for j in range(len(xyz32)):
        row = np.nonzero(close[j])[0]
        if taken[row].any():
            continue
        s = np.zeros(3, np.float32)
        for i in row:
            s = s + xyz32[i]
        merged.append(s / np.float32(len(row)))
        members.append(row.astype(np.int32))
        taken[row] = True
    return np.array(merged, np.float32).reshape(-1, 3), members


# ---- descriptors (feature_process.py:95-188, 297-317) ------------------------------------------------------------------------
def gather_descriptors(features, point_offsets, obs_image, obs_kpt):
    """features: per image dict(descriptors [dim,n] fp32, scores [n] fp32) -> (collect [K,dim] fp32, scores [K] fp32, idxs [N]
    int64, mean descriptors [N,dim] fp64, mean scores [N] fp64), sums in observation order."""
    K, N = len(obs_image), len(point_offsets) - 1
    dim = features[0]["descriptors"].shape[0]
    cd, cs = np.zeros((K, dim), np.float32), np.zeros(K, np.float32)
    for k in range(K):
        cd[k] = features[obs_image[k]]["descriptors"][:, obs_kpt[k]]
        cs[k] = np.asarray(features[obs_image[k]]["scores"]).reshape(-1)[obs_kpt[k]]
    md, ms, idxs = np.zeros((N, dim)), np.zeros(N), np.zeros(N, np.int64)
    for p in range(N):
        s, e = point_offsets[p], point_offsets[p + 1]
        acc, accs = np.zeros(dim), 0.0
        for k in range(s, e):
            acc = acc + cd[k].astype(F64)
            accs = accs + F64(cs[k])
        idxs[p] = e - s
        if e > s:
            md[p], ms[p] = acc / F64(e - s), accs / F64(e - s)
    return cd, cs, idxs, md, ms


# ---- the whole tail, as ObjectMapper.build_from_matches chains it ------------------------------------------------------------
def post_process(xyz, lengths, track_offsets, obs_image, obs_kpt, inlier_mask, features, box, max_num_kp3d=2500,
                 dist_threshold=DIST_THRESHOLD):
    """Track-length threshold, filters, merge and descriptor gathering on a triangulated model -> dict."""
    from onepose_amd.mapping import annotation_arrays, point_observations
    thr = track_length_threshold(lengths, max_num_kp3d)
    kept_ids, kept_xyz = filter_points(xyz, lengths, thr, box)
    merged, members = merge_points(kept_xyz, dist_threshold)
    member_offsets = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    flat = np.concatenate(members).astype(np.int32) if members else np.zeros(0, np.int32)
    point_offsets, g_img, g_kpt = point_observations(track_offsets, obs_image, obs_kpt, inlier_mask, kept_ids, member_offsets, flat)
    cd, cs, idxs, md, ms = gather_descriptors(features, point_offsets, g_img, g_kpt)
    return dict(threshold=thr, kept_ids=kept_ids, kept_xyz=kept_xyz, merged_xyz=merged, member_offsets=member_offsets, members=flat,
                point_offsets=point_offsets, gather_image=g_img, gather_kpt=g_kpt, anno=annotation_arrays(merged, cd, cs, idxs, md, ms))


def run_chain(features, pair_matches, poses, Ks, box, max_epipolar_error=MAX_EPIPOLAR_ERROR, min_pair_inliers=MIN_PAIR_INLIERS,
              max_reproj_error=MAX_REPROJ_ERROR, min_tri_angle=MIN_TRI_ANGLE, max_hypotheses=MAX_HYPOTHESES,
              refine_iterations=REFINE_ITERATIONS, max_num_kp3d=2500, dist_threshold=DIST_THRESHOLD, seed=0):
    from onepose_amd.mapping import build_tracks
    cams = make_cams(Ks, poses)
    n_kpts = [len(f["keypoints"]) for f in features]
    survivors, counts, residuals = [], [], []
    for i, j, m0 in pair_matches:
        s, c, dbg = verify_pair(features[i]["keypoints"], features[j]["keypoints"], cams[i], cams[j], m0, max_epipolar_error,
                                min_pair_inliers, return_debug=True)
        survivors.append(s[:c])
        counts.append(c)
        residuals.append(dbg["residuals"])
    pair_images = np.array([(i, j) for i, j, _ in pair_matches], np.int32)
    track_offsets, obs_image, obs_kpt = build_tracks(n_kpts, pair_images, survivors)
    kp = np.concatenate([np.asarray(f["keypoints"], np.float32).reshape(-1, 2) for f in features])
    offs = np.concatenate([[0], np.cumsum(n_kpts)])
    obs_xy = kp[offs[obs_image] + obs_kpt]
    xyz, mask, info, lengths, res = triangulate(track_offsets, obs_image, obs_xy, cams, max_reproj_error=max_reproj_error,
                                                min_tri_angle=min_tri_angle, max_hypotheses=max_hypotheses,
                                                refine_iterations=refine_iterations, seed=seed)
    out = post_process(xyz, lengths, track_offsets, obs_image, obs_kpt, mask, features, box, max_num_kp3d, dist_threshold)
    out.update(survivors=survivors, counts=np.array(counts, np.int32), verify_residuals=residuals, track_offsets=track_offsets,
               obs_image=obs_image, obs_kpt=obs_kpt, obs_xy=obs_xy, cams=cams, xyz=xyz, inlier_mask=mask, info=info, lengths=lengths,
               tracks=res)
    return out
