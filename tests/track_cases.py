"""Seeded inputs of the tracker tests: planted scenes (object points in a +-0.08 box, cameras about 0.45 away, f = 600,
c = 256), the update problems cut from them at the shapes the kernels are tested at, the hand cases, and two frame sequences
for the state machine.  Built once per process and shared (callers do not write into them)."""
import functools

import numpy as np

import flow_cases as fc

F, C = 600.0, 256.0
BOX, DISTANCE = 0.08, 0.45
D = 256
K = np.array([[F, 0, C], [0, F, C], [0, 0, 1.0]])
GATE, MAX_REPROJ, MAX_Z = 1.2, 20.0, 0.15

INPUTS = ("matches0", "kf_xy", "q_xy", "kf_pt_ids", "points", "K_kf", "K_q", "pose_kf", "pose_q")


def rotation(rx, ry, rz):
    cx, cy, cz = np.cos([rx, ry, rz])
    sx, sy, sz = np.sin([rx, ry, rz])
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def pose(rx, ry, rz, tx=0.0, ty=0.0, tz=DISTANCE):
    """[4, 4] world -> camera: the object at the origin, tz in front of the camera."""
    T = np.eye(4)
    T[:3, :3] = rotation(rx, ry, rz)
    T[:3, 3] = [tx, ty, tz]
    return T


def project(X, Kmat, T):
    c = X @ T[:3, :3].T + T[:3, 3]
    return (c @ Kmat.T)[:, :2] / c[:, 2:]


def unit_descriptors(n, seed):
    d = np.random.RandomState(seed).standard_normal((D, n))
    return (d / np.linalg.norm(d, axis=0)).astype(np.float32)


POSE_KF = pose(0.25, -0.3, 0.1, 0.01, -0.02)
POSE_Q = pose(0.05, 0.2, -0.15, -0.02, 0.01, 0.47)


def update_problem(n_kf, n_q, known="half", noise=0.3, seed=0, outliers=0.0, point_noise=5e-4):
    """One trk_update problem: m = about 3/4 of min(n_kf, n_q) object points seen in both views (at least one) under `noise` px
    of Gaussian keypoint noise, the other keypoints random; `known`: how many of the pairs carry a 3D id ("none", "all", "half"
    or a count), their map points off by `point_noise`; `outliers`: the share of pairs whose query keypoint is moved by 30-60 px."""
    rs = np.random.RandomState(seed)
    m = max(1, min(n_kf, n_q) * 3 // 4)
    X = rs.uniform(-BOX, BOX, (m, 3))
    kf_xy = rs.uniform(20, 492, (n_kf, 2))
    q_xy = rs.uniform(20, 492, (n_q, 2))
    slots_kf, slots_q = np.sort(rs.permutation(n_kf)[:m]), rs.permutation(n_q)[:m]
    kf_xy[slots_kf] = project(X, K, POSE_KF) + noise * rs.standard_normal((m, 2))
    q_xy[slots_q] = project(X, K, POSE_Q) + noise * rs.standard_normal((m, 2))
    bad = rs.uniform(size=m) < outliers
    q_xy[slots_q[bad]] += rs.uniform(30, 60, (int(bad.sum()), 2)) * rs.choice([-1, 1], (int(bad.sum()), 2))
    matches0 = np.full(n_kf, -1, np.int32)
    matches0[slots_kf] = slots_q
    n_known = {"none": 0, "all": m, "half": m // 2}.get(known, known)
    n_known = min(int(n_known), m)
    who = np.sort(rs.permutation(m)[:n_known])
    kf_pt_ids = np.full(n_kf, -1, np.int32)
    extra = 3                                                # map points no pair names
    order = rs.permutation(n_known + extra)
    points = rs.uniform(-BOX, BOX, (n_known + extra, 3))
    points[order[:n_known]] = X[who] + point_noise * rs.standard_normal((n_known, 3))
    kf_pt_ids[slots_kf[who]] = order[:n_known]
    return dict(matches0=matches0, kf_xy=kf_xy.astype(np.float32), q_xy=q_xy.astype(np.float32), kf_pt_ids=kf_pt_ids, points=points,
                K_kf=K.copy(), K_q=K.copy(), pose_kf=POSE_KF.copy(), pose_q=POSE_Q.copy())


SHAPES = [(1, 1), (5, 7), (63, 65), (64, 64), (65, 63), (255, 257), (257, 300), (1025, 1000), (8192, 8192)]


@functools.lru_cache(maxsize=None)
def shape_cases():
    """name -> problem: every shape with about half the pairs known, and at (257, 300) the known counts 0, 1, 2, odd, even, all
    (all: no candidate; 0: every pair a candidate)."""
    cases = {}
    for k, (n_kf, n_q) in enumerate(SHAPES):
        cases[f"{n_kf}x{n_q}"] = update_problem(n_kf, n_q, "half", seed=10 + k, outliers=0.1 if n_kf > 5 else 0.0)
    for k, known in enumerate(["none", 1, 2, 51, 52, "all"]):
        cases[f"257x300_known_{known}"] = update_problem(257, 300, known, seed=40 + k, outliers=0.1)
    cases["1x1_known"] = update_problem(1, 1, "all", seed=60)
    cases["8192x8192_all_known"] = update_problem(8192, 8192, "all", seed=61, outliers=0.05)
    cases["8192x8192_none_known"] = update_problem(8192, 8192, "none", seed=62, outliers=0.05)
    return cases


def _hand(matches0, kf_pt_ids, X, n_q=None, extra_points=0, q_shift=None, **over):
    """A small problem on exact projections of X: pair i of the keyframe sees X[i]; matches0 / kf_pt_ids as given."""
    n_kf = len(matches0)
    n_q = n_q or n_kf
    rs = np.random.RandomState(99)
    kf_xy = project(X[:n_kf], K, POSE_KF)
    q_xy = rs.uniform(50, 450, (n_q, 2))
    for i, j in enumerate(matches0):
        if 0 <= j < n_q:
            q_xy[j] = project(X[i:i + 1], K, POSE_Q)[0]
    if q_shift is not None:
        q_xy = q_xy + np.asarray(q_shift, np.float64)
    points = np.concatenate([X[:n_kf], rs.uniform(-BOX, BOX, (extra_points, 3))])
    case = dict(matches0=np.asarray(matches0, np.int32), kf_xy=kf_xy.astype(np.float32), q_xy=q_xy.astype(np.float32),
                kf_pt_ids=np.asarray(kf_pt_ids, np.int32), points=points, K_kf=K.copy(), K_q=K.copy(), pose_kf=POSE_KF.copy(),
                pose_q=POSE_Q.copy())
    case.update(over)
    return case


HAND_X = np.random.RandomState(7).uniform(-BOX, BOX, (8, 3))


@functools.lru_cache(maxsize=None)
def hand_cases():
    X = HAND_X
    cases = {}
    cases["no_pair"] = _hand([-1, -1, -1], [0, 1, -1], X, n_q=4)
    cases["one_known"] = _hand([0, -1, -1], [0, -1, -1], X)
    even = _hand([1, 0, -1], [0, 1, -1], X)
    even["q_xy"][0, 0] += 2.0                # two known pairs at different distances: the even median
    cases["two_known"] = even
    tied = _hand([0, 1, 2, 3], [0, 0, 0, 0], X)
    tied["kf_pt_ids"][:] = [0, 0, 0, 0]
    tied["q_xy"][:] = tied["q_xy"][0] + np.float32(3.0)      # four pairs on one map point and one pixel: four equal distances
    cases["tied_distances"] = tied
    nan_row = _hand([0, 1, 2, 3], [0, 1, 2, -1], X)
    nan_row["points"][1] = np.nan
    cases["nan_point"] = nan_row
    # One camera at the world origin seen twice, one pixel: the two rays coincide, A^T A has a two-dimensional null space (the
    # centre and the ray's direction) and its fourth row and column are exactly zero.  Whichever the Jacobi returns -- the
    # direction (v[3] = 0) or the centre (which projects to 0 / 0) -- nothing finite comes out.  (Away from the origin the
    # answer is an arbitrary point on the ray with no reprojection error, in the reference's SVD as here.)
    origin = np.eye(4)
    same = _hand([0, 1, 2], [-1, -1, 0], X, pose_kf=origin, pose_q=origin.copy())
    same["points"][0] = [0.01, 0.02, 0.3]
    same["kf_xy"][:] = np.array([[300, 200], [100, 400], [262, 290]], np.float32)
    same["q_xy"][:] = same["kf_xy"][[0, 1, 2]]
    same["q_xy"][2] = [276.5, 296.25]          # the known pair: a finite distance
    same["matches0"][:] = [0, 1, 2]
    cases["identical_cameras"] = same
    cases["out_of_range"] = _hand([0, 5, -2, 3, 4, 1], [0, -1, 1, 9, -3, -1], X, n_q=5)     # matches 5, -2 and ids 9, -3 are ignored
    cases["two_pairs_one_query"] = _hand([1, 1, 0, -1], [-1, 0, -1, -1], X, n_q=4)
    cases["no_points"] = _hand([0, 1, 2], [-1, -1, -1], X, points=np.zeros((0, 3)))
    return cases


# ---- golden cases: what the reference's own functions are run on ---------------------------------------------------------------

GOLDEN = {"clean": dict(noise=0.0, outliers=0.0), "half_px": dict(noise=0.5, outliers=0.0), "outliers": dict(noise=0.3, outliers=0.15)}


@functools.lru_cache(maxsize=None)
def golden_cases():
    return {name: update_problem(300, 320, "half", seed=80 + k, **kw) for k, (name, kw) in enumerate(sorted(GOLDEN.items()))}


METRIC_POSES = [(pose(0.1, 0.2, 0.3), pose(0.1, 0.2, 0.3)), (pose(0.1, 0.2, 0.3), pose(0.12, 0.18, 0.33, 0.01, 0.0, 0.46)),
                (pose(-0.4, 0.1, 0.0, 0.02, 0.03, 0.5), pose(0.3, -0.2, 0.1))]


# ---- sequences for the state machine ------------------------------------------------------------------------------------------

class Sequence:
    """kf: the keyframe dict of add_kf / update_kf; frames: the dicts of track(); truth: the true [4, 4] pose of every frame."""

    def __init__(self, kf, frames, truth, auto_mode):
        self.kf, self.frames, self.truth, self.auto_mode = kf, frames, truth, auto_mode

    def copy(self):
        """Fresh dicts (the tracker writes into them) over the same arrays."""
        dup = lambda d: {k: (dict(v) if isinstance(v, dict) else v) for k, v in d.items()}  # noqa: E731
        return Sequence(dup(self.kf), [dup(f) for f in self.frames], self.truth, self.auto_mode)


def _frame(X, desc, T, Kmat, image, rs, n_extra, seed):
    """The dict of one frame: the projections of X in a random order plus n_extra keypoints of their own."""
    n = len(X)
    order = rs.permutation(n + n_extra)
    xy = np.concatenate([project(X, Kmat, T), rs.uniform(30, 480, (n_extra, 2))])[order].astype(np.float32)
    d = np.concatenate([desc, unit_descriptors(n_extra, seed)], axis=1)[:, order]
    where = np.argsort(order)[:n]           # keypoint index of object point i
    frame = {'im_path': image, 'kpt_pred': {'keypoints': xy, 'descriptors': np.ascontiguousarray(d), 'scores': np.ones(n + n_extra, np.float32)},
             'pose_pred': T.copy(), 'pose_gt': T.copy(), 'K': Kmat.copy(), 'K_crop': Kmat.copy()}
    return frame, where


def _keyframe(frame, where, X, n_db, rs):
    """The first n_db object points are database points the keyframe matched (2D-3D), the others are to be triangulated."""
    kf = dict(frame)
    kf['kpt_pred'] = dict(frame['kpt_pred'])
    ids = np.sort(where[:n_db])
    src = np.argsort(where[:n_db])
    kf.update(valid_query_id=ids, mkpts2d=frame['kpt_pred']['keypoints'][ids], mkpts3d=X[:n_db][src].astype(np.float32).astype(np.float64),
              kpt3d_ids=(1000 + np.arange(n_db))[src])
    return kf


@functools.lru_cache(maxsize=None)
def auto_sequence(n_frames=12, n_points=96, n_db=96, n_extra=8):
    """A camera circling the object slowly, noise-free keypoints, no images: tracked with auto_mode=True (ground-truth initial
    poses while the init counter runs, motion prediction afterwards, which lags the motion by about 1.5 frames as the
    reference writes it).  Every object point is a database point of the first keyframe: the adjustment holds no camera or
    point fixed, so it shares the correction of a wrong initial pose between the new camera and the rest of the map, and the
    new camera takes the larger share only while the map is anchored by many points seen from several frames."""
    rs = np.random.RandomState(5)
    X = rs.uniform(-BOX, BOX, (n_points, 3))
    desc = unit_descriptors(n_points, 6)
    truth = [pose(0.2 + 0.0004 * k + 0.00001 * k * k, -0.3 + 0.0005 * k, 0.1 - 0.0002 * k, 0.00008 * k, -0.00006 * k, DISTANCE + 0.00004 * k)
             for k in range(n_frames + 1)]
    first, where = _frame(X, desc, truth[0], K, None, rs, n_extra, 100)
    kf = _keyframe(first, where, X, n_db, rs)
    frames = [_frame(X, desc, truth[k], K, None, rs, n_extra, 100 + k)[0] for k in range(1, n_frames + 1)]
    return Sequence(kf, frames, truth, True)


FLOW_SIZE, FLOW_SHIFTS = 512, [(2 * k, -k) for k in range(13)]


@functools.lru_cache(maxsize=None)
def flow_sequence(n_frames=12, n_points=96, n_db=96, n_extra=8):
    """A moving crop of one textured view for the flow step: frame k is the keyframe's image shifted by FLOW_SHIFTS[k] whole
    pixels, i.e. the same pose under an intrinsic matrix whose principal point moved by the shift (the crop follows the
    object), so the flow step has real pixels and the truth is known.  (A camera translating parallel to a textured plane
    gives the same images, but coplanar 3D points are singular for EPnP's barycentric coordinates.)"""
    rs = np.random.RandomState(8)
    X = rs.uniform(-BOX, BOX, (n_points, 3))
    desc = unit_descriptors(n_points, 9)
    T = pose(0.2, -0.25, 0.1, 0.0, 0.0, DISTANCE)
    big = fc.texture(FLOW_SIZE + 2 * 32, FLOW_SIZE + 2 * 32, 0.08, 21)

    def view(shift):
        dx, dy = shift
        Kk = K.copy()
        Kk[0, 2] += dx
        Kk[1, 2] += dy
        return np.ascontiguousarray(big[32 - dy:32 - dy + FLOW_SIZE, 32 - dx:32 - dx + FLOW_SIZE]), Kk

    image, K0 = view(FLOW_SHIFTS[0])
    first, where = _frame(X, desc, T, K0, image, rs, n_extra, 200)
    kf = _keyframe(first, where, X, n_db, rs)
    frames = []
    for k in range(1, n_frames + 1):
        image, Kk = view(FLOW_SHIFTS[k])
        frames.append(_frame(X, desc, T, Kk, image, rs, n_extra, 200 + k)[0])
    return Sequence(kf, frames, [T] * (n_frames + 1), False)
