"""MI355X-native keyframe tracker: the map update step on HIP and the ``BATracker`` state machine around the five cores.

Host-side mirror of the reference's ``src/tracker/ba_tracker.py``:

``MapUpdater`` is the raw-tensor entry to the C ABI of ``include/mapping/track_update.h``, the block of ``track_ba`` at
:499-603 that turns one frame's 2D-2D matches into the next bundle-adjustment problem (reprojection gate against
1.2 x median, two-view DLT, point filters, new ids, the unmatched list).  ``apply_triangulation`` is the numpy drop-in for
:267-273.  ``BATracker`` keeps the reference's attributes and dict keys, so the loop of ``inference_demo.py:264-299`` runs
unchanged; its bookkeeping is numpy on the host, as in the reference, and its numerics go through ``NearestNeighbour``,
``FlowTracker.flow_track_device``, ``MapUpdater.update`` and ``bundle_adjust.apply_ba``.  There is no PyTorch compute path
and no CPU fallback.

Not claimed (nothing to compare against where this was developed): parity with ``cv2.triangulatePoints`` (the DLT here is
the reference's own ``_triangulatePy``, the eigenvector of A^T A), with ``cv2.Rodrigues`` (``rotvec_from_matrix`` /
``matrix_from_rotvec`` state their algorithm) and with ``transforms3d`` (``mat2euler`` / ``euler2mat`` are the static-xyz
convention that library defaults to).
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _native_trk, bundle_adjust
from ._binding import Engine, gpu_tensor

NO_CPU = "onepose_amd.MapUpdater runs only on a ROCm GPU ({} on {}); there is no CPU fallback"

MapUpdate = collections.namedtuple("MapUpdate", "pair_kf pair_q q_pt_ids pair_dist new_points unmatched_q median summary")


def _gpu(t, name, dtype):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor on a GPU (got {type(t).__name__})")
    return gpu_tensor(t, dtype, NO_CPU.format(name + " is", "{}"))


class MapUpdater(Engine):
    """Raw-tensor entry to the HIP map update step: workspaces cached per (n_kf, n_q, device, stream); no weights."""

    native = _native_trk
    WORKSPACE_BYTES, LAST_ERROR = "trk_workspace_bytes", "map_last_error"
    PARAMETER_REFUSAL = NO_CPU.format("a parameter is", "{}")
    MAX_CACHED_WORKSPACES = 8

    def __init__(self):
        super().__init__(None)

    def update(self, matches0, kf_xy, q_xy, kf_pt_ids, points, K_kf, K_q, pose_kf, pose_q, gate_factor=1.2, max_reproj=20.0,
               max_z=0.15):
        """matches0 [n_kf] integer (query index or -1), kf_xy [n_kf,2], q_xy [n_q,2], kf_pt_ids [n_kf] integer (-1 or a row of
        points), points [n_points,3], K_kf / K_q [3,3], pose_kf / pose_q [4,4] or [3,4] world -> camera, all on one GPU ->
        MapUpdate(pair_kf, pair_q, q_pt_ids [n_kf] int32, pair_dist [n_kf,2], new_points [n_kf,3] (the first summary[4] rows),
        unmatched_q [n_q] int32, median [1], summary [8] int32), left on the GPU, nothing synchronised; the inputs are not
        written.  summary: m, known, known kept, candidates, candidates kept, non-finite removed, ignored, unmatched."""
        m0, ids = _gpu(matches0, "matches0", torch.int32), _gpu(kf_pt_ids, "kf_pt_ids", torch.int32)
        kf, q = _gpu(kf_xy, "kf_xy", torch.float32), _gpu(q_xy, "q_xy", torch.float32)
        pts = _gpu(points, "points", torch.float64)
        Ks = [_gpu(K, name, torch.float64) for K, name in ((K_kf, "K_kf"), (K_q, "K_q"))]
        poses = [_gpu(p, name, torch.float64) for p, name in ((pose_kf, "pose_kf"), (pose_q, "pose_q"))]
        n_kf, n_q, n_points = kf.shape[0], q.shape[0], pts.shape[0]
        if m0.shape != (n_kf,) or ids.shape != (n_kf,) or kf.shape != (n_kf, 2) or q.shape != (n_q, 2) or pts.shape != (n_points, 3):
            raise ValueError("matches0 and kf_pt_ids must be [n_kf], kf_xy [n_kf,2], q_xy [n_q,2] and points [n_points,3]")
        if any(K.shape != (3, 3) for K in Ks) or any(tuple(p.shape) not in ((3, 4), (4, 4)) for p in poses):
            raise ValueError("K_kf and K_q must be [3,3], pose_kf and pose_q [4,4] or [3,4]")
        dev = kf.device
        i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)  # noqa: E731
        f64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)  # noqa: E731
        out = MapUpdate(i32(n_kf), i32(n_kf), i32(n_kf), f64(n_kf, 2), f64(n_kf, 3), i32(n_q), f64(1), i32(_native_trk.SUMMARY_ENTRIES))
        ws = self.workspace(n_kf, n_q, dev)
        self.call("trk_update", dev, m0, kf, q, ids, pts if n_points else None, *Ks, *poses, n_kf, n_q, n_points, float(gate_factor),
                  float(max_reproj), float(max_z), *out, ws, ws.numel())
        return out

    def triangulate(self, P1, P2, xy1, xy2):
        """Stage: the two-view DLT.  P1, P2 [3,4], xy1, xy2 [n,2] -> X [n,3] float64."""
        P1, P2 = _gpu(P1, "P1", torch.float64), _gpu(P2, "P2", torch.float64)
        a, b = _gpu(xy1, "xy1", torch.float32), _gpu(xy2, "xy2", torch.float32)
        n = a.shape[0]
        if P1.shape != (3, 4) or P2.shape != (3, 4) or a.shape != (n, 2) or b.shape != (n, 2):
            raise ValueError("P1 and P2 must be [3,4], xy1 and xy2 [n,2]")
        X = torch.empty(n, 3, device=a.device, dtype=torch.float64)
        if n:
            self.call("trk_triangulate_pairs", a.device, P1, P2, a, b, n, X)
        return X

    def gate_median(self, dist, factor=1.2):
        """Stage: dist [n] -> (median [1] = factor x numpy.median(dist), keep [n] int32 = dist < median)."""
        d = _gpu(dist, "dist", torch.float64)
        n = d.shape[0]
        if d.shape != (n,):
            raise ValueError("dist must be [n]")
        median = torch.empty(1, device=d.device, dtype=torch.float64)
        keep = torch.empty(n, device=d.device, dtype=torch.int32)
        ws = self.workspace(n, 1, d.device)
        self.call("trk_gate_median", d.device, d, n, float(factor), median, keep, ws, ws.numel())
        return median, keep


_updater = None


def _shared_updater():
    global _updater
    if _updater is None:
        _updater = MapUpdater()
    return _updater


def projection_matrix(K, pose):
    """P = K pose[:3] as the kernels form it: row dots with the index ascending."""
    K, pose = np.asarray(K, np.float64), np.asarray(pose, np.float64)
    P = np.empty((3, 4))
    for r in range(3):
        for c in range(4):
            P[r, c] = (K[r, 0] * pose[0, c] + K[r, 1] * pose[1, c]) + K[r, 2] * pose[2, c]
    return P


def apply_triangulation(K1, K2, Tcw1, Tcw2, kpt2d_1, kpt2d_2, device="cuda", updater=None):
    """Drop-in for ``BATracker.apply_triangulation`` (reference :267-273): K [3,3], Tcw [4,4] camera -> world (inverted here, as
    there), kpt2d [n,2] -> point_3d_w [n,3] float64, numpy in, numpy out."""
    updater = updater or _shared_updater()
    P1 = projection_matrix(K1, np.linalg.inv(np.asarray(Tcw1, np.float64))[:3])
    P2 = projection_matrix(K2, np.linalg.inv(np.asarray(Tcw2, np.float64))[:3])
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)  # noqa: E731
    X = updater.triangulate(to(P1, np.float64), to(P2, np.float64), to(np.asarray(kpt2d_1).reshape(-1, 2), np.float32),
                            to(np.asarray(kpt2d_2).reshape(-1, 2), np.float32))
    return X.cpu().numpy()


# ---- host helpers: plain numpy on one pose -----------------------------------------------------------------------------------

def cm_degree_5_metric(pose_pred, pose_target):
    """Reference :105-111: (translation distance in cm, rotation distance in degrees)."""
    pose_pred, pose_target = np.asarray(pose_pred), np.asarray(pose_target)
    translation_distance = np.linalg.norm(pose_pred[:, 3] - pose_target[:, 3]) * 100
    rotation_diff = np.dot(pose_pred[:, :3], pose_target[:, :3].T)
    trace = np.trace(rotation_diff)
    trace = trace if trace <= 3 else 3
    angular_distance = np.rad2deg(np.arccos((trace - 1.) / 2.))
    return translation_distance, angular_distance


def rotvec_from_matrix(R):
    """Rotation vector (axis x angle) of a rotation matrix.  With r = (R21 - R12, R02 - R20, R10 - R01) the skew part,
    s = |r| / 2 = sin(angle), c = (trace - 1) / 2 = cos(angle): angle = atan2(s, c); zero at the identity (s == 0, c > 0);
    axis = r / (2 s) while c >= -1/2; beyond (towards pi, where r vanishes) the axis comes from the diagonal of the symmetric
    part B = (R + R^T) / 2 = c I + (1 - c) a a^T: the largest a_k = sqrt((B_kk - c) / (1 - c)), the others B_kj / ((1 - c) a_k),
    the sign that of r.  No re-orthonormalisation of R (cv2.Rodrigues runs an SVD first)."""
    R = np.asarray(R, np.float64)
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) / 2.0
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1.0) / 2.0
    angle = np.arctan2(s, c)
    if c >= -0.5:
        if s == 0.0:
            return np.zeros(3)
        return r * (angle / (2.0 * s))
    B = (R + R.T) / 2.0
    k = int(np.argmax(np.diag(B)))
    a = np.empty(3)
    a[k] = np.sqrt((B[k, k] - c) / (1.0 - c))
    for j in range(3):
        if j != k:
            a[j] = B[k, j] / ((1.0 - c) * a[k])
    a = a / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    if a[0] * r[0] + a[1] * r[1] + a[2] * r[2] < 0.0:
        a = -a
    return a * angle


def matrix_from_rotvec(w):
    """Rodrigues' formula: R = I + sin(angle) [a]x + 2 sin^2(angle / 2) [a]x^2, the identity at the zero vector."""
    w = np.asarray(w, np.float64).reshape(3)
    angle = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if angle == 0.0:
        return np.eye(3)
    a = w / angle
    A = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    h = np.sin(angle / 2.0)
    return np.eye(3) + np.sin(angle) * A + (2.0 * h * h) * (A @ A)


def get_cam_param(K, pose):
    """Reference :459-466: frame parameters -> BAL form [rotation vector, t, f, cx, cy]."""
    K, pose = np.asarray(K, np.float64), np.asarray(pose, np.float64)
    return np.concatenate([rotvec_from_matrix(pose[:3, :3]), pose[:3, 3], [K[0, 0], K[0, 2], K[1, 2]]])


def get_cam_params_back(cam_params):
    """Reference :443-457: BAL form -> (K [3,3], pose [4,4])."""
    cam_params = np.asarray(cam_params, np.float64)
    f, k1, k2 = cam_params[6], cam_params[7], cam_params[8]
    K = np.array([[f, 0, k1], [0, f, k2], [0, 0, 1]])
    pose_mat = np.eye(4)
    pose_mat[:3, :3] = matrix_from_rotvec(cam_params[:3])
    pose_mat[:3, 3] = cam_params[3:6]
    return K, pose_mat


def mat2euler(M):
    """Static-frame x, y, z Euler angles of a rotation matrix, R = Rz(az) Ry(ay) Rx(ax) (the default of
    transforms3d.euler.mat2euler); at the gimbal lock (cos(ay) below 4 eps) az = 0."""
    M = np.asarray(M, np.float64)
    cy = np.sqrt(M[0, 0] * M[0, 0] + M[1, 0] * M[1, 0])
    if cy > 4.0 * np.finfo(np.float64).eps:
        return np.array([np.arctan2(M[2, 1], M[2, 2]), np.arctan2(-M[2, 0], cy), np.arctan2(M[1, 0], M[0, 0])])
    return np.array([np.arctan2(-M[1, 2], M[1, 1]), np.arctan2(-M[2, 0], cy), 0.0])


def euler2mat(ax, ay, az):
    """R = Rz(az) Ry(ay) Rx(ax), the inverse of ``mat2euler``."""
    sx, cx, sy, cy, sz, cz = np.sin(ax), np.cos(ax), np.sin(ay), np.cos(ay), np.sin(az), np.cos(az)
    return np.array([[cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz],
                     [cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz],
                     [-sy, sx * cy, cx * cy]])


def motion_prediction(pose_list):
    """Reference :275-293 on the last three poses: constant translation and Euler-angle speed.  As written there, ``rot_t``
    is taken from ``pose1``, not from the latest pose."""
    pose0, pose1, pose_t = pose_list[-3], pose_list[-2], pose_list[-1]
    speed_trans = ((pose1[:3, 3] - pose0[:3, 3]) + (pose_t[:3, 3] - pose1[:3, 3])) / 2
    rot0 = mat2euler(pose0[:3, :3])
    rot1 = mat2euler(pose1[:3, :3])
    rot_t = mat2euler(pose1[:3, :3])
    speed_rot = ((rot1 - rot0) + (rot_t - rot1)) / 2
    trans_t = pose_t[:3, 3] + speed_trans
    rot_t = rot_t + speed_rot
    pose_new = np.eye(4)
    pose_new[:3, :3] = euler2mat(rot_t[0], rot_t[1], rot_t[2])
    pose_new[:3, 3] = trans_t
    return pose_new


# ---- the state machine -------------------------------------------------------------------------------------------------------

class TrackerState:
    """The bookkeeping of the reference's BATracker (ba_tracker.py:14-78, 128-235, 468-802), numpy on the host, with the four
    numerical cores left to the subclass:

      ``_match(frame_info_dict) -> matches0 [n_kf]``           the keyframe's keypoints against the frame's (:497-499)
      ``_flow_pnp(frame_info_dict, kf_frame_info) -> (pose [4,4], kpt_dist, kpt_new [n,2], valid_ids)``   :305-327
      ``_update(frame_info_dict, matches0, pose_init) -> (pair_q [m], q_pt_ids [m], new_points [r,3], unmatched [u], log)``   :499-598, :686
      ``_ba(kpt2ds, kpt2d3d_ids, kpt2d_fids, kpt3d_list, cams) -> (points, cams)``                        :358-441
      ``_keyframe_committed()``                                a hook: the keyframe of ``track_ba`` has changed

    Where the reference as written runs, it is followed (the ``len - 1 - n_q`` start at :703, the init counters, the use of the
    ground-truth pose at :328 and :758).  Four places where it raises or corrupts indices are fixed:
      :225-226 concatenates the [P,3] point array with a vector and raises on the second ``add_kf``: ``kpt3d_source_id``
               stays a vector here;
      :715     takes ``len()`` of the tuple ``np.where`` returns (always 1): the count of surviving keypoints is meant;
      :229     indexes the keyframe's database ids by 2D keypoint index: the position in the match list is meant;
      :213-214 hands a later keyframe's known database points the 3D ids in the order and at the positions of
               ``db_3d_list``, which are the keyframe's own order and the 3D ids only until a point is triangulated:
               ``db_3d_index`` (new) keeps the 3D id of every database id and each match looks its own up.
    Index arrays are integer throughout (the reference lets some become float by concatenation)."""

    def __init__(self, win_size=10, frame_interval=5):
        self._set_defaults(win_size, frame_interval)

    def _set_defaults(self, win_size, frame_interval):
        self.kf_frames = dict()
        self.query_frames = dict()
        self.id = 0
        self.last_kf_id = -1
        self.pose_list = []
        self.kpt2ds = []
        self.kpt2d_available_list = []
        self.kpt2d_descs = []
        self.kpt2d_fids = []
        self.cams = []
        self.kf_kpt_index_dict = dict()        # kf_id -> (2d_id_start, 2d_id_end)
        self.db_3d_list = np.array([])
        self.db_3d_index = np.array([], dtype=int)     # the 3D id of each entry of db_3d_list
        self.kpt3d_list = []
        self.kpt3d_sourceid = []
        self.kpt2d3d_ids = []                  # 3D id of each 2D keypoint
        self.update_th = 10
        self.frame_id = 0
        self.last_kf_info = None
        self.win_size = win_size
        self.frame_interval = frame_interval
        self.init_cnt = 3
        self.use_motion_cnt = 0

    def reset(self):
        """Reference :48-78: its second set of defaults (win_size 20, frame_interval 3)."""
        self._set_defaults(20, 3)
        self._keyframe_committed()

    # -- keyframes (:128-235)

    def update_kf(self, kf_info_dict):
        if self.last_kf_info is not None:
            trans_dist, rot_dist = cm_degree_5_metric(kf_info_dict['pose_pred'], self.pose_list[-1])
            if trans_dist > 10 or rot_dist > 10:        # reject invalid updates
                return False
        self.last_kf_info = kf_info_dict
        return True

    def add_kf(self, kf_info_dict):
        self.kf_frames[self.id] = kf_info_dict
        self.pose_list.append(kf_info_dict['pose_pred'])
        kpt_pred = kf_info_dict['kpt_pred']
        keypoints, descriptors = np.asarray(kpt_pred['keypoints']), np.asarray(kpt_pred['descriptors'])
        n_kpt = keypoints.shape[0]
        kf_cam = np.array([get_cam_param(kf_info_dict['K'], kf_info_dict['pose_pred'])])
        valid_2d_id = np.asarray(kf_info_dict['valid_query_id'], dtype=int)
        kf_db_ids = np.asarray(kf_info_dict['kpt3d_ids'])
        mkpts3d = np.asarray(kf_info_dict['mkpts3d'], dtype=np.float64)

        if len(self.kpt2ds) == 0:
            self.cams = kf_cam
            self.kpt2ds = keypoints
            self.kpt2d_match = np.zeros([n_kpt], dtype=int)
            self.kpt2d_descs = descriptors.transpose()
            self.kpt2d_fids = np.ones([n_kpt], dtype=int) * self.id
            self.kf_kpt_index_dict[self.id] = (0, n_kpt - 1)
            self.kpt3d_list = mkpts3d
            self.kpt3d_source_id = np.ones([len(self.kpt3d_list)], dtype=int) * self.id
            self.kpt2d3d_ids = np.ones([n_kpt], dtype=int) * -1
            self.kpt2d3d_ids[valid_2d_id] = np.arange(0, len(mkpts3d))
            self.db_3d_list = kf_db_ids
            self.db_3d_index = np.arange(0, len(mkpts3d))
        else:
            self.cams = np.concatenate([self.cams, kf_cam], axis=0)
            self.kpt2ds = np.concatenate([self.kpt2ds, keypoints], axis=0)
            self.kpt2d_match = np.concatenate([self.kpt2d_match, np.zeros([n_kpt], dtype=int)], axis=0)
            self.kpt2d_descs = np.concatenate([self.kpt2d_descs, descriptors.transpose()], axis=0)
            self.kpt2d_fids = np.concatenate([self.kpt2d_fids, np.ones([n_kpt], dtype=int) * self.id])
            start_id = self.kf_kpt_index_dict[self.last_kf_id][-1] + 1
            self.kf_kpt_index_dict[self.id] = (start_id, start_id + n_kpt - 1)

            # 3D points the keyframe shares with the map keep their id, the others are appended
            intersect_kpts = np.intersect1d(self.db_3d_list, kf_db_ids)
            mask_kf_3d_exist = np.isin(kf_db_ids, intersect_kpts)
            new_pos = np.where(~mask_kf_3d_exist)[0]
            kf_kpt3ds_new = mkpts3d[new_pos]
            kf_kpt2d3d_id = np.ones([n_kpt], dtype=int) * -1
            order = np.argsort(self.db_3d_list, kind="stable")
            seen = kf_db_ids[np.where(mask_kf_3d_exist)[0]]
            kf_kpt2d3d_id[valid_2d_id[np.where(mask_kf_3d_exist)[0]]] = self.db_3d_index[order[np.searchsorted(self.db_3d_list, seen, sorter=order)]]
            kpt3d_start_id = len(self.kpt3d_list)
            kf_kpt2d3d_id[valid_2d_id[new_pos]] = np.arange(kpt3d_start_id, kpt3d_start_id + len(kf_kpt3ds_new))
            self.kpt2d3d_ids = np.concatenate([self.kpt2d3d_ids, kf_kpt2d3d_id], axis=0)
            self.kpt3d_list = np.concatenate([self.kpt3d_list, kf_kpt3ds_new], axis=0)
            self.kpt3d_source_id = np.concatenate([self.kpt3d_source_id, np.ones(kf_kpt3ds_new.shape[0], dtype=int) * self.id])
            self.db_3d_list = np.concatenate([self.db_3d_list, kf_db_ids[new_pos]])
            self.db_3d_index = np.concatenate([self.db_3d_index, np.arange(kpt3d_start_id, kpt3d_start_id + len(kf_kpt3ds_new))])

        self.last_kf_info = kf_info_dict
        self.last_kf_id = self.id
        self.id += 1
        self._keyframe_committed()

    # -- one frame (:295-356, :468-802)

    def flow_track(self, frame_info_dict, kf_frame_info):
        pose_init_homo, kpt_dist, kpt_new, valid_ids = self._flow_pnp(frame_info_dict, kf_frame_info)
        trans_dist, rot_dist = cm_degree_5_metric(pose_init_homo, frame_info_dict['pose_gt'])
        if trans_dist <= 7 and rot_dist <= 7 and kpt_dist < 10:
            frame_info_dict['mkpts3d'] = np.asarray(kf_frame_info['mkpts3d'])[valid_ids]
            frame_info_dict['mkpts2d'] = kpt_new[valid_ids]
            self.last_kf_info = frame_info_dict
        return pose_init_homo, kpt_dist

    def apply_ba(self, kpt2ds, kpt2d3d_ids, kpt2d_fids, kpt3d_list, cams, verbose=False):
        return self._ba(kpt2ds, kpt2d3d_ids, kpt2d_fids, kpt3d_list, cams)

    def track_ba(self, frame_info_dict, verbose=False):
        ba_log = dict()
        pose_init = frame_info_dict['pose_init']
        kpt_pred_query = frame_info_dict['kpt_pred']
        kpt_pred_query.pop('scores', None)
        q_keypoints, q_descriptors = np.asarray(kpt_pred_query['keypoints']), np.asarray(kpt_pred_query['descriptors'])
        n_q = len(q_keypoints)

        matches0 = self._match(frame_info_dict)
        pair_q, query_2d3d_ids, new_points, unmatched_idx, log = self._update(frame_info_dict, matches0, pose_init)
        ba_log.update(log)
        mkpts2d_query = q_keypoints[pair_q]
        n_kpt_q = len(pair_q)

        kpt2ds_f = np.concatenate([self.kpt2ds, mkpts2d_query])
        kpt2d3d_ids_f = np.concatenate([self.kpt2d3d_ids, np.asarray(query_2d3d_ids, dtype=int)])
        kpt3d_list_f = np.concatenate([self.kpt3d_list, new_points]) if len(new_points) > 0 else np.copy(self.kpt3d_list)
        cams_f = np.concatenate([self.cams, [get_cam_param(frame_info_dict['K'], pose_init)]])
        kpt2d_fids_f = np.concatenate([self.kpt2d_fids, np.ones([n_kpt_q], dtype=int) * self.id])

        kpt3d_list_f, cams_f = self.apply_ba(kpt2ds_f, kpt2d3d_ids_f, kpt2d_fids_f, kpt3d_list_f, cams_f)
        _, pose_opt = get_cam_params_back(cams_f[-1])

        for key, pose in (('pred', frame_info_dict['pose_pred']), ('init', pose_init), ('opt', pose_opt)):
            trans_dist, rot_dist = cm_degree_5_metric(pose, frame_info_dict['pose_gt'])
            ba_log[key + '_err_trans'] = np.round(trans_dist, decimals=2)
            ba_log[key + '_err_rot'] = np.round(rot_dist, decimals=2)

        update_valid = True
        if (self.frame_id % self.frame_interval == 0 and update_valid) or self.init_cnt > 0:
            num_unmatch = len(unmatched_idx)
            self.kpt2ds = np.concatenate([kpt2ds_f, q_keypoints[unmatched_idx]])
            self.kpt2d_descs = np.concatenate([self.kpt2d_descs, q_descriptors[:, pair_q].transpose(),
                                               q_descriptors[:, unmatched_idx].transpose()])
            self.kpt2d_fids = np.concatenate([kpt2d_fids_f, np.ones(num_unmatch, dtype=int) * kpt2d_fids_f[-1]])
            self.cams = cams_f
            self.kpt3d_source_id = np.concatenate([self.kpt3d_source_id,
                                                   np.ones([len(kpt3d_list_f) - len(self.kpt3d_list)], dtype=int) * self.id])
            self.kpt3d_list = kpt3d_list_f
            self.kpt2d3d_ids = np.concatenate([kpt2d3d_ids_f, np.ones(num_unmatch, dtype=int) * -1])
            frame_info_dict['pose_pred'] = pose_init

            self.kf_kpt_index_dict[self.id] = (len(self.kpt2d_fids) - 1 - n_q, len(self.kpt2d_fids) - 1)
            self.kf_frames.pop(self.last_kf_id)
            self.kf_frames[self.id] = frame_info_dict
            self.last_kf_id = self.id
            self.id += 1

            if np.max(self.kpt2d_fids) > self.win_size:
                valid_idx_fid = np.where(self.kpt2d_fids > np.max(self.kpt2d_fids) - self.win_size)[0]
                num_del = len(self.kpt2d_fids) - len(valid_idx_fid)
                start_idx, end_idx = self.kf_kpt_index_dict[self.last_kf_id]
                self.kf_kpt_index_dict[self.last_kf_id] = (start_idx - num_del, end_idx - num_del)
                self.kpt2d_fids = self.kpt2d_fids[valid_idx_fid]
                self.kpt2ds = self.kpt2ds[valid_idx_fid]
                self.kpt2d3d_ids = self.kpt2d3d_ids[valid_idx_fid]
                self.kpt2d_descs = self.kpt2d_descs[valid_idx_fid]
            self._keyframe_committed()

        self.frame_id += 1
        return pose_opt, ba_log, update_valid

    def motion_prediction(self):
        return motion_prediction(self.pose_list)

    def track(self, frame_info_dict, flow_track_only=False, auto_mode=False):
        if not auto_mode:
            pose_ftk, kpt_dist = self.flow_track(frame_info_dict, self.last_kf_info)
            trans_dist_fkt, rot_dist_fkt = cm_degree_5_metric(self.pose_list[-1], pose_ftk)
            pose_mo = frame_info_dict['pose_pred'] if len(self.pose_list) < 3 else self.motion_prediction()
            # motion prediction when keypoint tracking is not valid
            if ((trans_dist_fkt > 10 or rot_dist_fkt > 10) and self.use_motion_cnt < 3) or kpt_dist > 10:
                frame_info_dict['pose_init'] = pose_mo
                self.use_motion_cnt += 1
            elif trans_dist_fkt < 20 and rot_dist_fkt < 20:
                frame_info_dict['pose_init'] = pose_ftk
                self.use_motion_cnt = 0
            else:
                frame_info_dict['pose_init'] = pose_mo
                self.use_motion_cnt += 1
            if self.init_cnt > 0:       # initialize with gt
                self.init_cnt -= 1
                frame_info_dict['pose_init'] = frame_info_dict['pose_gt']
        else:
            if self.init_cnt > 0:
                self.init_cnt -= 1
                frame_info_dict['pose_init'] = frame_info_dict['pose_gt']
            else:
                frame_info_dict['pose_init'] = self.motion_prediction()

        if not flow_track_only:
            pose_opt, ba_log, _ = self.track_ba(frame_info_dict, verbose=False)
            self.pose_list.append(pose_opt)
        else:
            pose_init = pose_opt = frame_info_dict['pose_init']
            ba_log = dict()
            for key, pose in (('pred', frame_info_dict['pose_pred']), ('init', pose_init), ('opt', pose_opt)):
                trans_dist, rot_dist = cm_degree_5_metric(pose, frame_info_dict['pose_gt'])
                ba_log[key + '_err_trans'] = np.round(trans_dist, decimals=2)
                ba_log[key + '_err_rot'] = np.round(rot_dist, decimals=2)
            self.pose_list.append(frame_info_dict['pose_init'])
        return frame_info_dict['pose_init'], pose_opt, ba_log

    def _keyframe_committed(self):
        pass


class BATracker(TrackerState):
    """Drop-in for the reference's ``BATracker`` (``update_kf`` / ``add_kf`` / ``track``) on the five HIP cores.

    ``matcher``: a ``NearestNeighbour``; ``flow``: a ``FlowTracker``; ``adjuster``: a ``BundleAdjuster``; ``updater``: a
    ``MapUpdater`` (each built on first use when None).  The current keyframe's keypoints, descriptors and 3D ids, the map's
    points and the pyramid of the flow step's reference image are kept on the device from the moment they are committed; a
    tracked frame uploads only its own data.

    Host reads of device values per tracked frame, each where the reference's control flow reads a number: the flow step's
    pose and distance (1) and its points and status (2), the update's summary (1) and the rows it counts (2: the integer rows,
    the new points), the solve's cameras and points (2): 8, of which 3 only with ``auto_mode=False``."""

    def __init__(self, win_size=10, frame_interval=5, matcher=None, flow=None, adjuster=None, updater=None, device="cuda"):
        super().__init__(win_size, frame_interval)
        self.device = torch.device(device)
        self.matcher, self.flow, self.adjuster, self.updater = matcher, flow, adjuster, updater
        self._kf_dev = None           # the keyframe of track_ba on the device
        self._flow_ref = None         # (frame dict, pyramid, mkpts2d, mkpts3d) of the flow step's reference frame

    def _cores(self):
        from .bundle_adjust import BundleAdjuster
        from .flow import FlowTracker
        from .nearest_neighbour import NearestNeighbour
        if self.matcher is None:
            self.matcher = NearestNeighbour()
        if self.flow is None:
            self.flow = FlowTracker()
        if self.adjuster is None:
            self.adjuster = BundleAdjuster()
        if self.updater is None:
            self.updater = MapUpdater()

    def _to(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype={torch.float32: np.float32, torch.float64: np.float64,
                                                               torch.int32: np.int32, torch.uint8: np.uint8}[dtype])).to(self.device)

    def _keyframe_committed(self):
        """Upload what the next frames read of the keyframe: once per keyframe."""
        self._kf_dev = None
        if self.last_kf_id < 0:
            self._flow_ref = None
            return
        start, end = self.kf_kpt_index_dict[self.last_kf_id]
        idx = np.arange(start, end + 1)
        info = self.kf_frames[self.last_kf_id]
        self._kf_dev = dict(
            xy=self._to(self.kpt2ds[idx], torch.float32),
            desc=self._to(self.kpt2d_descs[idx].transpose()[None], torch.float32),
            pt_ids=self._to(self.kpt2d3d_ids[idx], torch.int32),
            points=self._to(self.kpt3d_list, torch.float64),
            K=self._to(info['K'], torch.float64),
            pose=self._to(np.asarray(info['pose_pred'], np.float64)[:3], torch.float64))

    def _flow_reference(self, kf_frame_info):
        if self._flow_ref is None or self._flow_ref[0] is not kf_frame_info:
            self._cores()
            self._flow_ref = (kf_frame_info, self.flow.pyramid(self._to(kf_frame_info['im_path'], torch.uint8)),
                              self._to(kf_frame_info['mkpts2d'], torch.float32), self._to(kf_frame_info['mkpts3d'], torch.float32))
        return self._flow_ref

    def _flow_pnp(self, frame_info_dict, kf_frame_info):
        self._cores()
        _, pyr_kf, mkpts2d, mkpts3d = self._flow_reference(kf_frame_info)
        pyr_q = self.flow.pyramid(self._to(frame_info_dict['im_path'], torch.uint8))
        pose, _, _, next_pts, status, kpt_dist = self.flow.flow_track_device(pyr_kf, pyr_q, mkpts2d, mkpts3d, frame_info_dict['K_crop'])
        numbers = torch.cat([pose.reshape(-1), kpt_dist]).cpu().numpy()                 # read 1
        pose_homo = np.eye(4)
        pose_homo[:3] = numbers[:12].reshape(3, 4)
        dist = numbers[12] if numbers[13] > 0 else 1000086.0                           # no point survived: the reference's sentinel
        kpt_new, valid_ids = next_pts.cpu().numpy(), np.where(status.cpu().numpy() == 1)[0]      # reads 2 and 3
        # the frame may become the flow step's reference (flow_track decides): its pyramid is on the device already
        self._pending_flow_ref = (frame_info_dict, pyr_q)
        return pose_homo, dist, kpt_new, valid_ids

    def flow_track(self, frame_info_dict, kf_frame_info):
        out = super().flow_track(frame_info_dict, kf_frame_info)
        frame, pyr = self._pending_flow_ref
        if self.last_kf_info is frame:
            self._flow_ref = (frame, pyr, self._to(frame['mkpts2d'], torch.float32), self._to(frame['mkpts3d'], torch.float32))
        self._pending_flow_ref = None
        return out

    def _match(self, frame_info_dict):
        self._cores()
        desc_q = self._to(np.asarray(frame_info_dict['kpt_pred']['descriptors'])[None], torch.float32)
        return self.matcher({"descriptors0": self._kf_dev["desc"], "descriptors1": desc_q})["matches0"][0]

    def _update(self, frame_info_dict, matches0, pose_init):
        kf = self._kf_dev
        q_xy = self._to(np.asarray(frame_info_dict['kpt_pred']['keypoints']), torch.float32)
        out = self.updater.update(matches0, kf["xy"], q_xy, kf["pt_ids"], kf["points"], kf["K"], self._to(frame_info_dict['K'], torch.float64),
                                  kf["pose"], self._to(np.asarray(pose_init, np.float64)[:3], torch.float64))
        m, known, _, cand, kept, _, _, unmatched = out.summary.cpu().numpy().tolist()                                   # read 1
        rows = torch.cat([out.pair_q[:m], out.q_pt_ids[:m], out.unmatched_q[:unmatched]]).cpu().numpy().astype(int)       # read 2
        new_points = out.new_points[:kept].cpu().numpy()                                                                 # read 3
        log = {'pt_found': known}
        if cand > 0:
            log.update(pt_triang=cand, pt_triang_rm=cand - kept)
        return rows[:m], rows[m:2 * m], new_points, rows[2 * m:], log

    def _ba(self, kpt2ds, kpt2d3d_ids, kpt2d_fids, kpt3d_list, cams):
        self._cores()
        return bundle_adjust.apply_ba(kpt2ds, kpt2d3d_ids, kpt2d_fids, kpt3d_list, cams, self.win_size, device=self.device,
                                      adjuster=self.adjuster)
