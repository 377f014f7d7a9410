"""RANSAC-EPnP pose from 2D-3D correspondences on the GPU: host-side mirror of the reference's
``ransac_PnP`` (src/utils/eval_utils.py:18-42) and ``query_pose_error`` (:45-63).

``ransac_PnP(K, pts_2d, pts_3d, scale)`` keeps the reference signature and return convention
(``pose [3,4]``, ``pose_homo [4,4]``, ``inliers [m,1]`` as numpy; identity + ``[]`` when the solve fails, :40-42).
``ransac_pnp_device`` leaves everything in HBM (inputs: the ``mkpts2d`` / ``mkpts3d`` tensors of ``FrameMatcher``).
``ransac_pnp_batch`` / ``ransac_pnp_from_matches_batch`` solve many frames (padded to one capacity) in one chain of launches;
every frame's result is bitwise the single-frame call's.
The solver is the HIP library behind include/pnp.h; there is no cv2 / CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native_pnp
from ._binding import NativeError, gpu_tensor, k_array as _k_array  # noqa: F401

NO_CPU = "onepose_amd.pnp runs only on a ROCm GPU (there is no CPU fallback)"
REPROJ_ERROR = 5.0        # eval_utils.py:30
ITERATIONS = 10000        # eval_utils.py:31


@torch.no_grad()
def ransac_pnp_device(K, pts_2d, pts_3d, scale=1.0, reproj_error=REPROJ_ERROR, iterations=ITERATIONS, seed=0):
    """pts_2d [n,2], pts_3d [n,3] GPU tensors -> (pose [3,4] float64, inlier_mask [n] int32, info [4] int32:
    ok, inliers, best hypothesis, its count), all on the GPU, nothing synchronised."""
    p2, p3 = gpu_tensor(pts_2d, torch.float32, NO_CPU), gpu_tensor(pts_3d, torch.float32, NO_CPU)
    dev = p2.device
    n = p2.shape[0]
    lib = _native_pnp.load()
    nbytes = lib.pnp_workspace_bytes(n, iterations)
    ws = torch.empty(max(nbytes, 256), device=dev, dtype=torch.uint8)
    pose = torch.empty(3, 4, device=dev, dtype=torch.float64)
    mask = torch.zeros(max(n, 1), device=dev, dtype=torch.int32)
    info = torch.zeros(4, device=dev, dtype=torch.int32)
    _native_pnp.call("pnp_ransac_epnp", dev, p3, p2, _k_array(K), float(scale), n, float(reproj_error), int(iterations), int(seed),
                     pose, mask, info, ws, ws.numel())
    return pose, mask[:n], info


@torch.no_grad()
def ransac_pnp_from_matches(K, kpts2d, kpts3d, matches0, scale=1.0, reproj_error=REPROJ_ERROR, iterations=ITERATIONS, seed=0):
    """inference.py:148-155 without a host round trip: kpts2d [n1,2] (extractor), kpts3d [N3,3] (database), matches0 [n1]
    int64 (-1 = unmatched), all on the GPU -> (pose [3,4] float64, inlier_mask [n1] int32 per query keypoint, info [4])."""
    k2, k3 = gpu_tensor(kpts2d, torch.float32, NO_CPU), gpu_tensor(kpts3d, torch.float32, NO_CPU)
    m0 = gpu_tensor(matches0, torch.int64, NO_CPU)
    dev = k2.device
    n1 = k2.shape[0]
    lib = _native_pnp.load()
    ws = torch.empty(lib.pnp_workspace_bytes(n1, iterations), device=dev, dtype=torch.uint8)
    pose = torch.empty(3, 4, device=dev, dtype=torch.float64)
    mask = torch.empty(n1, device=dev, dtype=torch.int32)
    info = torch.empty(4, device=dev, dtype=torch.int32)
    _native_pnp.call("pnp_ransac_epnp_matches", dev, k2, k3, m0, n1, _k_array(K), float(scale), float(reproj_error), int(iterations),
                     int(seed), pose, mask, info, ws, ws.numel())
    return pose, mask, info


def frame_chunks(b, max_items=_native_pnp.MAX_ITEMS):
    """``range(b)`` in order, in ranges of at most ``max_items`` (itself at most PNP_MAX_ITEMS) frames: one native call each."""
    if not 1 <= max_items <= _native_pnp.MAX_ITEMS:
        raise ValueError(f"max_items must be in [1, {_native_pnp.MAX_ITEMS}] (got {max_items})")
    return [range(i, min(i + max_items, b)) for i in range(0, b, max_items)]


def _batch_host_arguments(K, counts, seeds, b, cap):
    """The per-frame HOST arguments of a batched call, checked: (K [b, 9] float64, counts [b] int32, seeds [b] uint64, taken modulo 2^64)."""
    if isinstance(K, (list, tuple)):
        K = [np.asarray(m.detach().cpu() if isinstance(m, torch.Tensor) else m, dtype=np.float64) for m in K]
    k = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    if k.shape == (3, 3):
        k = np.broadcast_to(k, (b, 3, 3))
    if k.shape != (b, 3, 3):
        raise ValueError(f"K must be [3, 3] or [{b}, 3, 3] (got {list(k.shape)})")
    if counts is None:
        n = np.full(b, cap, np.int64)
    else:
        n = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts, dtype=np.int64).reshape(-1)
    if n.shape != (b,) or (n < 0).any() or (n > cap).any():
        raise ValueError(f"counts must be {b} integers in [0, {cap}]")
    s = [int(seeds)] * b if isinstance(seeds, (int, np.integer)) else [int(v) for v in seeds]
    if len(s) != b:
        raise ValueError(f"seeds must be an int or {b} ints (got {len(s)})")
    s = np.array([v & (2 ** 64 - 1) for v in s], dtype=np.uint64)
    return np.ascontiguousarray(k.reshape(b, 9)), n.astype(np.int32), s


def _host_pointer(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def _batch_outputs(b, cap, dev):
    return (torch.empty(b, 3, 4, device=dev, dtype=torch.float64), torch.empty(b, cap, device=dev, dtype=torch.int32),
            torch.empty(b, 4, device=dev, dtype=torch.int32))


@torch.no_grad()
def ransac_pnp_batch(K, pts_2d, pts_3d, counts=None, scale=1.0, reproj_error=REPROJ_ERROR, iterations=ITERATIONS, seeds=0):
    """pts_2d [b,cap,2], pts_3d [b,cap,3] GPU tensors, frame i holding ``counts[i]`` correspondences (None: all cap; entries past a
    count are never read); K [3,3] or [b,3,3]; seeds an int or b ints -> (pose [b,3,4] float64, inlier_mask [b,cap] int32, zero past
    the count, info [b,4] int32), all on the GPU, nothing synchronised.  Frame i is bitwise ``ransac_pnp_device`` of its own
    correspondences, K and seed; a frame with fewer than 5 gets the identity, a zero mask and info = [0, 0, -1, 0].  More than
    PNP_MAX_ITEMS frames go in chunks of that many."""
    if pts_2d.dim() != 3 or pts_2d.shape[2] != 2 or pts_3d.dim() != 3 or pts_3d.shape[2] != 3 or pts_2d.shape[:2] != pts_3d.shape[:2]:
        raise ValueError(f"pts_2d must be [b, cap, 2] and pts_3d [b, cap, 3] (got {list(pts_2d.shape)} and {list(pts_3d.shape)})")
    if not (pts_2d.is_floating_point() and pts_3d.is_floating_point()):
        raise TypeError(f"pts_2d and pts_3d must be floating-point tensors (got {pts_2d.dtype} and {pts_3d.dtype})")
    p2, p3 = gpu_tensor(pts_2d, torch.float32, NO_CPU), gpu_tensor(pts_3d, torch.float32, NO_CPU)
    dev = p2.device
    b, cap = p2.shape[:2]
    if b < 1 or cap < 1:
        raise ValueError(f"an empty batch: b = {b}, cap = {cap}")
    k, n, s = _batch_host_arguments(K, counts, seeds, b, cap)
    lib = _native_pnp.load()
    pose, mask, info = _batch_outputs(b, cap, dev)
    for r in frame_chunks(b):
        i, j = r.start, r.stop
        ws = torch.empty(lib.pnp_batch_workspace_bytes(j - i, cap, int(iterations)), device=dev, dtype=torch.uint8)
        _native_pnp.call("pnp_ransac_epnp_batch", dev, p3[i:j], p2[i:j], _host_pointer(k[i:j], ctypes.c_double), _host_pointer(n[i:j], ctypes.c_int32),
                         _host_pointer(s[i:j], ctypes.c_uint64), j - i, cap, float(scale), float(reproj_error), int(iterations),
                         pose[i:j], mask[i:j], info[i:j], ws, ws.numel())
    return pose, mask, info


@torch.no_grad()
def ransac_pnp_from_matches_batch(K, kpts2d, kpts3d, matches0, counts=None, scale=1.0, reproj_error=REPROJ_ERROR, iterations=ITERATIONS,
                                  seeds=0):
    """The direct consumer of ``forward_batched``'s ``matches0``: kpts2d [b,cap1,2], matches0 [b,cap1] int64 (-1 = unmatched), frame i
    holding ``counts[i]`` query keypoints (None: all cap1), kpts3d one database [n3,3] for all frames or [b,n3,3] -> (pose [b,3,4]
    float64, inlier_mask [b,cap1] int32 per query keypoint, info [b,4]) on the GPU, nothing synchronised.  Frame i is bitwise
    ``ransac_pnp_from_matches`` of its own keypoints, matches, K and seed."""
    if kpts2d.dim() != 3 or kpts2d.shape[2] != 2 or matches0.shape != kpts2d.shape[:2]:
        raise ValueError(f"kpts2d must be [b, cap1, 2] and matches0 [b, cap1] (got {list(kpts2d.shape)} and {list(matches0.shape)})")
    b, cap1 = kpts2d.shape[:2]
    if kpts3d.shape[-1] != 3 or kpts3d.dim() not in (2, 3) or (kpts3d.dim() == 3 and kpts3d.shape[0] != b) or kpts3d.shape[-2] < 1:
        raise ValueError(f"kpts3d must be [n3, 3] or [{b}, n3, 3] (got {list(kpts3d.shape)})")
    if not (kpts2d.is_floating_point() and kpts3d.is_floating_point()) or matches0.dtype is not torch.int64:
        raise TypeError(f"kpts2d and kpts3d must be floating-point tensors and matches0 int64 (got {kpts2d.dtype}, {kpts3d.dtype} and "
                        f"{matches0.dtype})")
    k2, k3 = gpu_tensor(kpts2d, torch.float32, NO_CPU), gpu_tensor(kpts3d, torch.float32, NO_CPU)
    m0 = gpu_tensor(matches0, torch.int64, NO_CPU)
    dev = k2.device
    if b < 1 or cap1 < 1:
        raise ValueError(f"an empty batch: b = {b}, cap1 = {cap1}")
    shared, n3 = k3.dim() == 2, k3.shape[-2]
    k, n, s = _batch_host_arguments(K, counts, seeds, b, cap1)
    lib = _native_pnp.load()
    pose, mask, info = _batch_outputs(b, cap1, dev)
    for r in frame_chunks(b):
        i, j = r.start, r.stop
        ws = torch.empty(lib.pnp_batch_workspace_bytes(j - i, cap1, int(iterations)), device=dev, dtype=torch.uint8)
        _native_pnp.call("pnp_ransac_epnp_matches_batch", dev, k2[i:j], k3 if shared else k3[i:j], m0[i:j], _host_pointer(k[i:j], ctypes.c_double),
                         _host_pointer(n[i:j], ctypes.c_int32), _host_pointer(s[i:j], ctypes.c_uint64), j - i, cap1, n3, int(shared),
                         float(scale), float(reproj_error), int(iterations), pose[i:j], mask[i:j], info[i:j], ws, ws.numel())
    return pose, mask, info


def ransac_PnP(K, pts_2d, pts_3d, scale=1, iterations=ITERATIONS, seed=0):
    """ solve pnp -- drop-in for eval_utils.ransac_PnP (:18-42); numpy or tensor inputs, numpy outputs."""
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if dev is None:
        raise RuntimeError(NO_CPU)
    to = lambda a: a if isinstance(a, torch.Tensor) and a.is_cuda else torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float32)).to(dev)  # noqa: E731
    p2, p3 = to(pts_2d), to(pts_3d)
    if p2.shape[0] < 5:                       # cv2 raises / returns false for fewer than the 5 model points: :40-42
        return np.eye(4)[:3], np.eye(4), []
    pose, mask, info = ransac_pnp_device(K, p2, p3, scale, REPROJ_ERROR, iterations, seed)
    info = info.cpu().numpy()
    if not info[0]:
        return np.eye(4)[:3], np.eye(4), []
    pose = pose.cpu().numpy()
    inliers = np.nonzero(mask.cpu().numpy())[0].astype(np.int32)[:, None]      # cv2 returns an [m,1] int32 index array
    return pose, np.concatenate([pose, np.array([[0, 0, 0, 1.0]])], axis=0), inliers


@torch.no_grad()
def epnp(K, pts_2d, pts_3d, scale=1.0):
    """EPnP over all correspondences (cv2.solvePnP(flags=SOLVEPNP_EPNP)) -> pose [3,4] float64 on the GPU."""
    p2, p3 = gpu_tensor(pts_2d, torch.float32, NO_CPU), gpu_tensor(pts_3d, torch.float32, NO_CPU)
    pose = torch.empty(3, 4, device=p2.device, dtype=torch.float64)
    _native_pnp.call("pnp_epnp", p2.device, p3, p2, _k_array(K), float(scale), p2.shape[0], pose, None, 0)
    return pose


def query_pose_error(pose_pred, pose_gt):
    """eval_utils.query_pose_error (:45-63): (angular error [deg], translation error [cm]) -- host-side, six flops."""
    pose_pred, pose_gt = np.asarray(pose_pred)[:3], np.asarray(pose_gt)[:3]
    translation_distance = np.linalg.norm(pose_pred[:, 3] - pose_gt[:, 3]) * 100
    trace = np.trace(np.dot(pose_pred[:, :3], pose_gt[:, :3].T))
    trace = trace if trace <= 3 else 3
    return np.rad2deg(np.arccos((trace - 1.0) / 2.0)), translation_distance


class Evaluator:
    """cm-degree pose accuracy over a sequence: host-side mirror of src/evaluators/cmd_evaluator.py (the bookkeeping
    inference.py:102,163,166 does around the pose solver).  A frame counts for the k cm / k degree metric when its
    translation error is below k cm AND its rotation error below k degrees (k = 1, 3, 5)."""

    THRESHOLDS = (1, 3, 5)

    def __init__(self):
        self.cmd1, self.cmd3, self.cmd5, self.cmd7, self.add = [], [], [], [], []

    def _hits(self, k):
        return {1: self.cmd1, 3: self.cmd3, 5: self.cmd5}[k]

    def evaluate(self, pose_pred, pose_gt):
        if pose_pred is None:                      # cmd_evaluator.py:36-40 (also feeds the unused 7 cm list)
            for k in self.THRESHOLDS:
                self._hits(k).append(False)
            self.cmd7.append(False)
            return
        ang, trans = query_pose_error(pose_pred, pose_gt)
        for k in self.THRESHOLDS:
            self._hits(k).append(bool(trans < k and ang < k))

    def summarize(self):
        out = {f"cmd{k}": np.mean(self._hits(k)) for k in self.THRESHOLDS}
        for k in self.THRESHOLDS:
            print(f"{k} cm {k} degree metric: {out[f'cmd{k}']}")
        self.cmd1, self.cmd3, self.cmd5, self.cmd7 = [], [], [], []
        return out
