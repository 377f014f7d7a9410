"""MI355X-native windowed bundle adjustment: Levenberg-Marquardt on the exact Schur complement, on HIP kernels.

Two faces of the C ABI of ``include/mapping/bundle_adjust.h``:

``BundleAdjuster.solve`` takes and returns GPU tensors; ``apply_ba`` is the drop-in for the numerical core of the reference's
keyframe tracker, ``src/tracker/ba_tracker.py:358-441`` (``BATracker.apply_ba``): numpy in, numpy out, the window rule and the
per-observation intrinsics as written there.  The reference hands the optimisation to DeepLM; the solver here is the
published Ceres-style trust-region LM (see the header for what is and is not claimed).  There is no PyTorch compute path and
no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native_map
from ._binding import Engine, gpu_tensor

NO_CPU = "onepose_amd.BundleAdjuster runs only on a ROCm GPU ({} on {}); there is no CPU fallback"


def _gpu(t, name, dtype=torch.float64):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor on a GPU (got {type(t).__name__})")
    return gpu_tensor(t, dtype, NO_CPU.format(name + " is", "{}"))


class BundleAdjuster(Engine):
    """Raw-tensor entry to the HIP bundle adjustment: workspaces cached per (C, P, M, device, stream); no weights."""

    native = _native_map
    WORKSPACE_BYTES, LAST_ERROR = "ba_workspace_bytes", "map_last_error"
    PARAMETER_REFUSAL = NO_CPU.format("a parameter is", "{}")
    MAX_CACHED_WORKSPACES = 8

    def __init__(self):
        super().__init__(None)

    def _problem(self, cams, intr, points, obs_cam, obs_pt, obs_xy, cam_fixed, pt_fixed):
        cams, intr, points, obs_xy = _gpu(cams, "cams"), _gpu(intr, "intr"), _gpu(points, "points"), _gpu(obs_xy, "obs_xy")
        obs_cam, obs_pt = _gpu(obs_cam, "obs_cam", torch.int32), _gpu(obs_pt, "obs_pt", torch.int32)
        C, P, M = cams.shape[0], points.shape[0], obs_cam.shape[0]
        if cams.shape != (C, 6) or intr.shape != (C, 4) or points.shape != (P, 3):
            raise ValueError("cams must be [C,6], intr [C,4] and points [P,3]")
        if obs_cam.shape != (M,) or obs_pt.shape != (M,) or obs_xy.shape != (M, 2):
            raise ValueError("obs_cam and obs_pt must be [M] and obs_xy [M,2]")
        if cam_fixed is not None:
            cam_fixed = _gpu(cam_fixed, "cam_fixed", torch.int32)
            if cam_fixed.shape != (C,):
                raise ValueError("cam_fixed must be [C]")
        if pt_fixed is not None:
            pt_fixed = _gpu(pt_fixed, "pt_fixed", torch.int32)
            if pt_fixed.shape != (P,):
                raise ValueError("pt_fixed must be [P]")
        return cams, intr, points, obs_cam, obs_pt, obs_xy, cam_fixed, pt_fixed, C, P, M

    def solve(self, cams, intr, points, obs_cam, obs_pt, obs_xy, cam_fixed=None, pt_fixed=None, num_iterations=5,
              num_success_iterations=5):
        """cams [C,6] (angle-axis, translation), intr [C,4] (fx, fy, cx, cy), points [P,3], obs_cam / obs_pt [M] integer,
        obs_xy [M,2], optional masks cam_fixed [C] / pt_fixed [P] (non-zero = held fixed), all on one GPU ->
        (cams [C,6], points [P,3], trace [num_iterations,6], summary [6]), fp64, left on the GPU; the inputs are not written.
        trace: cost, candidate cost, model decrease, rho, mu used, accepted (-1 = not attempted); summary: initial cost, final
        cost, accepted, attempted, ignored observations, status."""
        cams, intr, points, obs_cam, obs_pt, obs_xy, cam_fixed, pt_fixed, C, P, M = self._problem(
            cams, intr, points, obs_cam, obs_pt, obs_xy, cam_fixed, pt_fixed)
        dev = cams.device
        cams_out, points_out = cams.clone(), points.clone()
        trace = torch.empty(int(num_iterations), _native_map.BA_TRACE_COLUMNS, device=dev, dtype=torch.float64)
        summary = torch.empty(_native_map.BA_SUMMARY_ENTRIES, device=dev, dtype=torch.float64)
        ws = self.workspace(C, P, M, dev)
        self.call("ba_solve", dev, cams_out, intr, points_out, obs_cam, obs_pt, obs_xy, cam_fixed, pt_fixed, C, P, M, int(num_iterations),
                  int(num_success_iterations), trace, summary, ws, ws.numel())
        return cams_out, points_out, trace, summary

    def linearize(self, cams, intr, points, obs_cam, obs_pt, obs_xy):
        """Stage: residuals r [M,2] and Jacobians Jc [M,2,6], Jp [M,2,3] of every observation."""
        cams, intr, points, obs_cam, obs_pt, obs_xy, _, _, C, P, M = self._problem(cams, intr, points, obs_cam, obs_pt, obs_xy, None, None)
        dev = cams.device
        r = torch.empty(M, 2, device=dev, dtype=torch.float64)
        Jc = torch.empty(M, 2, 6, device=dev, dtype=torch.float64)
        Jp = torch.empty(M, 2, 3, device=dev, dtype=torch.float64)
        self.call("ba_linearize", dev, cams, intr, points, obs_cam, obs_pt, obs_xy, C, P, M, r, Jc, Jp)
        return r, Jc, Jp

    def normal_blocks(self, r, Jc, Jp, obs_cam, obs_pt, C, P, cam_fixed=None, pt_fixed=None):
        """Stage: U [C,6,6], V [P,3,3], g_c [C,6], g_p [P,3] and the per-camera costs [C] of a linearisation."""
        dev, M = r.device, r.shape[0]
        U, V = torch.empty(C, 6, 6, device=dev, dtype=torch.float64), torch.empty(P, 3, 3, device=dev, dtype=torch.float64)
        g_c, g_p = torch.empty(C, 6, device=dev, dtype=torch.float64), torch.empty(P, 3, device=dev, dtype=torch.float64)
        cost_cam = torch.empty(C, device=dev, dtype=torch.float64)
        ws = self.workspace(C, P, M, dev)
        self.call("ba_normal_blocks", dev, r, Jc, Jp, obs_cam, obs_pt, cam_fixed, pt_fixed, C, P, M, U, V, g_c, g_p, cost_cam, ws, ws.numel())
        return U, V, g_c, g_p, cost_cam

    def step(self, U, V, g_c, g_p, r, Jc, Jp, obs_cam, obs_pt, mu, cam_fixed=None, pt_fixed=None):
        """Stage: the damped step (delta_c [C,6], delta_p [P,3], model decrease [1]) at ``mu``."""
        dev, C, P, M = r.device, U.shape[0], V.shape[0], r.shape[0]
        delta_c, delta_p = torch.empty(C, 6, device=dev, dtype=torch.float64), torch.empty(P, 3, device=dev, dtype=torch.float64)
        model_decrease = torch.empty(1, device=dev, dtype=torch.float64)
        ws = self.workspace(C, P, M, dev)
        self.call("ba_step", dev, U, V, g_c, g_p, r, Jc, Jp, obs_cam, obs_pt, cam_fixed, pt_fixed, C, P, M, float(mu), delta_c, delta_p,
                  model_decrease, ws, ws.numel())
        return delta_c, delta_p, model_decrease


def window_observations(kpt2d3d_ids, kpt2d_fids, win_size):
    """ba_tracker.py:362-365: the indices of the observations that enter the adjustment."""
    kpt2d3d_ids, kpt2d_fids = np.asarray(kpt2d3d_ids), np.asarray(kpt2d_fids)
    valid = np.where(kpt2d3d_ids != -1)[0]
    if np.max(kpt2d_fids) > win_size:
        in_window = np.where(kpt2d_fids > np.max(kpt2d_fids) - win_size)
        valid = np.intersect1d(in_window, valid)
    return valid


def compact_problem(kpt2ds, kpt2d3d_ids, kpt2d_fids, kpt3d_list, cams, win_size):
    """The problem ``apply_ba`` hands to the solver: the window's observations over the cameras and points they name,
    renumbered densely in ascending order.  Returns (cam_ids, pt_ids, cams6 [c,6], intr [c,4], points [p,3], obs_cam [m] int32,
    obs_pt [m] int32, obs_xy [m,2]); cam_ids / pt_ids index the caller's arrays."""
    valid = window_observations(kpt2d3d_ids, kpt2d_fids, win_size)
    cams = np.asarray(cams, dtype=np.float64)
    fids = np.asarray(kpt2d_fids)[valid].astype(np.int64)
    pids = np.asarray(kpt2d3d_ids)[valid].astype(np.int64)
    cam_ids, obs_cam = np.unique(fids, return_inverse=True)
    pt_ids, obs_pt = np.unique(pids, return_inverse=True)
    sel = cams[cam_ids]
    intr = np.stack([sel[:, 6], sel[:, 6], sel[:, 7], sel[:, 8]], axis=1)      # BAL: f, cx, cy -> fx = fy = f
    points = np.asarray(kpt3d_list, dtype=np.float64)[pt_ids]
    xy = np.asarray(kpt2ds, dtype=np.float64)[valid]
    return (cam_ids, pt_ids, np.ascontiguousarray(sel[:, :6]), np.ascontiguousarray(intr), np.ascontiguousarray(points),
            obs_cam.astype(np.int32), obs_pt.astype(np.int32), np.ascontiguousarray(xy))


_adjuster = None


def apply_ba(kpt2ds, kpt2d3d_ids, kpt2d_fids, kpt3d_list, cams, win_size, device="cuda", adjuster=None):
    """Drop-in for ``BATracker.apply_ba`` (reference :358-441) with ``win_size`` = the tracker's ``self.win_size``:
    kpt2ds [N,2], kpt2d3d_ids [N] (-1 = no 3D point), kpt2d_fids [N] (rows of ``cams``), kpt3d_list [P,3], cams [F,9] in BAL
    form (angle-axis, translation, f, cx, cy) -> (points_opt [P,3] float64, cam_opt [F,9] float64), 5 LM iterations.  Cameras
    and points no window observation names come back unchanged (the ABI's camera limit applies to the window)."""
    global _adjuster
    if adjuster is None:
        if _adjuster is None:
            _adjuster = BundleAdjuster()
        adjuster = _adjuster
    cams = np.asarray(cams, dtype=np.float64)
    points_opt = np.array(kpt3d_list, dtype=np.float64)
    cam_ids, pt_ids, cams6, intr, points, obs_cam, obs_pt, obs_xy = compact_problem(kpt2ds, kpt2d3d_ids, kpt2d_fids, kpt3d_list, cams, win_size)
    to = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    cams_new, points_new, _, _ = adjuster.solve(to(cams6), to(intr), to(points), to(obs_cam), to(obs_pt), to(obs_xy), num_iterations=5,
                                                num_success_iterations=5)
    cam_opt = cams.copy()
    cam_opt[cam_ids, :6] = cams_new.cpu().numpy()
    points_opt[pt_ids] = points_new.cpu().numpy()
    return points_opt, cam_opt
