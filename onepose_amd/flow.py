"""MI355X-native flow step of the keyframe tracker: pyramidal Lucas-Kanade on HIP, to pose.

Host-side mirror of the reference's ``BATracker.kpt_flow_track`` / ``flow_track`` (src/tracker/ba_tracker.py:113-126, 295-356):
the keyframe's PnP-inlier keypoints are tracked into the new crop (``cv2.calcOpticalFlowPyrLK`` with a 15 x 15 window, 2 pyramid
levels above the image, 10 iterations, eps 0.03), PnP is solved on what survived and the mean reprojection distance is measured.
``FlowTracker`` keeps all of it in HBM: two launches for the new frame's pyramid, one for the tracker, the PnP chain of
``onepose_amd.pnp`` fed through ``matches0`` (no compaction on the host) and one for the distance.  ``kpt_flow_track`` is the
numpy-in / numpy-out drop-in.  The kernels are the HIP library behind include/detector/flow.h; there is no cv2 / CPU fallback.

Not claimed: parity with ``cv2.calcOpticalFlowPyrLK`` itself (unmeasured: no cv2 where this was developed).  The header states
the algorithm -- OpenCV's fixed-point arrangement with the per-point algebra in fp64 instead of fp32.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native_det, pnp
from ._binding import NativeError, WorkspaceCache, gpu_tensor, k_array

NO_CPU = "onepose_amd.FlowTracker runs only on a ROCm GPU ({}); there is no CPU fallback"


class ImagePyramid:
    """The packed levels of one image on the GPU (level after level, rows dense).  A keyframe's is built once and reused for
    every frame tracked against it."""

    def __init__(self, data, H, W, levels):
        self.data, self.H, self.W, self.levels = data, H, W, levels

    @property
    def device(self):
        return self.data.device

    def level(self, l):
        """View of level ``l`` as a uint8 [H_l, W_l] tensor."""
        H, W, off = self.H, self.W, 0
        for _ in range(l):
            off += H * W
            H, W = (H + 1) // 2, (W + 1) // 2
        return self.data[off:off + H * W].view(H, W)


class FlowTracker:
    """``win_size``: (win_w, win_h), odd, 3 .. 31; ``max_level``: pyramid levels above the image (fewer are used when a level
    would not be larger than the window); ``max_iter`` / ``eps``: the termination criteria.  Workspaces are cached per
    (n, window, device, stream)."""

    def __init__(self, win_size=(15, 15), max_level=2, max_iter=10, eps=0.03, min_eig_threshold=1e-4):
        self.win = (int(win_size[0]), int(win_size[1]))
        self.max_level, self.max_iter, self.eps = int(max_level), int(max_iter), float(eps)
        self.min_eig_threshold = float(min_eig_threshold)
        if not torch.cuda.is_available():
            raise RuntimeError(NO_CPU.format("no GPU is visible"))
        self.lib = _native_det.load()
        self.call = self.lib.call
        if self.lib.flow_workspace_bytes(0, *self.win) == 0:
            raise ValueError(self.lib.det_last_error().decode())
        self._workspaces = WorkspaceCache(6)

    def _workspace(self, n, dev):
        shape = (n,) + self.win
        return self._workspaces.get(shape, dev, self.lib.flow_workspace_bytes,
                                    lambda: "flow_workspace_bytes: " + self.lib.det_last_error().decode())

    @torch.no_grad()
    def pyramid(self, image):
        """uint8 [H, W] GPU tensor, or a float [0, 1] crop as the detector returns it ([H, W], [1, H, W] or [1, 1, H, W];
        converted as inference_demo.py:251 does, (x * 255) truncated to uint8, on the device) -> ImagePyramid."""
        if not torch.is_tensor(image):
            raise TypeError("image must be a tensor on a GPU")
        if not image.is_cuda:
            raise RuntimeError(NO_CPU.format(f"the image is on {image.device}"))
        while image.dim() > 2 and image.shape[0] == 1:
            image = image[0]
        if image.dim() != 2:
            raise ValueError("expected one grayscale image [H, W]")
        H, W = int(image.shape[0]), int(image.shape[1])
        levels = self.lib.flow_pyramid_levels(H, W, self.win[0], self.win[1], self.max_level)
        if levels == 0:
            raise NativeError("flow_pyramid_levels: " + self.lib.det_last_error().decode())
        dev = image.device
        data = torch.empty(self.lib.flow_pyramid_bytes(H, W, levels - 1), device=dev, dtype=torch.uint8)
        level0 = data[:H * W].view(H, W)
        level0.copy_(image if image.dtype is torch.uint8 else (image * 255).to(torch.uint8))
        self.call("flow_build_pyramid", dev, data, H, W, levels, data)      # level 0 is in place: one launch per further level
        return ImagePyramid(data, H, W, levels)

    def _check_pair(self, pyr_kf, pyr_query):
        if (pyr_kf.H, pyr_kf.W, pyr_kf.levels) != (pyr_query.H, pyr_query.W, pyr_query.levels) or pyr_kf.device != pyr_query.device:
            raise ValueError("the two pyramids must have the same size and levels and live on one device")

    @torch.no_grad()
    def track(self, pyr_kf, pyr_query, pts, init=None, trace=False):
        """pts [n, 2] (fp32, keyframe pixels), optional init [n, 2] (first guess in the query) -> next_pts [n, 2] fp32,
        status [n] int32, matches0 [n] int64 (i where status is 1, else -1), on the GPU, nothing synchronised.
        ``trace=True`` appends trace [n, levels, 2] int32: {iterations run, exit code (_native_det.FLOW_EXIT)}."""
        self._check_pair(pyr_kf, pyr_query)
        p = gpu_tensor(pts, torch.float32, NO_CPU.format("the points are on {}"))
        g = None if init is None else gpu_tensor(init, torch.float32, NO_CPU.format("the initial guess is on {}"))
        dev = pyr_kf.device
        n = int(p.shape[0])
        if p.shape != (n, 2) or (g is not None and g.shape != (n, 2)):
            raise ValueError("pts and init must be [n, 2]")
        next_pts = torch.empty(n, 2, device=dev, dtype=torch.float32)
        status = torch.empty(n, device=dev, dtype=torch.int32)
        matches0 = torch.empty(n, device=dev, dtype=torch.int64)
        tr = torch.empty(n, pyr_kf.levels, 2, device=dev, dtype=torch.int32) if trace else None
        ws = self._workspace(n, dev)
        self.call("flow_track", dev, pyr_kf.data, pyr_query.data, pyr_kf.H, pyr_kf.W, pyr_kf.levels, p, g, n, self.win[0], self.win[1],
                  self.max_iter, self.eps, self.min_eig_threshold, next_pts, status, matches0, tr, ws, ws.numel())
        return (next_pts, status, matches0, tr) if trace else (next_pts, status, matches0)

    @torch.no_grad()
    def reproj_mean(self, pose, K, pts3d, pts2d, status):
        """[2] float64 on the GPU: mean ||project(pts3d, K, pose) - pts2d|| over status == 1, and their number."""
        p3 = gpu_tensor(pts3d, torch.float32, NO_CPU.format("the 3D points are on {}"))
        p2 = gpu_tensor(pts2d, torch.float32, NO_CPU.format("the 2D points are on {}"))
        dev = p3.device
        out = torch.empty(2, device=dev, dtype=torch.float64)
        self.call("flow_reproj_mean", dev, pose, k_array(K), p3, p2, status, int(p3.shape[0]), out)
        return out

    @torch.no_grad()
    def flow_track_device(self, pyr_kf, pyr_query, mkpts2d, mkpts3d, K_crop, seed=0):
        """ba_tracker.py:305-327 without a host round trip: the keyframe's mkpts2d [n, 2] / mkpts3d [n, 3] and the new crop's
        K_crop -> (pose [3, 4] float64, inlier_mask [n] int32, info [4] int32 as onepose_amd.pnp gives them, next_pts [n, 2],
        status [n], kpt_dist [2] float64 = {mean reprojection distance of the tracked points, their number}), on the GPU."""
        next_pts, status, matches0 = self.track(pyr_kf, pyr_query, mkpts2d)
        pose, mask, info = pnp.ransac_pnp_from_matches(K_crop, next_pts, mkpts3d, matches0, seed=seed)      # scale 1, as :322 calls it
        kpt_dist = self.reproj_mean(pose, K_crop, mkpts3d, next_pts, status)
        return pose, mask, info, next_pts, status, kpt_dist


_tracker = None


def kpt_flow_track(im_kf, im_query, kpt2d_last, device="cuda", tracker=None):
    """Drop-in for ``BATracker.kpt_flow_track`` (reference :113-126): im_kf, im_query uint8 [H, W] numpy, kpt2d_last [n, 2] ->
    (kpt_new [n, 2] float32, (valid_ids,)) as numpy, ``valid_ids`` the indices with status 1 (the form of ``np.where``)."""
    global _tracker
    if tracker is None:
        if _tracker is None:
            _tracker = FlowTracker()
        tracker = _tracker
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)  # noqa: E731
    pyr_kf, pyr_query = tracker.pyramid(to(im_kf, np.uint8)), tracker.pyramid(to(im_query, np.uint8))
    next_pts, status, _ = tracker.track(pyr_kf, pyr_query, to(np.asarray(kpt2d_last).reshape(-1, 2), np.float32))
    return next_pts.cpu().numpy(), np.where(status.cpu().numpy().flatten() == 1)
