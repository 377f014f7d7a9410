"""MI355X-native 2D object detector: host-side mirror of the reference's ``LocalFeatureObjectDetector``
(src/local_feature_2D_detector/local_feature_2D_detector.py), the step that turns a camera frame into the 512 x 512 crop and
``K_crop`` the rest of the chain (SuperPoint -> GATsSuperGlue -> RANSAC-EPnP) starts from.

Same class name, constructor and method contracts.  SuperPoint on the full frame and SuperGlue against the reference views
run as before; the tail -- match selection, partial-affine RANSAC (``cv2.estimateAffinePartial2D``), the box vote, the two
``cv2.warpAffine`` crops and ``get_K_crop_resize`` -- is the HIP library behind include/detector/detector.h.  Reference-view
features stay on the GPU, nothing goes to the host between the matcher and the crop, and there is no OpenCV / CPU fallback.

Not claimed: parity with OpenCV's ``estimateAffinePartial2D`` / ``warpAffine`` themselves (unmeasured: no cv2 where this was
developed).  The RANSAC differs from OpenCV's in three documented ways (hash-drawn samples, all ``iterations`` hypotheses, a
closed-form refit instead of 10 LM steps); the vote reproduces the reference as written: it ranks views by their number of
MATCHES (``inliers.shape[0]`` of cv2's N x 1 mask), not of inliers -- ``rank_by="inliers"`` is offered as a deviation.
"""
from __future__ import annotations

import os
import os.path as osp
import struct
import warnings

import numpy as np
import torch

from . import _native_det, _native_sg
from ._binding import NativeError, WorkspaceCache, gpu_tensor, k_array  # noqa: F401
from .nearest_neighbour import NearestNeighbour
from .superglue import SuperGlue

REPROJ_THRESHOLD = 6.0     # local_feature_2D_detector.py:105
NO_CPU = "onepose_amd.LocalFeatureObjectDetector runs only on a ROCm GPU ({}); there is no CPU fallback"


def _k_array(K):
    k = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K)
    return k_array(k[:, :3] if k.shape == (3, 4) else k)      # get_K_crop_resize accepts the homogeneous form too


# ---- COLMAP image names (only the names are needed; written from COLMAP's published model format) -----------------
def read_colmap_image_names(model_dir):
    """{image_id: name} from ``images.bin`` or ``images.txt`` of a COLMAP model directory.

    images.bin: uint64 image count; per image int32 id, 4 doubles (qvec), 3 doubles (tvec), int32 camera id, the
    zero-terminated name, uint64 point count and that many (double x, double y, int64 point3D id) records.
    images.txt: '#' comments; two lines per image, the first ``IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME``, the second its
    2D points (possibly empty)."""
    bin_path, txt_path = osp.join(model_dir, "images.bin"), osp.join(model_dir, "images.txt")
    names = {}
    if osp.exists(bin_path):
        with open(bin_path, "rb") as f:
            (count,) = struct.unpack("<Q", f.read(8))
            for _ in range(count):
                head = struct.unpack("<i7di", f.read(64))
                name = bytearray()
                while True:
                    c = f.read(1)
                    if c in (b"\0", b""):
                        break
                    name += c
                (npts,) = struct.unpack("<Q", f.read(8))
                f.seek(24 * npts, os.SEEK_CUR)
                names[head[0]] = name.decode("utf-8")
        return names
    if osp.exists(txt_path):
        with open(txt_path) as f:
            lines = f.read().split("\n")
        i = 0
        while i < len(lines):
            line = lines[i].strip()
            i += 1
            if not line or line.startswith("#"):
                continue
            elems = line.split()
            names[int(elems[0])] = " ".join(elems[9:])
            i += 1                              # the image's 2D points
        return names
    raise FileNotFoundError(f"no images.bin / images.txt under {model_dir}")


def sample_reference_ids(names, n_ref_view):
    """The reference's choice of views (:56-60): ``range(1, len(images), len(images) // n_ref_views)`` over image ids."""
    gap = max(1, len(names) // n_ref_view)
    return list(range(1, len(names), gap))


def _read_gray(path):
    """uint8 [H, W] with whatever decoder is importable (image decoding is not part of this package)."""
    try:
        from PIL import Image
        return np.asarray(Image.open(path).convert("L"))
    except ImportError:
        pass
    try:
        import cv2
        img = cv2.imread(path, cv2.IMREAD_GRAYSCALE)
        if img is None:
            raise FileNotFoundError(path)
        return img
    except ImportError:
        raise RuntimeError(f"cannot decode {path}: neither PIL nor cv2 is importable; pass ref_images=[...] (GPU tensors "
                           "[1,1,H,W] in [0, 1]) instead of sfm_ws_dir") from None


def _write_gray(path, img_u8):
    try:
        from PIL import Image
        Image.fromarray(img_u8).save(path)
        return True
    except ImportError:
        pass
    try:
        import cv2
        return bool(cv2.imwrite(path, img_u8))
    except ImportError:
        warnings.warn("detection crop not saved: neither PIL nor cv2 is importable", RuntimeWarning, stacklevel=3)
        return False


class LocalFeatureObjectDetector:
    """extractor: onepose_amd.SuperPoint; matcher: onepose_amd.SuperGlue (its engine is driven directly, the V forwards
    enqueued back to back), onepose_amd.NearestNeighbour (one ragged call over the views, which share the query plane) or any callable with SuperGlue's ``forward(data)`` contract on GPU tensors (called once per view).

    ``ref_images``: list of [1,1,H,W] GPU tensors in [0, 1] -- the reference views, no file reader needed.  ``sfm_ws_dir``
    keeps the reference's meaning: image names from the COLMAP model there, sampled like the reference.
    ``rank_by``: "matches" (the reference as written) or "inliers"; ``iterations``: RANSAC hypotheses (OpenCV's default
    maxIters); ``seed``: of the hash that draws the samples."""

    def __init__(self, extractor, matcher, sfm_ws_dir=None, n_ref_view=15, output_results=False, detect_save_dir=None,
                 K_crop_save_dir=None, *, ref_images=None, rank_by="matches", iterations=2000, seed=0):
        if rank_by not in _native_det.RANK_BY:
            raise ValueError(f"rank_by must be one of {sorted(_native_det.RANK_BY)} (got {rank_by!r})")
        if not torch.cuda.is_available():
            raise RuntimeError(NO_CPU.format("no GPU is visible"))
        self.lib = _native_det.load()
        self.extractor = extractor.cuda()
        self.matcher = matcher.cuda() if hasattr(matcher, "cuda") else matcher
        self.rank_by, self.iterations, self.seed = rank_by, int(iterations), int(seed)
        self.output_results = output_results
        self.detect_save_dir = detect_save_dir
        self.K_crop_save_dir = K_crop_save_dir
        self._workspaces = WorkspaceCache(6)
        self.last = None
        if ref_images is None:
            if sfm_ws_dir is None:
                raise ValueError("give sfm_ws_dir (a COLMAP model directory) or ref_images")
            self.db_dict = self.extract_ref_view_features(sfm_ws_dir, n_ref_view)
        else:
            self.db_dict = self._extract(dict(enumerate(ref_images)))
        self._pack()

    # ---- reference views ----
    def extract_ref_view_features(self, sfm_ws_dir, n_ref_views):
        assert osp.exists(sfm_ws_dir), f"SfM work space:{sfm_ws_dir} not exists!"
        names = read_colmap_image_names(sfm_ws_dir)
        images = {}
        for idx in sample_reference_ids(names, n_ref_views):
            if idx not in names:
                raise KeyError(f"the COLMAP model under {sfm_ws_dir} has no image id {idx} (the reference samples ids 1, 1 + gap, ...)")
            img = torch.from_numpy(np.ascontiguousarray(_read_gray(names[idx]))).cuda()
            images[idx] = (img.to(torch.float32) / 255.0)[None, None]
        return self._extract(images)

    @torch.no_grad()
    def _extract(self, images):
        db = {}
        for idx, img in images.items():
            if not (torch.is_tensor(img) and img.is_cuda):
                raise RuntimeError(NO_CPU.format("a reference image is not a GPU tensor"))
            if img.dim() != 4:
                img = img[None]
            det = self.extractor(img)
            db[idx] = {"keypoints": det["keypoints"][0].contiguous(), "scores": det["scores"][0].contiguous(),
                       "descriptors": det["descriptors"][0].contiguous(), "size": np.array(img.shape[-2:])}
        if not db:
            raise ValueError("no reference views")
        return db

    def _pack(self):
        """Padded device buffers of the reference views: kpts0 [V,cap0,2], n0 [V], hw0 [V,2], and the matcher's outputs; for
        the native matcher's ragged batch also the view-side scores [V,cap0] and descriptors [V,256,cap0] of the views that
        have keypoints (``live``), built once."""
        views = list(self.db_dict.values())
        dev = views[0]["keypoints"].device
        self.device = dev
        self.ids = list(self.db_dict.keys())
        V = len(views)
        cap0 = max(1, max(v["keypoints"].shape[0] for v in views))
        self.V, self.cap0 = V, cap0
        self.kpts0 = torch.zeros(V, cap0, 2, device=dev, dtype=torch.float32)
        for i, v in enumerate(views):
            self.kpts0[i, :v["keypoints"].shape[0]] = v["keypoints"]
        self.n0_host = [int(v["keypoints"].shape[0]) for v in views]
        self.n0 = torch.tensor(self.n0_host, device=dev, dtype=torch.int32)
        self.hw0 = torch.tensor(np.stack([v["size"] for v in views]).astype(np.int32), device=dev)
        self.matches0 = torch.full((V, cap0), -1, device=dev, dtype=torch.int64)
        self.scores0 = torch.zeros(V, cap0, device=dev, dtype=torch.float32)
        self.live = [i for i, n in enumerate(self.n0_host) if n > 0]
        self.view_scores = torch.zeros(V, cap0, device=dev, dtype=torch.float32)
        self.view_desc = torch.zeros(V, views[0]["descriptors"].shape[0], cap0, device=dev, dtype=torch.float32)
        for i, v in enumerate(views):
            self.view_scores[i, :self.n0_host[i]] = v["scores"]
            self.view_desc[i, :, :self.n0_host[i]] = v["descriptors"]
        self.hw0_host = [(int(v["size"][0]), int(v["size"][1])) for v in views]
        self.ragged = True             # native matcher: one ragged batch over the views; False keeps the per-view loop

    def _workspace(self, dev):
        shape = (self.V, self.cap0, self.iterations)
        return self._workspaces.get(shape, dev, self.lib.det_workspace_bytes,
                                    lambda: "det_workspace_bytes({}, {}, {}) refused the shape".format(*shape))

    # ---- stages ----
    def _check_frame(self, query_img):
        if not torch.is_tensor(query_img):
            raise TypeError("query_img must be a tensor [1,1,H,W] (or [1,H,W]) in [0, 1]")
        img = gpu_tensor(query_img if query_img.dim() == 4 else query_img[None], torch.float32, NO_CPU.format("the frame is on {}"))
        if img.dim() != 4 or img.shape[0] != 1 or img.shape[1] != 1:
            raise ValueError("expected one grayscale frame [1,1,H,W]")
        return img

    @torch.no_grad()
    def _match_views(self, kpts1, scores1, desc1, query_hw):
        """V matcher forwards into the padded matches0 / scores0 buffers (rows beyond n0[v] are never read)."""
        n1 = int(kpts1.shape[0])
        dev = kpts1.device
        if n1 == 0:
            self.matches0.fill_(-1)
            return
        native = isinstance(self.matcher, SuperGlue)
        if native and self.ragged and len(self.live) > 1:
            return self._match_views_ragged(kpts1, scores1, desc1, query_hw)
        if isinstance(self.matcher, NearestNeighbour) and self.ragged and len(self.live) > 1:
            return self._match_views_nn(desc1)
        if native:
            m1 = torch.empty(1, n1, device=dev, dtype=torch.int64)
            s1 = torch.empty(1, n1, device=dev, dtype=torch.float32)
        qh, qw = int(query_hw[0]), int(query_hw[1])
        for i, view in enumerate(self.db_dict.values()):
            n0 = self.n0_host[i]
            if n0 == 0:
                continue
            size = view["size"]
            if native:      # SuperGlueEngine.forward writes straight into the slices of the padded buffers
                self.matcher.engine.forward(view["keypoints"][None], view["scores"][None], view["descriptors"][None], kpts1[None],
                                            scores1[None], desc1[None], (int(size[0]), int(size[1])), (qh, qw),
                                            out=(self.matches0[i:i + 1, :n0], m1, self.scores0[i:i + 1, :n0], s1))
            else:
                data = {"keypoints0": view["keypoints"][None], "scores0": view["scores"][None], "descriptors0": view["descriptors"][None],
                        "keypoints1": kpts1[None], "scores1": scores1[None], "descriptors1": desc1[None],
                        "image0": torch.empty(1, 1, int(size[0]), int(size[1]), device="meta"),
                        "image1": torch.empty(1, 1, qh, qw, device="meta")}
                pred = self.matcher(data)
                if not pred["matches0"].is_cuda:
                    raise RuntimeError(NO_CPU.format("the matcher returned host tensors"))
                self.matches0[i, :n0] = pred["matches0"][0].to(torch.int64)
                self.scores0[i, :n0] = pred["matching_scores0"][0]

    def _match_views_ragged(self, kpts1, scores1, desc1, query_hw):
        """The views that have keypoints as ragged batches of the native matcher (bitwise the loop's results): the query side
        is expanded per frame; with no empty view the outputs land straight in matches0 / scores0."""
        n1, dev = int(kpts1.shape[0]), kpts1.device
        engine, step = self.matcher.engine, _native_sg.MAX_ITEMS
        qhw = (int(query_hw[0]), int(query_hw[1]))
        for k in range(0, len(self.live), step):
            live = self.live[k:k + step]
            b = len(live)
            whole = b == self.V
            sel = slice(None) if whole else torch.tensor(live, device=dev)
            m0 = self.matches0 if whole else torch.empty(b, self.cap0, device=dev, dtype=torch.int64)
            s0 = self.scores0 if whole else torch.empty(b, self.cap0, device=dev, dtype=torch.float32)
            m1 = torch.empty(b, n1, device=dev, dtype=torch.int64)
            s1 = torch.empty(b, n1, device=dev, dtype=torch.float32)
            engine.forward_ragged(self.kpts0[sel], self.view_scores[sel], self.view_desc[sel], kpts1[None].expand(b, -1, -1),
                                  scores1[None].expand(b, -1), desc1[None].expand(b, -1, -1), [self.n0_host[i] for i in live],
                                  [n1] * b, [self.hw0_host[i] for i in live], [qhw] * b, out=(m0, m1, s0, s1))
            if not whole:
                self.matches0[sel] = m0
                self.scores0[sel] = s0

    def _match_views_nn(self, desc1):
        """The views that have keypoints as ragged batches of the nearest-neighbour matcher (bitwise the loop's results): every
        view reads the ONE query plane; with no empty view the outputs land straight in matches0 / scores0."""
        n1, dev = int(desc1.shape[1]), desc1.device
        engine, step = self.matcher.engine, _native_sg.NNM_MAX_ITEMS
        for k in range(0, len(self.live), step):
            live = self.live[k:k + step]
            b = len(live)
            whole = b == self.V
            sel = slice(None) if whole else torch.tensor(live, device=dev)
            m0 = self.matches0 if whole else torch.empty(b, self.cap0, device=dev, dtype=torch.int64)
            s0 = self.scores0 if whole else torch.empty(b, self.cap0, device=dev, dtype=torch.float32)
            m1 = torch.empty(b, n1, device=dev, dtype=torch.int64)
            s1 = torch.empty(b, n1, device=dev, dtype=torch.float32)
            engine.match_ragged(self.view_desc[sel], desc1, [self.n0_host[i] for i in live], [n1] * b, out=(m0, m1, s0, s1))
            if not whole:
                self.matches0[sel] = m0
                self.scores0[sel] = s0

    @torch.no_grad()
    def _tail(self, kpts1, query_hw):
        """One RANSAC launch over all views and one vote -> dict of device tensors."""
        dev, V, cap0 = self.device, self.V, self.cap0
        ws = self._workspace(dev)
        k1 = gpu_tensor(kpts1, torch.float32, NO_CPU.format("the query keypoints are on {}"))
        out = {"affine": torch.empty(V, 2, 3, device=dev, dtype=torch.float64), "mask": torch.empty(V, cap0, device=dev, dtype=torch.int32),
               "info": torch.empty(V, 4, device=dev, dtype=torch.int32), "boxes": torch.empty(V, 4, device=dev, dtype=torch.int32),
               "bbox": torch.empty(4, device=dev, dtype=torch.int32), "best_view": torch.empty(1, device=dev, dtype=torch.int32)}
        _native_det.call("det_affine_partial_from_matches", dev, self.kpts0, self.n0, self.matches0, k1 if k1.shape[0] else None, V, cap0,
                         int(k1.shape[0]), REPROJ_THRESHOLD, self.iterations, self.seed, out["affine"], out["mask"], out["info"], ws,
                         ws.numel())
        _native_det.call("det_bbox_vote", dev, out["affine"], out["info"], self.hw0, V, int(query_hw[0]), int(query_hw[1]),
                         _native_det.RANK_BY[self.rank_by], out["boxes"], out["bbox"], out["best_view"])
        return out

    @torch.no_grad()
    def crop_device(self, frame, bbox, K, crop_size=512):
        """crop_img_by_bbox (:160-186) on the GPU: frame [1,1,H,W] fp32 in [0, 1], bbox int32 [4] on the GPU ->
        (crop [1,1,c,c] fp32, K_crop [3,3] float64, info int32 [4] = {ok, w, h, 0}), all on the GPU."""
        dev = frame.device
        H, W = int(frame.shape[-2]), int(frame.shape[-1])
        plane = torch.round(frame.reshape(H, W) * 255.0).clamp_(0, 255).to(torch.uint8)      # exact for frames that were u8 / 255
        crop = torch.empty(1, 1, crop_size, crop_size, device=dev, dtype=torch.float32)
        K_crop = torch.empty(3, 3, device=dev, dtype=torch.float64)
        info = torch.empty(4, device=dev, dtype=torch.int32)
        _native_det.call("det_crop_resize", dev, plane, H, W, bbox, _k_array(K), int(crop_size), crop, K_crop, info)
        return crop, K_crop, info

    @torch.no_grad()
    def detect_device(self, query_img, K, crop_size=512):
        """frame [1,1,H,W] on the GPU -> (bbox int32 [4], crop [1,1,c,c], K_crop [3,3] float64, best_view int32 [1]) left on
        the GPU, nothing synchronised after the extractor's own read of its keypoint count.  ``self.last`` keeps the per-view
        results (affine, mask, info, boxes) and the crop's info for callers that want them."""
        frame = self._check_frame(query_img)
        det = self.extractor(frame)
        kpts1, scores1, desc1 = det["keypoints"][0], det["scores"][0], det["descriptors"][0]
        hw = frame.shape[-2:]
        self._match_views(kpts1, scores1, desc1.contiguous(), hw)
        out = self._tail(kpts1, hw)
        crop, K_crop, crop_info = self.crop_device(frame, out["bbox"], K, crop_size)
        out.update(crop_info=crop_info, keypoints1=kpts1)
        self.last = out
        return out["bbox"], crop, K_crop, out["best_view"]

    # ---- the reference's methods ----
    @torch.no_grad()
    def match_worker(self, query):
        """query: dict(keypoints [n,2], scores [n], descriptors [256,n], size (H, W)) on the GPU (numpy is uploaded) ->
        {view id: {"inliers": cv2-style [n_matches, 1] uint8 mask (empty for a failed view), "bbox": [x0, y0, x1, y1]}}."""
        to = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).to(self.device)      # noqa: E731
        kpts1, scores1, desc1 = (gpu_tensor(to(query[k]), torch.float32, NO_CPU.format("the query features are on {}"))
                                 for k in ("keypoints", "scores", "descriptors"))
        self._match_views(kpts1, scores1, desc1, query["size"])
        out = self._tail(kpts1, query["size"])
        self.last = out
        info, boxes, mask = (out[k].cpu().numpy() for k in ("info", "boxes", "mask"))
        matches = self.matches0.cpu().numpy()
        results = {}
        for i, idx in enumerate(self.ids):
            if not info[i, 0]:
                results[idx] = {"inliers": np.empty((0)), "bbox": boxes[i].copy()}
                continue
            m = matches[i, :self.n0_host[i]]
            valid = (m > -1) & (m < kpts1.shape[0])
            results[idx] = {"inliers": mask[i, :self.n0_host[i]][valid].astype(np.uint8)[:, None], "bbox": boxes[i].copy()}
        return results

    def detect_by_matching(self, query):
        self.match_worker(query)
        return self.last["bbox"].cpu().numpy()

    def crop_img_by_bbox(self, query_img, bbox, K=None, crop_size=512):
        """bbox: numpy [x0, y0, x1, y1] -> (image_crop uint8 [c, c] numpy, K_crop numpy or None)."""
        frame = self._check_frame(query_img)
        box = torch.from_numpy(np.asarray(bbox).astype(np.int32)).to(frame.device)
        crop, K_crop, info = self.crop_device(frame, box, np.eye(3) if K is None else K, crop_size)
        if not int(info[0]):
            raise ValueError(f"empty box {np.asarray(bbox).tolist()}: w and h must be positive")
        img = torch.round(crop[0, 0] * 255.0).to(torch.uint8).cpu().numpy()
        return img, (K_crop.cpu().numpy() if K is not None else None)

    def save_detection(self, crop_img, query_img_path):
        if self.output_results and self.detect_save_dir is not None and query_img_path is not None:
            _write_gray(osp.join(self.detect_save_dir, osp.basename(query_img_path)), crop_img)

    def save_K_crop(self, K_crop, query_img_path):
        if self.output_results and self.K_crop_save_dir is not None and query_img_path is not None:
            np.savetxt(osp.join(self.K_crop_save_dir, osp.splitext(osp.basename(query_img_path))[0] + ".txt"), K_crop)  # K_crop: 3*3

    def _finish(self, bbox, crop, K_crop, crop_info, query_img_path):
        if not int(crop_info[0].item()):
            raise ValueError(f"empty box {bbox.cpu().numpy().tolist()}: w and h must be positive")
        bbox, K_crop = bbox.cpu().numpy(), K_crop.cpu().numpy()
        if self.output_results and self.detect_save_dir is not None:
            self.save_detection(torch.round(crop[0, 0] * 255.0).to(torch.uint8).cpu().numpy(), query_img_path)
        self.save_K_crop(K_crop, query_img_path)
        return bbox, crop, K_crop

    def detect(self, query_img, query_img_path, K, crop_size=512):
        """
        Detect object by local feature matching and crop image (:196-230).
        Input:
            query_image: tensor[1*1*H*W] on the GPU (the frame; the path is only used for the optional save),
            query_img_path: str or None,
            K: np.ndarray[3*3], intrinsic matrix of original image
        Output:
            bounding_box: np.ndarray[x0, y0, x1, y1]
            cropped_image: torch.tensor[1 * 1 * crop_size * crop_size] (normalized) on the GPU,
            cropped_K: np.ndarray[3*3];
        """
        bbox, crop, K_crop, _ = self.detect_device(query_img, K, crop_size)
        return self._finish(bbox, crop, K_crop, self.last["crop_info"], query_img_path)

    def previous_pose_detect(self, query_img, K, pre_pose, bbox3D_corner, crop_size=512, query_img_path=None):
        """
        Detect object by projecting 3D bbox with estimated last frame pose (:232-259).
        Input:
            query_image: tensor[1*1*H*W] on the GPU,
            K: np.ndarray[3*3], intrinsic matrix of original image
            pre_pose: np.ndarray[3*4] or [4*4], pose of last frame
            bbox3D_corner: np.ndarray[8*3], corner coordinate of annotated 3D bbox
        Output: as detect().
        """
        frame = self._check_frame(query_img)
        K = np.asarray(K, dtype=np.float64)
        pose = np.asarray(pre_pose, dtype=np.float64)[:3]
        pts = np.asarray(bbox3D_corner, dtype=np.float64).reshape(-1, 3)
        proj = (K[:, :3] @ pose @ np.concatenate([pts, np.ones((len(pts), 1))], axis=1).T)        # vis_utils.reproj :209-236
        proj = (proj[:2] / proj[2:]).T
        x0, y0 = np.min(proj, axis=0)
        x1, y1 = np.max(proj, axis=0)
        bbox = torch.from_numpy(np.array([x0, y0, x1, y1]).astype(np.int32)).to(frame.device)
        crop, K_crop, info = self.crop_device(frame, bbox, K, crop_size)
        return self._finish(bbox, crop, K_crop, info, query_img_path)
