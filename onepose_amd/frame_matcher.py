"""The per-frame part of the reference inference loop (inference.py:132-152) with every hand-off in HBM.

    extractor(image) -> pack_data -> matcher(inp_data) -> valid matches -> (mkpts2d, mkpts3d, mconf)

The reference moves the detector output to the host and back (``.cpu().numpy()`` at :141, ``torch.Tensor(..).cuda()`` in
``pack_data`` :80-94) and re-uploads the 3D database every frame; here the database dict (``database_io.load_object_database``)
stays resident, the descriptors go from the extractor's output buffer straight into the matcher, and only the final
variable-length correspondence lists are gathered; ``solve_pose`` feeds them, still on the GPU, to the RANSAC-EPnP solver
of ``onepose_amd.pnp`` (``ransac_PnP``, :155).
"""
from __future__ import annotations

import torch


class FrameMatcher:
    """extractor: onepose_amd.SuperPoint; matcher: onepose_amd.GATsSuperGlue; database: the dict of
    ``load_object_database`` (keypoints3d [1,N,3], descriptors3d_db [1,256,N], descriptors2d_db [1,256,N*L])."""

    def __init__(self, extractor, matcher, database, cache_database=True):
        self.extractor, self.matcher, self.db = extractor, matcher, database
        for k in ("keypoints3d", "descriptors3d_db", "descriptors2d_db"):
            if not database[k].is_cuda:
                raise RuntimeError(f"database['{k}'] must live on the GPU (there is no CPU fallback)")
        # the query-independent part of the first three GNN layers, computed once per object
        self.db_cache = matcher.prepare_database(database) if cache_database else None

    @torch.no_grad()
    def __call__(self, image):
        """image [1,1,H,W] on the GPU -> dict(mkpts2d [m,2], mkpts3d [m,3], mconf [m], keypoints2d, matches0) (inference.py:140-152)."""
        det = self.extractor(image)                                           # :140
        kpts2d, desc2d = det["keypoints"][0], det["descriptors"][0]
        inp = {"keypoints2d": kpts2d[None], "keypoints3d": self.db["keypoints3d"],            # pack_data :80-94
               "descriptors2d_query": desc2d[None].contiguous(), "descriptors3d_db": self.db["descriptors3d_db"],
               "descriptors2d_db": self.db["descriptors2d_db"]}
        pred, _ = self.matcher(inp, database=self.db_cache) if self.db_cache is not None else self.matcher(inp)   # :146
        matches, conf = pred["matches0"], pred["matching_scores0"]           # :147-151
        valid = matches > -1
        return {"mkpts2d": kpts2d[valid], "mkpts3d": self.db["keypoints3d"][0][matches[valid]], "mconf": conf[valid],
                "keypoints2d": kpts2d, "matches0": matches}

    @torch.no_grad()
    def solve_pose_device(self, image, K_crop, scale=1000, seed=0):
        """image -> (pose [3,4] float64, inlier mask per query keypoint, info [4], detections) all left on the GPU: the valid
        matches are selected on the device (``pnp_ransac_epnp_matches``), nothing is synchronised after the extractor."""
        from . import pnp
        det = self.extractor(image)
        kpts2d = det["keypoints"][0]
        inp = {"keypoints2d": kpts2d[None], "keypoints3d": self.db["keypoints3d"],
               "descriptors2d_query": det["descriptors"][0][None].contiguous(), "descriptors3d_db": self.db["descriptors3d_db"],
               "descriptors2d_db": self.db["descriptors2d_db"]}
        pred, _ = self.matcher(inp, database=self.db_cache) if self.db_cache is not None else self.matcher(inp)
        pose, mask, info = pnp.ransac_pnp_from_matches(K_crop, kpts2d, self.db["keypoints3d"][0], pred["matches0"], scale=scale, seed=seed)
        return pose, mask, info, det

    def _single(self, det):
        """One frame through the matcher's single-frame path (pack_data :80-94, :146): (matches0, matching_scores0)."""
        kpts2d = det["keypoints"][0]
        inp = {"keypoints2d": kpts2d[None], "keypoints3d": self.db["keypoints3d"],
               "descriptors2d_query": det["descriptors"][0][None].contiguous(), "descriptors3d_db": self.db["descriptors3d_db"],
               "descriptors2d_db": self.db["descriptors2d_db"]}
        pred, _ = self.matcher(inp, database=self.db_cache) if self.db_cache is not None else self.matcher(inp)
        return pred["matches0"].reshape(-1), pred["matching_scores0"].reshape(-1)

    def _match_dets(self, dets):
        """(matches0, matching_scores0) per extractor output: the frames with at least 2 keypoints through ONE ragged matcher batch
        against the resident database (``GATsSuperGlue.match_frames``: each frame bitwise its own single-frame forward), the others
        stay out of the batch and are answered -- or refused -- by the single-frame path exactly as without it."""
        if self.db_cache is None:
            raise RuntimeError("the batched matcher needs the resident database cache (cache_database=True)")
        out = [None] * len(dets)
        batch = [i for i, d in enumerate(dets) if d["keypoints"][0].shape[0] >= 2]
        preds = self.matcher.match_frames([dets[i]["descriptors"][0] for i in batch], self.db_cache) if batch else []
        for i, p in zip(batch, preds):
            out[i] = (p["matches0"], p["matching_scores0"])
        for i, det in enumerate(dets):
            if out[i] is None:
                out[i] = self._single(det)
        return out

    @torch.no_grad()
    def match_frames(self, images):
        """A list (or [B,1,H,W] batch) of crops of this object -> one dict per frame, each what ``__call__`` returns for it.  The
        extractor runs frame by frame, the matcher ONCE over all frames (``_match_dets``)."""
        frames = [images[i:i + 1] for i in range(images.shape[0])] if isinstance(images, torch.Tensor) else list(images)
        dets = [self.extractor(image) for image in frames]
        out = []
        for det, (matches, conf) in zip(dets, self._match_dets(dets)):
            kpts2d = det["keypoints"][0]
            valid = matches > -1
            out.append({"mkpts2d": kpts2d[valid], "mkpts3d": self.db["keypoints3d"][0][matches[valid]], "mconf": conf[valid],
                        "keypoints2d": kpts2d, "matches0": matches})
        return out

    @torch.no_grad()
    def solve_poses_device(self, images, K_crops, scale=1000, seeds=0, batched_matcher=None):
        """A list (or [B,1,H,W] batch) of crops -> (poses [B,3,4] float64, masks [B,cap1] per query keypoint, infos [B,4],
        detections), all left on the GPU.  The extractor runs frame by frame exactly as in ``solve_pose_device`` (each frame
        keeps its own keypoint count), the matcher once over all frames (below); the keypoints and matches go into padded [B, cap1]
        buffers, cap1 the largest count, and ONE batched solve (``pnp_ransac_epnp_matches_batch``) answers all frames: frame i
        bitwise as ``solve_pose_device`` answers it with ``K_crops[i]`` and ``seeds[i]``.  K_crops: [3,3] or B of them; seeds: an
        int or B ints.
        batched_matcher: True = the matcher runs ONCE over all frames (``_match_dets``: one ragged frame batch against the resident
        database; needs the database cache), False = frame by frame as in ``solve_pose_device``; the outputs are the same bit for
        bit.  Default (None): batched whenever the database cache exists -- from 4 frames on the batch is 1.2x to 2.9x the loop's
        matcher throughput."""
        from . import pnp
        frames = [images[i:i + 1] for i in range(images.shape[0])] if isinstance(images, torch.Tensor) else list(images)
        if not frames:
            raise ValueError("solve_poses_device needs at least one image")
        if batched_matcher is None:
            batched_matcher = self.db_cache is not None
        dets = [self.extractor(image) for image in frames]
        matches = [m for m, _ in (self._match_dets(dets) if batched_matcher else [self._single(det) for det in dets])]
        counts = [d["keypoints"][0].shape[0] for d in dets]
        dev = dets[0]["keypoints"][0].device
        cap1 = max(max(counts), 1)
        kpts = torch.zeros(len(frames), cap1, 2, device=dev, dtype=torch.float32)
        m0 = torch.full((len(frames), cap1), -1, device=dev, dtype=torch.int64)
        for i, (det, m, n1) in enumerate(zip(dets, matches, counts)):
            kpts[i, :n1] = det["keypoints"][0]
            m0[i, :n1] = m
        poses, masks, infos = pnp.ransac_pnp_from_matches_batch(K_crops, kpts, self.db["keypoints3d"][0], m0, counts=counts, scale=scale,
                                                                seeds=seeds)
        return poses, masks, infos, dets

    @torch.no_grad()
    def solve_pose(self, image, K_crop, scale=1000, seed=0):
        """image -> (pose_pred [3,4], pose_pred_homo [4,4], inliers [m,1]) like inference.py:140-155; numpy outputs, identity
        when fewer than 5 matches survive or the solve fails (eval_utils.py:40-42)."""
        from . import pnp
        out = self(image)
        return pnp.ransac_PnP(K_crop, out["mkpts2d"], out["mkpts3d"], scale=scale, seed=seed)
