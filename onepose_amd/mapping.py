"""The object database builder: what OnePose's ``run.py +preprocess=sfm_spp_spg_*`` (run.py:80-163) produces for one scanned
object -- ``anno/anno_3d_average.npz``, ``anno_3d_collect.npz`` and ``idxs.npy``, the 3D feature database that
``load_object_database``, ``FrameMatcher`` and ``inference_runner`` consume.

    python -m onepose_amd.mapping --data-dir data --object 0408-colorbox-box [--sequences colorbox-1 ...]

Chain: SuperPoint on every posed frame (max_keypoints 4096, extract_features.py:19-26) -> covisible pairs from the poses
(``covis_pairs``, pairs_from_poses.py:6-70) -> SuperGlue on the pairs (match threshold 0.7, match_features.py:14; unordered pairs
matched once, :51-53) -> the HIP tail of libmap_hip.so (include/mapping/mapping.h): geometric verification with the known poses,
triangulation of the tracks with every camera fixed, the track-length / 3D-box / 1 mm merge filters, descriptor collection and
averaging.  Only the track building sits on the host between the kernels (``build_tracks``): one pass of connected components
over the verified matches, whose semantics are ordering, not arithmetic.

The reference hands verification and triangulation to COLMAP, an external binary.  Parity with COLMAP is NOT claimed and has
not been measured: see DESIGN.md section 15 for the list of known differences.  The per-image training annotations
(``anno_2d.json``, feature_process.py:233-294) come from ``ObjectMapper.training_set`` (onepose_amd/trainset.py).
"""
from __future__ import annotations

import argparse
import ctypes
import glob
import os
import os.path as osp
import sys

import numpy as np
import torch

from . import _native_map, _native_sg
from ._binding import NativeError
from .nearest_neighbour import NearestNeighbour
from .superglue import SuperGlue

THRESHOLDS = dict(max_epipolar_error=4.0, min_pair_inliers=15, max_reproj_error=4.0, min_tri_angle=1.5, max_hypotheses=120,
                  refine_iterations=10, max_num_kp3d=2500, dist_threshold=1e-3, seed=0)
SPP_CONF = {"descriptor_dim": 256, "nms_radius": 3, "max_keypoints": 4096}     # src/sfm/extract_features.py:19-26
SG_MATCH_THRESHOLD = 0.7                                                       # src/sfm/match_features.py:14
DOWN_RATIO = 5                                                                 # configs: sfm.down_ratio
COVIS_NUM = 10                                                                 # configs: sfm.covis_num


def covis_pairs(poses, seq_ids=None, num_matched=COVIS_NUM, max_rotation=50):
    """pairs_from_poses.py:6-70 in numpy, as written.  poses [n,3|4,4] world->camera; seq_ids [n]: the sequence every frame
    comes from (None: one sequence) -> list of (i, j).

    Per frame and per sequence, candidates are the frames whose viewing direction differs by more than 10 degrees (the
    reference's ``min_rotation``); ``num_matched // n_sequences`` of them are taken as every second entry of an
    ``argpartition`` of twice that many by camera distance.  ``argpartition`` does not order inside the partition, so which
    of the 2n nearest are taken -- and what happens on ties -- is numpy's choice here exactly as in the reference.
    ``max_rotation`` is accepted and never applied, as in the reference."""
    from scipy.spatial import distance
    poses = np.asarray(poses, np.float64)
    n = len(poses)
    seq_ids = [0] * n if seq_ids is None else list(seq_ids)
    seqs = {}
    for i, s in enumerate(seq_ids):
        seqs.setdefault(s, []).append(i)
    Rs = poses[:, :3, :3].transpose(0, 2, 1)
    ts = -(Rs @ poses[:, :3, 3:])[:, :, 0]
    dist = distance.squareform(distance.pdist(ts))
    trace = np.einsum("nji,mji->mn", Rs, Rs, optimize=True)
    dR = np.rad2deg(np.abs(np.arccos(np.clip((trace - 1) / 2, -1.0, 1.0))))
    valid = dR > 10
    np.fill_diagonal(valid, False)
    dist = np.where(valid, dist, np.inf)
    pairs = []
    per_seq = num_matched // len(seqs)
    for i in range(n):
        dist_i = dist[i]
        for s in seqs:
            ids = np.array(seqs[s])
            try:
                idx = np.argpartition(dist_i[ids], per_seq * 2)[:per_seq:2]
            except ValueError:
                idx = np.argpartition(dist_i[ids], dist_i.shape[0] - 1)
            idx = ids[idx]
            idx = idx[np.argsort(dist_i[idx])]
            idx = idx[valid[i][idx]]
            pairs.extend((i, int(j)) for j in idx)
    return pairs


def unique_pairs(pairs):
    """match_features.py:51-53: an unordered pair is matched once, in the orientation it first occurs in."""
    seen, out = set(), []
    for i, j in pairs:
        if (i, j) in seen or (j, i) in seen:
            continue
        seen.add((i, j))
        out.append((i, j))
    return out


def build_tracks(n_kpts, pair_images, survivors, max_track_length=_native_map.MAX_TRACK_LENGTH):
    """Feature tracks from the verified matches.  Nodes are (image, keypoint), edges the verified matches; a track is a
    connected component (scipy.sparse.csgraph.connected_components).  Tracks are ordered by their smallest node (image-major),
    observations by image; where an image occurs more than once in a component its lowest keypoint index is kept (a rule
    of this project, not COLMAP's); a track longer than ``max_track_length`` keeps its first observations.
    survivors: per pair an [n,2] array of (keypoint of i, keypoint of j) -> (track_offsets [T+1], obs_image [M], obs_kpt [M])
    int32."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    offs = np.concatenate([[0], np.cumsum(np.asarray(n_kpts, np.int64))])
    src = [offs[i] + np.asarray(s, np.int64)[:, 0] for (i, j), s in zip(pair_images, survivors) if len(s)]
    dst = [offs[j] + np.asarray(s, np.int64)[:, 1] for (i, j), s in zip(pair_images, survivors) if len(s)]
    empty = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    if not src:
        return empty
    src, dst = np.concatenate(src), np.concatenate(dst)
    total = int(offs[-1])
    _, labels = connected_components(coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(total, total)), directed=False)
    nodes = np.unique(np.concatenate([src, dst]))               # ascending: image-major, keypoint-minor
    lab = labels[nodes]
    first = np.full(labels.max() + 1, total, np.int64)
    np.minimum.at(first, lab, nodes)
    order = np.lexsort((nodes, first[lab]))
    nodes, key = nodes[order], first[lab][order]
    image = np.searchsorted(offs, nodes, side="right") - 1
    keep = np.ones(len(nodes), bool)
    keep[1:] = (key[1:] != key[:-1]) | (image[1:] != image[:-1])         # the lowest keypoint of an image in a track
    nodes, key, image = nodes[keep], key[keep], image[keep]
    start = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
    rank = np.arange(len(nodes)) - np.repeat(start, np.diff(np.concatenate([start, [len(nodes)]])))
    keep = rank < max_track_length
    nodes, key, image = nodes[keep], key[keep], image[keep]
    start = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
    track_offsets = np.concatenate([start, [len(nodes)]]).astype(np.int32)
    return track_offsets, image.astype(np.int32), (nodes - offs[image]).astype(np.int32)


def make_cams(Ks, poses):
    """[V,16] float64: world->camera [R | t] row-major, then fx, fy, cx, cy (the layout of include/mapping/mapping.h)."""
    Ks, poses = np.asarray(Ks, np.float64), np.asarray(poses, np.float64)
    if Ks.ndim == 2:
        Ks = np.broadcast_to(Ks, (len(poses), 3, 3))
    return np.ascontiguousarray(np.concatenate([poses[:, :3, :4].reshape(-1, 12), Ks[:, 0, 0:1], Ks[:, 1, 1:2], Ks[:, 0, 2:3], Ks[:, 1, 2:3]],
                                               axis=1))


class MapTail:
    """The six entry points of libmap_hip.so, one call each, on torch tensors of one device.  No fallback: a missing
    library raises."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.lib = _native_map.load()

    def tensor(self, a, dtype):
        """``a`` (a tensor or anything array-like: the builder takes numpy) uploaded or moved to this tail's device as a
        contiguous ``dtype`` tensor."""
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        return a.to(device=self.device, dtype=dtype).contiguous()

    def verify(self, kpts, kpt_offsets, cams, pair_images, match_offsets, matches0, max_epipolar_error=4.0, min_pair_inliers=15):
        """-> (out_matches [sum, 2] int32, counts [P] int32) on the device."""
        kpts, cams = self.tensor(kpts, torch.float32), self.tensor(cams, torch.float64)
        kpt_offsets, pair_images = self.tensor(kpt_offsets, torch.int32), self.tensor(pair_images, torch.int32)
        match_offsets, matches0 = self.tensor(match_offsets, torch.int32), self.tensor(matches0, torch.int64)
        P, V = pair_images.shape[0], cams.shape[0]
        out = torch.full((max(1, matches0.shape[0]), 2), -1, device=self.device, dtype=torch.int32)
        counts = torch.zeros(P, device=self.device, dtype=torch.int32)
        _native_map.call("map_verify_matches", self.device, kpts, kpt_offsets, cams, V, pair_images, match_offsets, matches0, P,
                         float(max_epipolar_error), int(min_pair_inliers), out, counts)
        return out, counts

    def triangulate(self, track_offsets, obs_image, obs_xy, cams, max_track_length, max_reproj_error=4.0, min_tri_angle=1.5,
                    max_hypotheses=120, refine_iterations=10, seed=0):
        """-> (xyz [T,3] float64, inlier_mask [M] int32, info [T,4] int32, lengths [T] int32) on the device."""
        track_offsets, obs_image = self.tensor(track_offsets, torch.int32), self.tensor(obs_image, torch.int32)
        obs_xy, cams = self.tensor(obs_xy, torch.float32), self.tensor(cams, torch.float64)
        T, M = track_offsets.shape[0] - 1, obs_image.shape[0]
        xyz = torch.full((T, 3), float("nan"), device=self.device, dtype=torch.float64)
        mask = torch.full((max(1, M),), -1, device=self.device, dtype=torch.int32)
        info = torch.full((T, 4), -9, device=self.device, dtype=torch.int32)
        lengths = torch.full((T,), -1, device=self.device, dtype=torch.int32)
        _native_map.call("map_triangulate_tracks", self.device, track_offsets, obs_image, obs_xy, cams, T, cams.shape[0],
                         int(max_track_length), float(max_reproj_error), float(min_tri_angle), int(max_hypotheses),
                         int(refine_iterations), int(seed), xyz, mask, info, lengths)
        return xyz, mask[:M], info, lengths

    def track_length_threshold(self, lengths, max_num_kp3d):
        lengths = self.tensor(lengths, torch.int32)
        thr = torch.full((1,), -1, device=self.device, dtype=torch.int32)
        _native_map.call("map_track_length_threshold", self.device, lengths, lengths.shape[0], int(max_num_kp3d), thr)
        return thr

    def filter_points(self, xyz, lengths, threshold, box_corners):
        """-> (kept_ids [n] int32, kept_xyz [n,3] float32) on the device (reads the count: one synchronisation)."""
        xyz, lengths, threshold = self.tensor(xyz, torch.float64), self.tensor(lengths, torch.int32), self.tensor(threshold, torch.int32)
        T = lengths.shape[0]
        ids = torch.full((T,), -1, device=self.device, dtype=torch.int32)
        out = torch.zeros(T, 3, device=self.device, dtype=torch.float32)
        count = torch.zeros(1, device=self.device, dtype=torch.int32)
        box = (ctypes.c_float * 24)(*np.asarray(box_corners, np.float64).astype(np.float32).reshape(24).tolist())
        _native_map.call("map_filter_points", self.device, xyz, lengths, T, threshold, box, ids, out, count)
        n = int(count.item())
        return ids[:n], out[:n]

    def merge_points(self, xyz32, dist_threshold=1e-3):
        """-> (merged [n',3] float32, member_offsets [n'+1] int32, members int32) on the device (one synchronisation)."""
        xyz32 = self.tensor(xyz32, torch.float32)
        n = xyz32.shape[0]
        nbytes = self.lib.map_workspace_bytes(n)
        if nbytes == 0:
            raise NativeError(f"map_workspace_bytes refused {n} points: {self.lib.map_last_error().decode()}")
        ws = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        merged = torch.zeros(n, 3, device=self.device, dtype=torch.float32)
        offs = torch.zeros(n + 1, device=self.device, dtype=torch.int32)
        members = torch.full((n,), -1, device=self.device, dtype=torch.int32)
        count = torch.zeros(1, device=self.device, dtype=torch.int32)
        _native_map.call("map_merge_points", self.device, xyz32, n, float(dist_threshold), merged, offs, members, count, ws, nbytes)
        k = int(count.item())
        offs = offs[:k + 1]
        return merged[:k], offs, members[:int(offs[-1].item())]

    def gather(self, descriptors, scores, point_offsets, obs_image, obs_kpt):
        """descriptors: per image a [dim, n_v] float32 device tensor, scores: per image [n_v] ->
        (collect [K,dim] float32, collect_scores [K] float32, idxs [N] int64, mean [N,dim] float64, mean_scores [N] float64)."""
        descriptors = [self.tensor(d, torch.float32) for d in descriptors]
        scores = [self.tensor(s, torch.float32).reshape(-1) for s in scores]
        dim = descriptors[0].shape[0]
        dtab = torch.tensor([d.data_ptr() for d in descriptors], dtype=torch.int64).to(self.device)
        stab = torch.tensor([s.data_ptr() for s in scores], dtype=torch.int64).to(self.device)
        n_kpts = torch.tensor([d.shape[1] for d in descriptors], dtype=torch.int32).to(self.device)
        point_offsets, obs_image, obs_kpt = (self.tensor(a, torch.int32) for a in (point_offsets, obs_image, obs_kpt))
        N, K = point_offsets.shape[0] - 1, obs_image.shape[0]
        cd = torch.full((max(1, K), dim), float("nan"), device=self.device, dtype=torch.float32)
        cs = torch.full((max(1, K),), float("nan"), device=self.device, dtype=torch.float32)
        idxs = torch.full((N,), -1, device=self.device, dtype=torch.int64)
        md = torch.full((N, dim), float("nan"), device=self.device, dtype=torch.float64)
        ms = torch.full((N,), float("nan"), device=self.device, dtype=torch.float64)
        _native_map.call("map_gather_descriptors", self.device, dtab, stab, n_kpts, len(descriptors), point_offsets, obs_image, obs_kpt,
                         N, dim, cd, cs, idxs, md, ms)
        torch.cuda.synchronize(self.device)      # the pointer tables and the per-image tensors must outlive the kernel
        return cd[:K], cs[:K], idxs, md, ms


def point_observations(track_offsets, obs_image, obs_kpt, inlier_mask, kept_ids, member_offsets, members):
    """The surviving observations grouped by merged point in the reference's traversal order (feature_process.py:95-188):
    merged member after member (ascending old id), image order inside -> (point_offsets [N+1], obs_image [K], obs_kpt [K])."""
    offs, img, kpt = [0], [], []
    for p in range(len(member_offsets) - 1):
        n = 0
        for pos in members[member_offsets[p]:member_offsets[p + 1]]:
            t = kept_ids[pos]
            s, e = track_offsets[t], track_offsets[t + 1]
            sel = np.nonzero(inlier_mask[s:e])[0] + s
            img.append(obs_image[sel])
            kpt.append(obs_kpt[sel])
            n += len(sel)
        offs.append(offs[-1] + n)
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)  # noqa: E731
    return np.array(offs, np.int32), cat(img), cat(kpt)


def annotation_arrays(merged_xyz, collect_desc, collect_scores, idxs, mean_desc, mean_scores):
    """The contents of the three annotation files with the reference's keys, shapes and dtypes (feature_process.py:191-194,
    357-363: everything went through float64 numpy appends; idxs is int64)."""
    kp = np.asarray(merged_xyz, np.float32).astype(np.float64)
    return {"average": dict(keypoints3d=kp, descriptors3d=np.ascontiguousarray(np.asarray(mean_desc, np.float64).T),
                            scores3d=np.asarray(mean_scores, np.float64).reshape(-1, 1)),
            "collect": dict(keypoints3d=kp, descriptors3d=np.ascontiguousarray(np.asarray(collect_desc, np.float32).astype(np.float64).T),
                            scores3d=np.asarray(collect_scores, np.float32).astype(np.float64).reshape(-1, 1)),
            "idxs": np.asarray(idxs, np.int64)}


def write_annotation_files(out_dir, anno):
    """<out_dir>/anno/{anno_3d_average.npz, anno_3d_collect.npz, idxs.npy} -> their paths."""
    anno_dir = osp.join(out_dir, "anno")
    os.makedirs(anno_dir, exist_ok=True)
    paths = (osp.join(anno_dir, "anno_3d_average.npz"), osp.join(anno_dir, "anno_3d_collect.npz"), osp.join(anno_dir, "idxs.npy"))
    np.savez(paths[0], **anno["average"])
    np.savez(paths[1], **anno["collect"])
    np.save(paths[2], anno["idxs"])
    return paths


def database_from_annotation(anno, num_leaf=8, seed=None, device="cuda"):
    """What load_object_database makes of the three files, from the arrays (inference.py:113-130)."""
    from .database_io import build_features3d_leaves, pad_features3d_random
    kp3d = anno["collect"]["keypoints3d"].astype(np.float32)
    n = kp3d.shape[0]
    d3, _ = pad_features3d_random(anno["average"]["descriptors3d"], anno["average"]["scores3d"], n)
    leaves, _ = build_features3d_leaves(anno["collect"]["descriptors3d"], anno["collect"]["scores3d"], anno["idxs"], n, num_leaf, rng=seed)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None].to(device)  # noqa: E731
    return {"keypoints3d": to(kp3d), "descriptors3d_db": to(d3), "descriptors2d_db": to(leaves)}


class ObjectMapper:
    """Builds an object's 3D feature database from a posed scan.

    ``extractor``: a ``SuperPoint`` (max_keypoints 4096 in the reference), ``matcher``: a ``SuperGlue`` (match threshold 0.7);
    both may be None when only ``build_from_features`` / ``build_from_matches`` are used.  ``pair_batch``: image pairs per
    ragged batch of a native matcher (``SuperGlue.match_pairs`` / ``NearestNeighbour.match_pairs``; the matches are bitwise those of one forward per pair);
    1, or any other matcher, runs one forward per pair.  ``thresholds``: any of THRESHOLDS.
    Every entry point returns the dict ``load_object_database`` returns and, with ``out_dir``, writes the three annotation
    files it reads; ``self.last`` keeps the intermediate results of the latest build (numpy)."""

    def __init__(self, extractor=None, matcher=None, num_leaf=8, leaf_seed=None, device="cuda", pair_batch=16, **thresholds):
        unknown = set(thresholds) - set(THRESHOLDS)
        if unknown:
            raise TypeError(f"unknown thresholds {sorted(unknown)}; known: {sorted(THRESHOLDS)}")
        if int(pair_batch) < 1:
            raise ValueError(f"pair_batch must be >= 1 (got {pair_batch})")
        self.extractor, self.matcher, self.pair_batch = extractor, matcher, int(pair_batch)
        self.num_leaf, self.leaf_seed, self.device = num_leaf, leaf_seed, torch.device(device)
        self.cfg = dict(THRESHOLDS, **thresholds)
        self.tail = MapTail(device)
        self.last = None
        self._resident = None           # the device tensors of the latest build that TrainingSet.from_mapper takes

    @torch.no_grad()
    def build(self, frames, poses, Ks, box3d_corners, seq_ids=None, out_dir=None):
        """frames: grey images [1,1,H,W] in [0, 1] (tensors), poses [V,3|4,4] world->camera, Ks [V,3,3] or [3,3]."""
        if self.extractor is None:
            raise RuntimeError("ObjectMapper.build needs an extractor")
        features = []
        for img in frames:
            det = self.extractor(img.to(self.device))
            features.append({"keypoints": det["keypoints"][0].contiguous(), "scores": det["scores"][0].contiguous(),
                             "descriptors": det["descriptors"][0].contiguous(), "size": tuple(img.shape[-2:])})
        pairs = covis_pairs(poses, seq_ids, COVIS_NUM)
        return self.build_from_features(features, pairs, poses, Ks, box3d_corners, out_dir=out_dir)

    @torch.no_grad()
    def build_from_features(self, features, pairs, poses, Ks, box3d_corners, out_dir=None):
        """features: per image dict(keypoints [n,2], scores [n], descriptors [256,n], size (H, W)); pairs: (i, j) image pairs."""
        if self.matcher is None:
            raise RuntimeError("ObjectMapper.build_from_features needs a matcher")
        to = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(self.device)  # noqa: E731

        def pair_data(i, j):
            f0, f1 = features[i], features[j]
            return {"keypoints0": to(f0["keypoints"])[None], "scores0": to(f0["scores"])[None], "descriptors0": to(f0["descriptors"])[None],
                    "keypoints1": to(f1["keypoints"])[None], "scores1": to(f1["scores"])[None], "descriptors1": to(f1["descriptors"])[None],
                    "image0": torch.empty(1, 1, int(f0["size"][0]), int(f0["size"][1]), device="meta"),
                    "image1": torch.empty(1, 1, int(f1["size"][0]), int(f1["size"][1]), device="meta")}

        todo = list(unique_pairs(pairs))
        pair_matches = []
        if isinstance(self.matcher, (SuperGlue, NearestNeighbour)) and self.pair_batch > 1:
            step = min(self.pair_batch, _native_sg.MAX_ITEMS)
            for k in range(0, len(todo), step):      # one batch of pairs in memory at a time
                chunk = todo[k:k + step]
                preds = self.matcher.match_pairs([pair_data(i, j) for i, j in chunk], max_items=step)
                pair_matches += [(i, j, pred["matches0"][0].to(torch.int64).clone()) for (i, j), pred in zip(chunk, preds)]
        else:
            for i, j in todo:
                pair_matches.append((i, j, self.matcher(pair_data(i, j))["matches0"][0].to(torch.int64)))
        return self.build_from_matches(features, pair_matches, poses, Ks, box3d_corners, out_dir=out_dir)

    @torch.no_grad()
    def build_from_matches(self, features, pair_matches, poses, Ks, box3d_corners, out_dir=None):
        """pair_matches: (i, j, matches0 [n_i] int64: index into the keypoints of j or -1) per image pair."""
        cfg, tail, dev = self.cfg, self.tail, self.device
        host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
        V = len(features)
        n_kpts = [int(f["keypoints"].shape[0]) for f in features]
        kpt_offsets = np.concatenate([[0], np.cumsum(n_kpts)]).astype(np.int32)
        kpts = torch.cat([tail.tensor(f["keypoints"], torch.float32).reshape(-1, 2) for f in features])
        cams = make_cams(Ks, poses)
        if len(cams) != V:
            raise ValueError(f"{V} images but {len(cams)} poses")
        if not pair_matches:
            raise ValueError("no image pairs")
        pair_images = np.array([(i, j) for i, j, _ in pair_matches], np.int32)
        m0 = [tail.tensor(m, torch.int64).reshape(-1) for _, _, m in pair_matches]
        for (i, j, _), m in zip(pair_matches, m0):
            if m.shape[0] != n_kpts[i]:
                raise ValueError(f"pair ({i}, {j}): matches0 has {m.shape[0]} entries, image {i} has {n_kpts[i]} keypoints")
        match_offsets = np.concatenate([[0], np.cumsum([m.shape[0] for m in m0])]).astype(np.int32)
        out, counts = tail.verify(kpts, kpt_offsets, cams, pair_images, match_offsets, torch.cat(m0), cfg["max_epipolar_error"],
                                  cfg["min_pair_inliers"])
        out, counts = host(out), host(counts)
        survivors = [out[match_offsets[p]:match_offsets[p] + counts[p]] for p in range(len(pair_matches))]
        track_offsets, obs_image, obs_kpt = build_tracks(n_kpts, pair_images, survivors)
        T = len(track_offsets) - 1
        if T == 0:
            raise RuntimeError("no feature track survived the geometric verification")
        obs_xy = kpts[torch.from_numpy(kpt_offsets[obs_image].astype(np.int64) + obs_kpt).to(dev)]
        xyz, mask, info, lengths = tail.triangulate(track_offsets, obs_image, obs_xy, cams, int(np.diff(track_offsets).max()),
                                                    cfg["max_reproj_error"], cfg["min_tri_angle"], cfg["max_hypotheses"],
                                                    cfg["refine_iterations"], cfg["seed"])
        threshold = tail.track_length_threshold(lengths, cfg["max_num_kp3d"])
        kept_ids, kept_xyz = tail.filter_points(xyz, lengths, threshold, box3d_corners)
        if kept_ids.shape[0] == 0:
            raise RuntimeError("no 3D point survived the track-length and box filters")
        merged, member_offsets, members = tail.merge_points(kept_xyz, cfg["dist_threshold"])
        mask_h, kept_h, moffs_h, members_h = host(mask), host(kept_ids), host(member_offsets), host(members)
        point_offsets, g_img, g_kpt = point_observations(track_offsets, obs_image, obs_kpt, mask_h, kept_h, moffs_h, members_h)
        cd, cs, idxs, md, ms = tail.gather([f["descriptors"] for f in features], [f["scores"] for f in features], point_offsets, g_img, g_kpt)
        anno = annotation_arrays(host(merged), host(cd), host(cs), host(idxs), host(md), host(ms))
        self.last = dict(survivors=survivors, counts=counts, track_offsets=track_offsets, obs_image=obs_image, obs_kpt=obs_kpt,
                         xyz=host(xyz), inlier_mask=mask_h, info=host(info), lengths=host(lengths), threshold=int(threshold.item()),
                         kept_ids=kept_h, kept_xyz=host(kept_xyz), merged_xyz=host(merged), member_offsets=moffs_h, members=members_h,
                         point_offsets=point_offsets, gather_image=g_img, gather_kpt=g_kpt, anno=anno)
        self._resident = dict(point_offsets=point_offsets, obs_image=g_img, obs_kpt=g_kpt, collect=cd, mean_desc=md, points3d=merged)
        if out_dir is not None:
            self.last["paths"] = write_annotation_files(out_dir, anno)
        return database_from_annotation(anno, self.num_leaf, self.leaf_seed, dev)

    def training_set(self, features, image_size=None):
        """The ``TrainingSet`` of the latest build (onepose_amd/trainset.py): ``features`` as the build took them, with their ``size``
        (H, W) or one ``image_size`` for all."""
        from .trainset import TrainingSet
        return TrainingSet.from_mapper(self, features, image_size)


def scan_lists(data_dir, obj, sequences=None, down_ratio=DOWN_RATIO):
    """run.py:86-101: the colour frames of the object's sequences whose index is a multiple of ``down_ratio``.  The reference
    takes them in glob's order, which is the file system's; here they are sorted by frame index, so that image ids, pairs and
    the written database do not depend on the directory listing."""
    root = osp.join(data_dir, obj)
    seqs = sequences or sorted(d for d in (os.listdir(root) if osp.isdir(root) else []) if osp.isdir(osp.join(root, d, "color")))
    imgs, seq_ids = [], []
    for s in seqs:
        for f in sorted(glob.glob(osp.join(root, s, "color", "*.png")), key=lambda q: int(osp.basename(q).split(".")[0])):
            if int(osp.basename(f).split(".")[0]) % down_ratio == 0:
                imgs.append(f)
                seq_ids.append(s)
    return root, imgs, seq_ids


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-dir", default="data/onepose_datasets/train_data")
    ap.add_argument("--object", required=True, help="object directory under --data-dir (holds box3d_corners.txt and the sequences)")
    ap.add_argument("--sequences", nargs="*", default=None, help="sequence directories of the object (default: all with color/)")
    ap.add_argument("--models-dir", default="data/models")
    ap.add_argument("--out-dir", default=None, help="default: data/sfm_model/<object>/outputs_superpoint_superglue")
    a = ap.parse_args(argv)
    root, imgs, seq_ids = scan_lists(a.data_dir, a.object, a.sequences)
    spp = osp.join(a.models_dir, "extractors", "SuperPoint", "superpoint_v1.pth")
    spg = osp.join(a.models_dir, "matchers", "SuperGlue", "superglue_outdoor.pth")
    box = osp.join(root, "box3d_corners.txt")
    missing = [q for q in (spp, spg, box) if not osp.exists(q)] + ([] if imgs else [osp.join(root, "<sequence>", "color", "*.png")])
    if missing:
        print("onepose_amd.mapping: nothing to build -- not found:\n  " + "\n  ".join(missing) +
              "\n(the OnePose scans and checkpoints are not shipped with this repository; place them as in the reference's README "
              "and re-run: the object's anno/ directory is written)")
        return 0
    if not torch.cuda.is_available():
        print("onepose_amd.mapping needs a ROCm GPU (the HIP path has no CPU fallback)", file=sys.stderr)
        return 2
    from . import SuperGlue, SuperPoint
    from .inference_runner import read_image
    extractor = SuperPoint(dict(SPP_CONF)).eval()
    sd = torch.load(spp, map_location="cpu")
    extractor.load_state_dict(sd.get("net", sd.get("state_dict", sd)) if isinstance(sd, dict) else sd, strict=True)
    matcher = SuperGlue({"match_threshold": SG_MATCH_THRESHOLD}).eval()
    matcher.load_state_dict(torch.load(spg, map_location="cpu"), strict=True)
    poses = np.stack([np.loadtxt(f.replace("/color/", "/poses_ba/").replace(".png", ".txt")) for f in imgs])      # path_utils.py:22-26
    Ks = np.stack([np.loadtxt(f.replace("/color/", "/intrin_ba/").replace(".png", ".txt")) for f in imgs])        # path_utils.py:39-43
    out_dir = a.out_dir or osp.join("data", "sfm_model", a.object, "outputs_superpoint_superglue")
    mapper = ObjectMapper(extractor.to("cuda"), matcher.to("cuda"))
    db = mapper.build((read_image(f) for f in imgs), poses, Ks, np.loadtxt(box), seq_ids=seq_ids, out_dir=out_dir)
    print(f"{a.object}: {len(imgs)} frames -> {db['keypoints3d'].shape[1]} 3D points, written to {osp.join(out_dir, 'anno')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
