"""Training batches from a built object database (reference: src/sfm/postprocess/feature_process.py:197-294,
src/datasets/GATs_spg_dataset.py:53-162, src/utils/data_utils.py:60-205).

``TrainingSet`` keeps what an ``ObjectMapper`` build leaves on the GPU -- the per-image SuperPoint features, the grouped observation
lists, the collected and mean descriptors, the merged points -- and the per-image ground-truth pairs that ``gts_assign_pairs`` makes
of them.  ``batch(image_ids, epoch)`` is one ``gts_build_batch`` (include/gatsspg_trainset.h): leaf selection, leaf gather, query and
database padding as one chain of HIP launches with no host read-back, giving ``(data, SparseTarget)`` for ``training_loss``.

    mapper = ObjectMapper(...); mapper.build_from_matches(features, ...)
    ts = mapper.training_set(features)
    data, target = ts.batch(ts.image_ids[:8], epoch=0)
    training_loss(model, data, target, MatchingLoss()).backward()

Every random choice (which leaves, where the pads lie) is a hash of (seed, epoch, image): a sample does not depend on its slot in
the batch, and a new epoch draws new leaves.  The stated differences from the reference are listed in the header.

The reference's on-disk form of the same data -- ``anno_2d.json`` and one JSON file per image -- is written by
``write_training_annotations`` and read by ``from_reference_files`` (``json`` only; the host halves ``write_annotation_json`` and
``read_annotation_json`` work on numpy arrays).  There is no CPU fallback: the device side runs on a ROCm GPU only.
"""
from __future__ import annotations

import json
import os
import os.path as osp

import numpy as np
import torch

from . import _native_trainset, database_io
from ._binding import NativeError
from .training import SparseTarget

_NO_CPU = ("onepose_amd.TrainingSet runs only on a ROCm GPU ({} is on {}); there is no CPU fallback -- move the tensors to the GPU")
DATA_KEYS = ("keypoints2d", "descriptors2d_query", "keypoints3d", "descriptors3d_db", "descriptors2d_db", "image_size")
ANNO_3D_FILES = ("anno_3d_average.npz", "anno_3d_collect.npz", "idxs.npy")


# ---- the host side: the reference's files ----
def pairs_from_observations(point_offsets, obs_image, obs_kpt, n_kpts):
    """The rule of ``gts_assign_pairs`` in numpy: per image a [2, k] int64 array (keypoint, point), ascending keypoint; the pair of
    point p in image v is its lowest keypoint there, an out-of-range observation is ignored, the lower point wins a keypoint."""
    V = len(n_kpts)
    owner = [dict() for _ in range(V)]
    for p in range(len(point_offsets) - 1):
        best = {}
        for j in range(point_offsets[p], point_offsets[p + 1]):
            v, q = int(obs_image[j]), int(obs_kpt[j])
            if 0 <= v < V and 0 <= q < n_kpts[v]:
                best[v] = min(best.get(v, q), q)
        for v, q in best.items():
            owner[v][q] = min(owner[v].get(q, p), p)
    return [np.array(sorted(o.items()), np.int64).reshape(-1, 2).T for o in owner]


def write_annotation_json(out_dir, features, pairs, image_names=None, pose_files=None):
    """``<out_dir>/anno_2d/<v>.json`` per image with at least one pair (keys and shapes of save_2d_anno_for_each_image:
    keypoints2d [n,2], descriptors2d [dim,n], scores2d [n,1], assign_matrix [2,k], num_matches) and the list ``<out_dir>/anno_2d.json``
    (anno_id from 1, anno_file, img_file, pose_file); images without a pair are left out (feature_process.py:283).  -> the list's path."""
    anno_dir = osp.join(out_dir, "anno_2d")
    os.makedirs(anno_dir, exist_ok=True)
    records = []
    for v, (f, a) in enumerate(zip(features, pairs)):
        a = np.asarray(a).reshape(2, -1)
        if a.shape[1] == 0:
            continue
        path = osp.join(anno_dir, f"{v}.json")
        with open(path, "w") as fh:
            json.dump({"keypoints2d": np.asarray(f["keypoints"]).tolist(), "descriptors2d": np.asarray(f["descriptors"]).tolist(),
                       "scores2d": np.asarray(f["scores"]).reshape(-1, 1).tolist(), "assign_matrix": a.tolist(), "num_matches": int(a.shape[1])}, fh)
        records.append({"anno_id": len(records) + 1, "anno_file": path, "img_file": image_names[v] if image_names else f"{v}.png",
                        "pose_file": pose_files[v] if pose_files else ""})
    list_path = osp.join(out_dir, "anno_2d.json")
    with open(list_path, "w") as fh:
        json.dump(records, fh)
    return list_path


def read_annotation_json(anno_2d_json, anno_dir=None, relocate=None):
    """The list and the per-image files -> (features, pairs, records): per listed image dict(keypoints [n,2], descriptors [dim,n],
    scores [n]) float32 and the assign matrix [2,k] int64 (GATs_spg_dataset.read_anno2d, without the padding).  An ``anno_file`` that
    is not there is looked for by its base name under ``relocate`` (files moved since they were written)."""
    with open(anno_2d_json) as fh:
        records = json.load(fh)
    features, pairs = [], []
    for r in records:
        path = r["anno_file"]
        if not osp.exists(path) and relocate is not None:
            path = osp.join(relocate, osp.basename(path))
        with open(path) as fh:
            d = json.load(fh)
        features.append({"keypoints": np.asarray(d["keypoints2d"], np.float32).reshape(-1, 2),
                         "descriptors": np.asarray(d["descriptors2d"], np.float32).reshape(len(d["descriptors2d"]), -1),
                         "scores": np.asarray(d["scores2d"], np.float32).reshape(-1)})
        pairs.append(np.asarray(d["assign_matrix"], np.float32).astype(np.int64).reshape(2, -1))   # torch.Tensor(...).long() in the reference
    return features, pairs, records


def read_annotation_3d(anno_dir):
    """anno_3d_average.npz, anno_3d_collect.npz, idxs.npy -> dict(points3d [N,3], mean_desc [256,N], collect [K,256], idxs [N]) float32,
    as GATs_spg_dataset.read_anno3d converts them (torch.Tensor of the float64 arrays)."""
    avg, clt, idxs = database_io.read_annotation_arrays(*(osp.join(anno_dir, f) for f in ANNO_3D_FILES))
    collect = np.ascontiguousarray(np.asarray(clt["descriptors3d"], np.float32).T)
    return {"points3d": np.asarray(clt["keypoints3d"], np.float32), "mean_desc": np.asarray(avg["descriptors3d"], np.float32), "collect": collect,
            "idxs": idxs}


# ---- the device side ----
def _device_tensor(a, dtype, name, device):
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise RuntimeError(_NO_CPU.format(name, a.device))
        return a.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(device=device, dtype=dtype).contiguous()


class TrainingSet:
    """One object's training data, resident on one GPU.  ``len(ts)`` and ``ts.image_ids``: the images with at least one pair (the
    entries of the reference's anno_2d.json); ``ts.pairs(v)``: the [2, k_v] int32 device tensor (keypoint, point) of image v;
    ``ts.ignored``: observations outside their image, counted by ``gts_assign_pairs``."""

    def __init__(self, device, point_offsets, collect, points3d, mean_desc, features, image_sizes, obs_image=None, obs_kpt=None, pairs=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(_NO_CPU.format("the training set", self.device))
        dev, to = self.device, _device_tensor
        named = dict(point_offsets=point_offsets, collect=collect, points3d=points3d, mean_desc=mean_desc, obs_image=obs_image, obs_kpt=obs_kpt)
        named.update({f"features[{v}][{k!r}]": f[k] for v, f in enumerate(features) for k in ("keypoints", "descriptors", "scores")})
        named.update({f"pairs[{v}]": p for v, p in enumerate(pairs or [])})
        for name, a in named.items():                  # before anything is uploaded
            if isinstance(a, torch.Tensor) and not a.is_cuda:
                raise RuntimeError(_NO_CPU.format(name, a.device))
        self.lib = _native_trainset.load()
        self.point_offsets = to(point_offsets, torch.int32, "point_offsets", dev).reshape(-1)
        self.collect = to(collect, torch.float32, "collect", dev)
        self.points3d = to(points3d, torch.float32, "points3d", dev).reshape(-1, 3)
        self.mean_desc = to(mean_desc, torch.float32, "mean_desc", dev)
        self.N, self.K, self.V = self.points3d.shape[0], self.collect.shape[0], len(features)
        D = _native_trainset.DESC_DIM
        if self.collect.dim() != 2 or self.collect.shape[1] != D or tuple(self.mean_desc.shape) != (D, self.N):
            raise ValueError(f"collect must be [K, {D}] and mean_desc [{D}, N = {self.N}] (got {list(self.collect.shape)}, {list(self.mean_desc.shape)})")
        if self.point_offsets.shape[0] != self.N + 1 or min(self.N, self.K, self.V) < 1:
            raise ValueError(f"point_offsets must be [N + 1] with N, K, V >= 1 (got {self.point_offsets.shape[0]} offsets, N = {self.N}, K = {self.K}, V = {self.V})")
        self.n_kpts = [int(f["keypoints"].shape[0]) for f in features]
        self.kpt_offsets_host = np.concatenate([[0], np.cumsum(self.n_kpts)]).astype(np.int32)
        self.total_kpts = int(self.kpt_offsets_host[-1])
        if self.total_kpts < 1:
            raise ValueError("the images have no keypoints")
        for v, f in enumerate(features):
            if tuple(f["descriptors"].shape) != (D, self.n_kpts[v]):
                raise ValueError(f"image {v}: descriptors must be [{D}, {self.n_kpts[v]}] (got {list(f['descriptors'].shape)})")
        self.kpt_offsets = torch.from_numpy(self.kpt_offsets_host).to(dev)
        self.kpts2d = torch.cat([to(f["keypoints"], torch.float32, "keypoints", dev).reshape(-1, 2) for f in features]).contiguous()
        self.scores2d = torch.cat([to(f["scores"], torch.float32, "scores", dev).reshape(-1) for f in features]).contiguous()
        self.desc2d = torch.cat([to(f["descriptors"], torch.float32, "descriptors", dev).reshape(-1) for f in features]).contiguous()
        sizes = np.asarray(image_sizes, np.int32).reshape(-1, 2)
        if len(sizes) == 1:
            sizes = np.repeat(sizes, self.V, axis=0)
        if len(sizes) != self.V:
            raise ValueError(f"{self.V} images but {len(sizes)} image sizes")
        self.image_hw_host = np.ascontiguousarray(sizes)
        self.image_hw = torch.from_numpy(self.image_hw_host).to(dev)
        if pairs is None:
            self._assign(to(obs_image, torch.int32, "obs_image", dev).reshape(-1), to(obs_kpt, torch.int32, "obs_kpt", dev).reshape(-1))
        else:
            if len(pairs) != self.V:
                raise ValueError(f"{self.V} images but {len(pairs)} pair lists")
            lists = [to(p, torch.int32, "pairs", dev).reshape(2, -1) for p in pairs]
            self.pair_counts = [int(p.shape[1]) for p in lists]
            self._pairs = lists
            self.ignored = torch.zeros(1, dtype=torch.int32, device=dev)
        self.image_ids = [v for v in range(self.V) if self.pair_counts[v] > 0]

    def _assign(self, obs_image, obs_kpt):
        """``gts_assign_pairs`` once; the per-image counts are read back here, at construction, and never again"""
        dev = self.device
        if obs_image.shape[0] != self.K or obs_kpt.shape[0] != self.K:
            raise ValueError(f"obs_image and obs_kpt must have K = {self.K} entries")
        nbytes = self._workspace_bytes(self.total_kpts, 0, 0, 0)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        offsets = torch.empty(self.V + 1, dtype=torch.int32, device=dev)
        kpt, point = torch.empty(self.K, dtype=torch.int32, device=dev), torch.empty(self.K, dtype=torch.int32, device=dev)
        self.ignored = torch.empty(1, dtype=torch.int32, device=dev)
        self.lib.call("gts_assign_pairs", dev, self.point_offsets, obs_image, obs_kpt, self.N, self.K, self.kpt_offsets, self.V, self.total_kpts,
                      offsets, kpt, point, self.ignored, ws, nbytes)
        host = offsets.cpu().numpy()
        both = torch.stack([kpt, point])                                # [2, K]: the per-image lists are views of it
        self.pair_counts = np.diff(host).astype(int).tolist()
        self._pairs = [both[:, host[v]:host[v + 1]] for v in range(self.V)]

    def _workspace_bytes(self, *shape):
        nbytes = self.lib.gts_workspace_bytes(*shape)
        if nbytes == 0:
            raise NativeError("gts_workspace_bytes: " + self.lib.gts_last_error().decode())
        return nbytes

    # ---- constructors ----
    @classmethod
    def from_arrays(cls, point_offsets, collect, points3d, mean_desc, features, obs_image=None, obs_kpt=None, pairs=None, image_size=None,
                    device="cuda"):
        """point_offsets [N+1], obs_image / obs_kpt [K] as ``mapping.point_observations`` returns them (or ``pairs``: per image a [2, k]
        list, in their place); collect [K,256]; points3d [N,3]; mean_desc [256,N]; features: per image dict(keypoints [n,2], descriptors
        [256,n], scores [n] and, without ``image_size``, size (H, W)).  Arrays are uploaded; tensors must be on a GPU."""
        if (pairs is None) == (obs_image is None or obs_kpt is None):
            raise ValueError("give either obs_image and obs_kpt or pairs")
        sizes = [image_size] if image_size is not None else [tuple(int(s) for s in f["size"]) for f in features]
        return cls(device, point_offsets, collect, points3d, mean_desc, features, sizes, obs_image, obs_kpt, pairs)

    @classmethod
    def from_mapper(cls, mapper, features, image_size=None):
        """From the latest build of an ``ObjectMapper``: its grouped observations, collected and mean descriptors and merged points, which
        the build left on the GPU, and the features the build was given."""
        res = getattr(mapper, "_resident", None)
        if res is None:
            raise RuntimeError("TrainingSet.from_mapper: the mapper has not built a database yet")
        return cls.from_arrays(res["point_offsets"], res["collect"], res["points3d"], res["mean_desc"].t().to(torch.float32), features,
                               obs_image=res["obs_image"], obs_kpt=res["obs_kpt"], image_size=image_size, device=mapper.device)

    @classmethod
    def from_reference_files(cls, anno_2d_json, anno_dir, image_size=(512, 512), device="cuda", relocate=None):
        """From the reference's files: the ``anno_2d.json`` list with its per-image JSON files, and ``anno_dir`` holding
        anno_3d_average.npz, anno_3d_collect.npz and idxs.npy.  ``image_size`` (H, W) is an argument because the reference reads it
        from the image file.  The images are the list's entries, in its order."""
        features, pairs, _ = read_annotation_json(anno_2d_json, relocate=relocate)
        a = read_annotation_3d(anno_dir)
        offsets = np.concatenate([[0], np.cumsum(a["idxs"])]).astype(np.int32)
        return cls.from_arrays(offsets, a["collect"], a["points3d"], a["mean_desc"], features, pairs=pairs, image_size=image_size, device=device)

    # ---- the resident pairs ----
    def __len__(self):
        return len(self.image_ids)

    def pairs(self, v):
        return self._pairs[v]

    def features(self):
        """the per-image features as host arrays (the form ``write_annotation_json`` takes)"""
        kp, sc, de = self.kpts2d.cpu().numpy(), self.scores2d.cpu().numpy(), self.desc2d.cpu().numpy()
        o, D = self.kpt_offsets_host, _native_trainset.DESC_DIM
        return [{"keypoints": kp[o[v]:o[v + 1]], "scores": sc[o[v]:o[v + 1]], "descriptors": de[D * o[v]:D * o[v + 1]].reshape(D, -1)}
                for v in range(self.V)]

    def write_training_annotations(self, out_dir, image_names=None, pose_files=None):
        """The reference's per-image JSON files and the ``anno_2d.json`` list under ``out_dir`` -> the list's path."""
        return write_annotation_json(out_dir, self.features(), [p.cpu().numpy().astype(np.int64) for p in self._pairs], image_names, pose_files)

    # ---- batches ----
    def _fill(self, out, rows, image_ids, epochs, shape2d, shape3d, num_leaf, seed):
        """one ``gts_build_batch`` into the rows ``rows`` (a slice) of the shared tensors ``out``"""
        dev, b = self.device, len(image_ids)
        for v in image_ids:
            if not 0 <= int(v) < self.V:
                raise ValueError(f"image {v} is outside [0, {self.V})")
        sample_image = torch.tensor([int(v) for v in image_ids], dtype=torch.int32).to(dev)
        sample_epoch = torch.tensor([int(e) for e in epochs], dtype=torch.int32).to(dev)
        nbytes = self._workspace_bytes(0, b, shape3d, num_leaf)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.lib.call("gts_build_batch", dev, self.point_offsets, self.collect, self.points3d, self.mean_desc, self.N, self.K, self.desc2d,
                      self.kpts2d, self.scores2d, self.kpt_offsets, self.image_hw, self.V, sample_image, sample_epoch, b, shape2d, shape3d,
                      num_leaf, int(seed) & (2 ** 64 - 1), out["descriptors2d_query"][rows], out["keypoints2d"][rows], None,
                      out["keypoints3d"][rows], out["descriptors3d_db"][rows], out["descriptors2d_db"][rows], ws, nbytes)
        out["image_size"][rows] = torch.from_numpy(self.image_hw_host[[int(v) for v in image_ids]].astype(np.float32)).to(dev)

    def batch(self, image_ids, epoch, shape2d=1000, shape3d=2000, num_leaf=8, pad_val=0, seed=0):
        """``(data, SparseTarget)`` of the images ``image_ids`` for ``epoch`` (an int, or one per image): ``data`` has the keys of
        GATsSPGDataset.read_anno's train split, batched; the target holds views of the resident pair lists and the host-side counts
        kept at construction.  One chain of launches, no host read-back."""
        return TrainingSet.batch_of([(self, image_ids)], epoch, shape2d, shape3d, num_leaf, pad_val, seed)

    @staticmethod
    def batch_of(parts, epoch, shape2d=1000, shape3d=2000, num_leaf=8, pad_val=0, seed=0):
        """A batch across objects: ``parts`` is [(training set, image_ids), ...]; one ``gts_build_batch`` per object into its row slice of
        shared tensors.  ``epoch``: an int, or one per sample in batch order."""
        parts = [(ts, list(ids)) for ts, ids in parts]
        b = sum(len(ids) for _, ids in parts)
        if b < 1 or any(not ids for _, ids in parts):
            raise ValueError("every part of a batch needs at least one image")
        if b > _native_trainset.MAX_BATCH:
            raise ValueError(f"a batch holds at most {_native_trainset.MAX_BATCH} samples (got {b})")
        if not 1 <= int(num_leaf) <= _native_trainset.MAX_LEAF:
            raise ValueError(f"num_leaf must be in [1, {_native_trainset.MAX_LEAF}] (got {num_leaf})")
        if min(int(shape2d), int(shape3d)) < 1 or max(int(shape2d), int(shape3d)) > _native_trainset.MAX_POINTS:
            raise ValueError(f"shape2d and shape3d must be in [1, {_native_trainset.MAX_POINTS}] (got {shape2d}, {shape3d})")
        shape2d, shape3d, num_leaf = int(shape2d), int(shape3d), int(num_leaf)
        epochs = [int(epoch)] * b if isinstance(epoch, (int, np.integer)) else [int(e) for e in epoch]
        if len(epochs) != b:
            raise ValueError(f"{b} samples but {len(epochs)} epochs")
        dev, D = parts[0][0].device, _native_trainset.DESC_DIM
        if any(ts.device != dev for ts, _ in parts):
            raise RuntimeError("the training sets of one batch must be on one device")
        empty = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        out = {"keypoints2d": empty(b, shape2d, 2), "descriptors2d_query": empty(b, D, shape2d), "keypoints3d": empty(b, shape3d, 3),
               "descriptors3d_db": empty(b, D, shape3d), "descriptors2d_db": empty(b, D, shape3d * num_leaf), "image_size": empty(b, 2)}
        pairs, n_orig, m_orig, row = [], [], [], 0
        for ts, ids in parts:
            ts._fill(out, slice(row, row + len(ids)), ids, epochs[row:row + len(ids)], shape2d, shape3d, num_leaf, seed)
            row += len(ids)
            pairs += [ts._pairs[int(v)] for v in ids]
            n_orig += [min(ts.n_kpts[int(v)], shape2d) for v in ids]
            m_orig += [min(ts.N, shape3d)] * len(ids)
        return out, SparseTarget(pairs, n_orig, m_orig, pad_val)
