"""The cases and call bodies that tests/test_trainset_gpu.py (bitwise against tests/trainset_oracle.py) and
tests/test_placement_trainset.py (guard bands, capture and replay) share: small objects at the edges of the gather tile, and one
``body(mem)`` per entry point of include/gatsspg_trainset.h that places its arguments through ``mem`` (tests/arena.py).
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np
import torch

import trainset_oracle as oracle
from onepose_amd import _native_trainset

BINDING = _native_trainset
_SAMPLES = dict(sample_image="in", sample_epoch="in")
ROLES = {
    "gts_assign_pairs": dict(point_offsets="in", obs_image="in", obs_kpt="in", kpt_offsets="in", pair_offsets="out", pair_kpt="out",
                             pair_point="out", ignored="out", workspace="scratch"),
    "gts_select_leaves": dict(point_offsets="in", leaf_src="out", **_SAMPLES),
    "gts_gather_leaves": dict(collect="in", leaf_src="in", descriptors2d_db="out"),
    "gts_pad_query": dict(desc2d="in", kpts2d="in", scores2d="in", kpt_offsets="in", image_hw="in", descriptors2d_query="out",
                          keypoints2d="out", scores_query="out", **_SAMPLES),
    "gts_pad_points": dict(points3d="in", mean_desc="in", keypoints3d="out", descriptors3d_db="out", **_SAMPLES),
    "gts_build_batch": dict(point_offsets="in", collect="in", points3d="in", mean_desc="in", desc2d="in", kpts2d="in", scores2d="in",
                            kpt_offsets="in", image_hw="in", descriptors2d_query="out", keypoints2d="out", scores_query="out",
                            keypoints3d="out", descriptors3d_db="out", descriptors2d_db="out", workspace="scratch", **_SAMPLES),
}
TILES = [(1, 1), (7, 9), (8, 8), (13, 5), (33, 8)]         # shape3d x num_leaf: 1, 63, 64, 65 and 264 leaf columns of a 64-column tile
SHAPES2D = [1, 63, 64, 65, 130]
N_KPTS = [0, 40, 63, 64, 65, 130, 200]                      # per image: none, and below / at / above every shape2d but 1
N_POINTS = 8                                                # above, at and below the shape3d of TILES
SEED = 0x5EED0123456789


@functools.lru_cache(maxsize=None)
def case(L):
    """8 points with 1, L - 1, L, L + 1, 3 L, 0, 2 and 5 observations, the seven images of N_KPTS (24 x 32 pixels, so that a random
    pad meets a keypoint of the 200 now and then); built once per L and shared read-only"""
    return oracle.make_case(N_POINTS, (1, max(L - 1, 0), L, L + 1, 3 * L, 0, 2, 5), N_KPTS, seed=L)


def samples(b, k=0):
    """b images and epochs; the k-th choice"""
    images = [(3 + k + 2 * i) % len(N_KPTS) for i in range(b)]
    return np.array(images, np.int32), np.array([k + i for i in range(b)], np.int32)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def place_tables(mem, c, names):
    t = oracle.tables(c)
    return [mem.place(i32(t[n]) if t[n].dtype.kind == "i" else f32(t[n]), "in", n) for n in names]


def out(mem, name, *shape, dtype=torch.float32):
    return mem.place(torch.empty(*shape, dtype=dtype), "out", name)


def workspace(mem, *shape):
    nbytes = BINDING.load().gts_workspace_bytes(*shape)
    assert nbytes > 0 and nbytes % 256 == 0
    return mem.place(nbytes, "scratch", "workspace")


def body_assign(c):
    t = oracle.tables(c)
    N, K, V, G = len(t["point_offsets"]) - 1, len(t["obs_image"]), len(t["kpt_offsets"]) - 1, int(t["kpt_offsets"][-1])
    total = int(oracle.assign_pairs(t["point_offsets"], t["obs_image"], t["obs_kpt"], t["kpt_offsets"])[0][-1])

    def body(mem):
        po, oi, ok, ko = place_tables(mem, c, ["point_offsets", "obs_image", "obs_kpt", "kpt_offsets"])
        offs, kpt, point = out(mem, "pair_offsets", V + 1, dtype=torch.int32), out(mem, "pair_kpt", K, dtype=torch.int32), out(mem, "pair_point", K, dtype=torch.int32)
        ignored = out(mem, "ignored", 1, dtype=torch.int32)
        ws = workspace(mem, G, 0, 0, 0)
        mem.call(BINDING, "gts_assign_pairs", po, oi, ok, N, K, ko, V, G, offs, kpt, point, ignored, ws, ws.numel())
        full = dict(pair_offsets=offs, pair_kpt=kpt, pair_point=point, ignored=ignored)
        return full, dict(pair_kpt=kpt[:total], pair_point=point[:total])       # the entries from pair_offsets[V] on are not written
    return body


def body_select(c, images, epochs, shape3d, L, seed=SEED):
    def body(mem):
        po, = place_tables(mem, c, ["point_offsets"])
        si, se = mem.place(i32(images), "in", "sample_image"), mem.place(i32(epochs), "in", "sample_epoch")
        leaf = out(mem, "leaf_src", len(images), shape3d * L, dtype=torch.int32)
        mem.call(BINDING, "gts_select_leaves", po, len(c["point_offsets"]) - 1, si, se, len(images), shape3d, L, seed, leaf)
        return dict(leaf_src=leaf)
    return body


def body_gather(c, leaf_src, shape3d, L, skew=0):
    def body(mem):
        co, = place_tables(mem, c, ["collect"])
        src = mem.place(i32(leaf_src), "in", "leaf_src")
        dst = mem.place(torch.empty(leaf_src.shape[0], 256, shape3d * L), "out", "descriptors2d_db", skew=skew)
        mem.call(BINDING, "gts_gather_leaves", co, len(c["collect"]), src, leaf_src.shape[0], shape3d, L, dst)
        return dict(descriptors2d_db=dst)
    return body


def body_pad_query(c, images, epochs, shape2d, seed=SEED):
    def body(mem):
        tabs = place_tables(mem, c, ["desc2d", "kpts2d", "scores2d", "kpt_offsets", "image_hw"])
        si, se = mem.place(i32(images), "in", "sample_image"), mem.place(i32(epochs), "in", "sample_epoch")
        b = len(images)
        dq, kq, sq = out(mem, "descriptors2d_query", b, 256, shape2d), out(mem, "keypoints2d", b, shape2d, 2), out(mem, "scores_query", b, shape2d)
        mem.call(BINDING, "gts_pad_query", *tabs, len(c["features"]), si, se, b, shape2d, seed, dq, kq, sq)
        return dict(descriptors2d_query=dq, keypoints2d=kq, scores_query=sq)
    return body


def body_pad_points(c, images, epochs, shape3d, seed=SEED):
    def body(mem):
        tabs = place_tables(mem, c, ["points3d", "mean_desc"])
        si, se = mem.place(i32(images), "in", "sample_image"), mem.place(i32(epochs), "in", "sample_epoch")
        b = len(images)
        k3, d3 = out(mem, "keypoints3d", b, shape3d, 3), out(mem, "descriptors3d_db", b, 256, shape3d)
        mem.call(BINDING, "gts_pad_points", *tabs, len(c["points3d"]), si, se, b, shape3d, seed, k3, d3)
        return dict(keypoints3d=k3, descriptors3d_db=d3)
    return body


def body_build(c, images, epochs, shape2d, shape3d, L, seed=SEED, calls=1):
    """``calls`` > 1: the same call again into the same tensors and workspace"""
    def body(mem):
        po, co, p3, md = place_tables(mem, c, ["point_offsets", "collect", "points3d", "mean_desc"])
        tabs = place_tables(mem, c, ["desc2d", "kpts2d", "scores2d", "kpt_offsets", "image_hw"])
        si, se = mem.place(i32(images), "in", "sample_image"), mem.place(i32(epochs), "in", "sample_epoch")
        b = len(images)
        dq, kq, sq = out(mem, "descriptors2d_query", b, 256, shape2d), out(mem, "keypoints2d", b, shape2d, 2), out(mem, "scores_query", b, shape2d)
        k3, d3, leaves = out(mem, "keypoints3d", b, shape3d, 3), out(mem, "descriptors3d_db", b, 256, shape3d), out(mem, "descriptors2d_db", b, 256, shape3d * L)
        ws = workspace(mem, 0, b, shape3d, L)
        for _ in range(calls):
            mem.call(BINDING, "gts_build_batch", po, co, p3, md, len(c["points3d"]), len(c["collect"]), *tabs, len(c["features"]), si, se, b, shape2d,
                     shape3d, L, seed, dq, kq, sq, k3, d3, leaves, ws, ws.numel())
        return dict(descriptors2d_query=dq, keypoints2d=kq, scores_query=sq, keypoints3d=k3, descriptors3d_db=d3, descriptors2d_db=leaves)
    return body
