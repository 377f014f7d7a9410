"""ctypes binding of the training-set builder in libgatsspg_hip.so (C ABI declared in include/gatsspg_trainset.h).  No fallback: a missing library raises."""
from __future__ import annotations

from ctypes import c_char_p, c_int, c_size_t, c_uint64

from . import build_ext
from ._binding import F32, I32, RAW, STREAM, bind

LIB_PATH = build_ext.LIB_PATH

DESC_DIM = 256                              # GTS_DESC_DIM
MAX_BATCH = 64                              # GTS_MAX_BATCH
MAX_POINTS = 1 << 22                        # GTS_MAX_POINTS
MAX_LEAF = 64                               # GTS_MAX_LEAF
MAX_COLUMNS = 1 << 24                       # GTS_MAX_COLUMNS
MAX_REDRAWS = 256                           # GTS_MAX_REDRAWS
TAG_LEAVES, TAG_PAD2D, TAG_PAD3D = 1, 2, 3  # GTS_TAG_*

_SAMPLES = [I32, I32, c_int]                # sample_image, sample_epoch, b
# name -> (restype, parameters); every symbol include/gatsspg_trainset.h declares
SYMBOLS = {
    "gts_version": (c_int, []),
    "gts_last_error": (c_char_p, []),
    "gts_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    # point_offsets, obs_image, obs_kpt | N, K | kpt_offsets | V, total_kpts | pair_offsets, pair_kpt, pair_point, ignored | workspace
    "gts_assign_pairs": (c_int, [I32, I32, I32, c_int, c_int, I32, c_int, c_int, I32, I32, I32, I32, RAW, c_size_t, STREAM]),
    # point_offsets, N | samples | shape3d, num_leaf, seed | leaf_src
    "gts_select_leaves": (c_int, [I32, c_int] + _SAMPLES + [c_int, c_int, c_uint64, I32, STREAM]),
    # collect, K, leaf_src | b, shape3d, num_leaf | descriptors2d_db
    "gts_gather_leaves": (c_int, [F32, c_int, I32, c_int, c_int, c_int, F32, STREAM]),
    # desc2d, kpts2d, scores2d, kpt_offsets, image_hw, V | samples | shape2d, seed | descriptors2d_query, keypoints2d, scores_query
    "gts_pad_query": (c_int, [F32, F32, F32, I32, I32, c_int] + _SAMPLES + [c_int, c_uint64, F32, F32, F32, STREAM]),
    # points3d, mean_desc, N | samples | shape3d, seed | keypoints3d, descriptors3d_db
    "gts_pad_points": (c_int, [F32, F32, c_int] + _SAMPLES + [c_int, c_uint64, F32, F32, STREAM]),
    # point_offsets, collect, points3d, mean_desc, N, K | desc2d, kpts2d, scores2d, kpt_offsets, image_hw, V | samples | shape2d, shape3d,
    # num_leaf, seed | descriptors2d_query, keypoints2d, scores_query, keypoints3d, descriptors3d_db, descriptors2d_db | workspace
    "gts_build_batch": (c_int, [I32, F32, F32, F32, c_int, c_int, F32, F32, F32, I32, I32, c_int] + _SAMPLES +
                        [c_int, c_int, c_int, c_uint64, F32, F32, F32, F32, F32, F32, RAW, c_size_t, STREAM]),
}

_lib = None
load, check, call = bind(globals(), "training set", "gts")
