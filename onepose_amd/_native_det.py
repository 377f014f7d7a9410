"""ctypes binding of libdet_hip.so (C ABI declared in include/detector/detector.h).  No fallback: a missing library raises."""
from __future__ import annotations

from ctypes import POINTER, c_char_p, c_double, c_int, c_size_t, c_uint64

from ._binding import F32, F64, I32, I64, RAW, STREAM, U8, bind
from .build_ext import DET_LIB_PATH as LIB_PATH

RANK_BY = {"matches": 0, "inliers": 1}      # DET_RANK_BY_MATCHES / DET_RANK_BY_INLIERS
MIN_MATCHES = 6                             # DET_MIN_MATCHES

_FIT = [c_double, c_int, c_uint64, F64, I32, I32, RAW, c_size_t, STREAM]   # threshold, iterations, seed, affine, mask, info, ws
# name -> (restype, parameters); every symbol include/detector/detector.h declares
SYMBOLS = {
    "det_version": (c_int, []),
    "det_last_error": (c_char_p, []),
    "det_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "det_affine_partial_ransac": (c_int, [F32, F32, c_int] + _FIT),
    "det_affine_partial_from_matches": (c_int, [F32, I32, I64, F32, c_int, c_int, c_int] + _FIT),
    "det_bbox_vote": (c_int, [F64, I32, I32, c_int, c_int, c_int, c_int, I32, I32, I32, STREAM]),
    "det_crop_resize": (c_int, [U8, c_int, c_int, I32, POINTER(c_double), c_int, F32, F64, I32, STREAM]),
}

_lib = None
load, check, call = bind(globals(), "detector", "det", fallback="OpenCV")
