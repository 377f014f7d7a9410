"""ctypes binding of libdet_hip.so (C ABI declared in include/detector/detector.h).  No fallback: a missing library raises."""
from __future__ import annotations

from ctypes import POINTER, c_char_p, c_double, c_int, c_size_t, c_uint64, c_void_p

from ._binding import bind
from .build_ext import DET_LIB_PATH as LIB_PATH

RANK_BY = {"matches": 0, "inliers": 1}      # DET_RANK_BY_MATCHES / DET_RANK_BY_INLIERS
MIN_MATCHES = 6                             # DET_MIN_MATCHES

_P = c_void_p
# name -> (restype, argtypes); every symbol include/detector/detector.h declares
SYMBOLS = {
    "det_version": (c_int, []),
    "det_last_error": (c_char_p, []),
    "det_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "det_affine_partial_ransac": (c_int, [_P, _P, c_int, c_double, c_int, c_uint64, _P, _P, _P, _P, c_size_t, _P]),
    "det_affine_partial_from_matches": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_double, c_int, c_uint64, _P, _P, _P, _P,
                                                c_size_t, _P]),
    "det_bbox_vote": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "det_crop_resize": (c_int, [_P, c_int, c_int, _P, POINTER(c_double), c_int, _P, _P, _P, _P]),
}

_lib = None
load, check = bind(globals(), "detector", "det", fallback="OpenCV")
