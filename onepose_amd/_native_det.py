"""ctypes binding of libdet_hip.so (C ABI declared in include/detector/detector.h).  No fallback: a missing library raises."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_size_t, c_uint64, c_void_p

from ._native import NativeError
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


def load():
    """dlopen the HIP library and bind every entry point.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} is missing: the detector HIP extension has not been built "
            "(run `python -m onepose_amd.build_ext`; needs hipcc).  There is no CPU / OpenCV fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().det_last_error()
        raise NativeError(f"{what} failed: {msg.decode() if msg else 'unknown error'}")
