"""ctypes binding of libdet_hip.so (C ABI declared in include/detector/detector.h and include/detector/flow.h).  No fallback: a missing library raises."""
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
# every symbol include/detector/flow.h declares (the tracker's flow step, same library): bound with the table above
FLOW_MIN_WINDOW, FLOW_MAX_WINDOW = 3, 31    # FLOW_MIN_WINDOW / FLOW_MAX_WINDOW
FLOW_MAX_LEVEL = 5                          # FLOW_MAX_LEVEL
FLOW_MAX_ITERATIONS = 100                   # FLOW_MAX_ITERATIONS
FLOW_MAX_SIZE = 4096                        # FLOW_MAX_SIZE
FLOW_MAX_POINTS = 65536                     # FLOW_MAX_POINTS
FLOW_REGISTER_SAMPLES = 256                 # FLOW_REGISTER_SAMPLES
FLOW_REPROJ_THREADS = 256                   # FLOW_REPROJ_THREADS
FLOW_EXIT = {"converged": 0, "oscillation": 1, "iteration_cap": 2, "left_range": 3, "rejected": 4, "skipped": 5}   # FLOW_EXIT_*
_WIN = [c_int, c_int]                       # win_w, win_h
MORE_SYMBOLS = {
    "flow_pyramid_bytes": (c_size_t, [c_int, c_int, c_int]),
    "flow_pyramid_levels": (c_int, [c_int, c_int] + _WIN + [c_int]),
    "flow_workspace_bytes": (c_size_t, [c_int] + _WIN),
    "flow_build_pyramid": (c_int, [U8, c_int, c_int, c_int, U8, STREAM]),
    "flow_patch_sums": (c_int, [U8, c_int, c_int, c_int, F64, c_int] + _WIN + [I64, RAW, STREAM]),       # out_patches: int16
    "flow_mismatch_sums": (c_int, [U8, U8, c_int, c_int, c_int, F64, F64, c_int] + _WIN + [I64, STREAM]),
    "flow_track": (c_int, [U8, U8, c_int, c_int, c_int, F32, F32, c_int] + _WIN + [c_int, c_double, c_double, F32, I32, I64, I32, RAW,
                           c_size_t, STREAM]),
    "flow_reproj_mean": (c_int, [F64, POINTER(c_double), F32, F32, I32, c_int, F64, STREAM]),
}

_lib = None
load, check, call = bind(globals(), "detector", "det", fallback="OpenCV")
