"""ctypes binding of libmap_hip.so (C ABI declared in include/mapping/mapping.h and include/mapping/bundle_adjust.h).  No fallback: a missing library raises."""
from __future__ import annotations

from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_size_t, c_uint64

from ._binding import F32, F64, I32, I64, RAW, STREAM, bind
from .build_ext import MAP_LIB_PATH as LIB_PATH

MAX_TRACK_LENGTH = 448                      # MAP_MAX_TRACK_LENGTH
MAX_POINTS = 32768                          # MAP_MAX_POINTS
MAX_LENGTH_BINS = 1024                      # MAP_MAX_LENGTH_BINS

# name -> (restype, parameters); every symbol include/mapping/mapping.h declares
SYMBOLS = {
    "map_version": (c_int, []),
    "map_last_error": (c_char_p, []),
    "map_workspace_bytes": (c_size_t, [c_int]),
    "map_verify_matches": (c_int, [F32, I32, F64, c_int, I32, I32, I64, c_int, c_double, c_int, I32, I32, STREAM]),
    "map_triangulate_tracks": (c_int, [I32, I32, F32, F64, c_int, c_int, c_int, c_double, c_double, c_int, c_int, c_uint64,
                                       F64, I32, I32, I32, STREAM]),
    "map_track_length_threshold": (c_int, [I32, c_int, c_int, I32, STREAM]),
    "map_filter_points": (c_int, [F64, I32, c_int, I32, POINTER(c_float), I32, F32, I32, STREAM]),
    "map_merge_points": (c_int, [F32, c_int, c_double, F32, I32, I32, I32, RAW, c_size_t, STREAM]),
    # desc_table / score_table: device arrays of device pointers
    "map_gather_descriptors": (c_int, [RAW, RAW, I32, c_int, I32, I32, I32, c_int, c_int, F32, F32, I64, F64, F64, STREAM]),
}
# every symbol include/mapping/bundle_adjust.h declares (the windowed bundle adjustment, same library): bound with the table above
BA_MAX_CAMERAS = 32                         # BA_MAX_CAMERAS
BA_MAX_POINTS = 32768                       # BA_MAX_POINTS
BA_MAX_OBSERVATIONS = 262144                # BA_MAX_OBSERVATIONS
BA_MAX_ITERATIONS = 1000                    # BA_MAX_ITERATIONS
BA_CAMERA_CHUNK = 256                       # BA_CAMERA_CHUNK
BA_TRACE_COLUMNS = 6                        # BA_TRACE_COLUMNS
BA_SUMMARY_ENTRIES = 6                      # BA_SUMMARY_ENTRIES
BA_STATUS_OK, BA_STATUS_NONFINITE_START = 0, 1
_OBS = [I32, I32]                           # obs_cam, obs_pt
_FIXED = [I32, I32]                         # cam_fixed, pt_fixed (None = none fixed)
_SIZES = [c_int, c_int, c_int]              # C, P, M
_WS = [RAW, c_size_t, STREAM]               # workspace, workspace_bytes, stream
MORE_SYMBOLS = {
    "ba_workspace_bytes": (c_size_t, _SIZES),
    "ba_solve": (c_int, [F64, F64, F64] + _OBS + [F64] + _FIXED + _SIZES + [c_int, c_int, F64, F64] + _WS),
    "ba_linearize": (c_int, [F64, F64, F64] + _OBS + [F64] + _SIZES + [F64, F64, F64, STREAM]),
    "ba_normal_blocks": (c_int, [F64, F64, F64] + _OBS + _FIXED + _SIZES + [F64, F64, F64, F64, F64] + _WS),
    "ba_step": (c_int, [F64, F64, F64, F64, F64, F64, F64] + _OBS + _FIXED + _SIZES + [c_double, F64, F64, F64] + _WS),
}

_lib = None
load, check, call = bind(globals(), "object database builder", "map", fallback="COLMAP")
