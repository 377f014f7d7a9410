"""ctypes binding of libmap_hip.so (C ABI declared in include/mapping/mapping.h).  No fallback: a missing library raises."""
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

_lib = None
load, check, call = bind(globals(), "object database builder", "map", fallback="COLMAP")
