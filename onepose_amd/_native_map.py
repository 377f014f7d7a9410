"""ctypes binding of libmap_hip.so (C ABI declared in include/mapping/mapping.h).  No fallback: a missing library raises."""
from __future__ import annotations

from ctypes import c_char_p, c_double, c_int, c_size_t, c_uint64, c_void_p

from ._binding import bind
from .build_ext import MAP_LIB_PATH as LIB_PATH

MAX_TRACK_LENGTH = 448                      # MAP_MAX_TRACK_LENGTH
MAX_POINTS = 32768                          # MAP_MAX_POINTS
MAX_LENGTH_BINS = 1024                      # MAP_MAX_LENGTH_BINS

_P = c_void_p
# name -> (restype, argtypes); every symbol include/mapping/mapping.h declares
SYMBOLS = {
    "map_version": (c_int, []),
    "map_last_error": (c_char_p, []),
    "map_workspace_bytes": (c_size_t, [c_int]),
    "map_verify_matches": (c_int, [_P, _P, _P, c_int, _P, _P, _P, c_int, c_double, c_int, _P, _P, _P]),
    "map_triangulate_tracks": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_double, c_double, c_int, c_int, c_uint64, _P, _P, _P, _P,
                                       _P]),
    "map_track_length_threshold": (c_int, [_P, c_int, c_int, _P, _P]),
    "map_filter_points": (c_int, [_P, _P, c_int, _P, _P, _P, _P, _P, _P]),
    "map_merge_points": (c_int, [_P, c_int, c_double, _P, _P, _P, _P, _P, c_size_t, _P]),
    "map_gather_descriptors": (c_int, [_P, _P, _P, c_int, _P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P, _P]),
}

_lib = None
load, check = bind(globals(), "object database builder", "map", fallback="COLMAP")
