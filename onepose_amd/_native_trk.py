"""ctypes binding of the tracker's map update step in libmap_hip.so (C ABI declared in include/mapping/track_update.h).  No fallback: a missing library raises."""
from __future__ import annotations

from ctypes import c_char_p, c_double, c_int, c_size_t

from . import build_ext
from ._binding import F32, F64, I32, RAW, STREAM, bind

LIB_PATH = build_ext.MAP_LIB_PATH

MAX_KEYPOINTS = 8192                        # TRK_MAX_KEYPOINTS
SUMMARY_ENTRIES = 8                         # TRK_SUMMARY_ENTRIES

_WS = [RAW, c_size_t, STREAM]               # workspace, workspace_bytes, stream
# name -> (restype, parameters); every symbol include/mapping/track_update.h declares, and the two of mapping.h it leans on
SYMBOLS = {
    "map_version": (c_int, []),
    "map_last_error": (c_char_p, []),
    "trk_workspace_bytes": (c_size_t, [c_int, c_int]),
    # matches0, kf_xy, q_xy, kf_pt_ids, points, K_kf, K_q, pose_kf, pose_q | n_kf, n_q, n_points | gate_factor, max_reproj, max_z |
    # pair_kf, pair_q, q_pt_ids, pair_dist, new_points, unmatched_q, median, summary
    "trk_update": (c_int, [I32, F32, F32, I32, F64, F64, F64, F64, F64, c_int, c_int, c_int, c_double, c_double, c_double,
                           I32, I32, I32, F64, F64, I32, F64, I32] + _WS),
    "trk_triangulate_pairs": (c_int, [F64, F64, F32, F32, c_int, F64, STREAM]),
    "trk_gate_median": (c_int, [F64, c_int, c_double, F64, I32] + _WS),
}

_lib = None
load, check, call = bind(globals(), "tracker map update", "map", fallback="numpy")
