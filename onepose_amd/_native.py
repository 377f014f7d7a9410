"""ctypes binding of libgatsspg_hip.so (C ABI declared in include/gatsspg.h).

The library is built in-tree by ``python -m onepose_amd.build_ext`` (hipcc, gfx950).  There is no
fallback: if the shared object is missing, ``load()`` raises.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_size_t, c_void_p

from ._binding import F32, I64, RAW, STREAM, NativeError, bind  # noqa: F401
from .build_ext import LIB_PATH

NUM_GATS, NUM_ATTN = 4, 8
FLAG_INCLUDE_SELF, FLAG_ADDITIONAL, FLAG_WITH_LINEAR_TRANSFORM = 1, 2, 4
FLAG_PREC_BF16X3 = 0x100
FLAG_PREC_BF16X6 = 0x200
FLAG_PREC_FP16X3 = 0x400
FLAG_PREC_FP16X4 = 0x800
FLAG_NO_DB_REUSE = 0x1000   # gatsspg_forward: always the plain chain (never set by the engine; the tests' reference for "identical")
PRECISIONS = {"fp32": 0, "bf16x3": FLAG_PREC_BF16X3, "bf16x6": FLAG_PREC_BF16X6, "fp16x3": FLAG_PREC_FP16X3, "fp16x4": FLAG_PREC_FP16X4}   # GEMM arithmetic of the attention layers, selected per call
KERNEL_IDS = {"load_state": 0, "gats": 1, "qkv_kv": 2, "kv_final": 3, "mlp0": 5, "stat_final": 6,
              "mlp3": 7, "final_proj_norm": 8, "score_exp": 9, "conf_finalize": 10, "match_tail": 11, "gats_wlt": 12,
              "softmax_stats": 13}
LAYER_SELF, LAYER_CROSS = 0, 1
MAX_FRAMES = 32      # GATSSPG_MAX_FRAMES: frames per gatsspg_forward_frames call


class RawWeights(ctypes.Structure):
    """struct gatsspg_raw_weights (device pointers)."""
    _fields_ = [
        ("gats_W", c_void_p * NUM_GATS), ("gats_a", c_void_p * NUM_GATS),
        ("proj_w", (c_void_p * 3) * NUM_ATTN), ("proj_b", (c_void_p * 3) * NUM_ATTN),
        ("merge_w", c_void_p * NUM_ATTN), ("merge_b", c_void_p * NUM_ATTN),
        ("mlp0_w", c_void_p * NUM_ATTN), ("mlp0_b", c_void_p * NUM_ATTN),
        ("mlp3_w", c_void_p * NUM_ATTN), ("mlp3_b", c_void_p * NUM_ATTN),
        ("final_w", c_void_p), ("final_b", c_void_p),
    ]


class KencWeights(ctypes.Structure):
    """struct gatsspg_kenc_weights (device pointers)."""
    _fields_ = [("w", c_void_p * 4), ("b", c_void_p * 4), ("inp_dim", c_int)]


_FWD_OUT = [F32, I64, I64, F32, F32, RAW, c_size_t, STREAM]      # conf, matches0 / 1, mscores0 / 1, ws, ws_bytes, stream
_FWD = [F32, F32, F32, F32, c_int, c_int, c_int, c_int, c_int, c_float, c_float] + _FWD_OUT
_STATE = [c_int, c_int, c_int, c_int]                             # b, n1, n2, num_leaf

# name -> (restype, parameters); every symbol include/gatsspg.h declares
SYMBOLS = {
    "gatsspg_version": (c_int, []),
    "gatsspg_last_error": (c_char_p, []),
    "gatsspg_packed_weights_bytes": (c_size_t, []),
    "gatsspg_workspace_bytes": (c_size_t, _STATE),
    "gatsspg_pack_weights": (c_int, [POINTER(RawWeights), F32, STREAM]),
    "gatsspg_forward": (c_int, _FWD),
    "gatsspg_forward_profiled": (c_int, _FWD + [c_int, c_int, c_void_p, c_void_p]),       # ... kernel_id, occurrence, two hipEvent_t
    "gatsspg_db_cache_bytes": (c_size_t, [c_int, c_int]),
    "gatsspg_prepare_database": (c_int, [F32, F32, F32, c_int, c_int, c_int, c_int, RAW, c_size_t, RAW, c_size_t, STREAM]),
    "gatsspg_forward_cached": (c_int, [F32, F32, F32, RAW, c_size_t, c_int, c_int, c_int, c_int, c_int, c_float, c_float]
                               + _FWD_OUT),
    # packed, desc2d_query [b,256,cap1], n1 (HOST int32 array, b entries), desc2d_db, cache, cache_bytes, b, cap1, n2, num_leaf, flags, ...
    "gatsspg_forward_frames": (c_int, [F32, F32, POINTER(c_int32), F32, RAW, c_size_t, c_int, c_int, c_int, c_int, c_int, c_float, c_float]
                               + _FWD_OUT),
    "gatsspg_gats_layer_frames": (c_int, [F32, c_int, F32, F32, c_int, c_int, c_int, c_int, c_int, c_int, RAW, c_size_t, STREAM]),
    "gatsspg_load_state": (c_int, [F32, F32] + _STATE + [RAW, c_size_t, STREAM]),
    "gatsspg_store_state": (c_int, [c_int, F32, F32] + _STATE + [RAW, c_size_t, STREAM]),
    "gatsspg_gats_layer": (c_int, [F32, c_int, F32] + _STATE + [c_int, RAW, c_size_t, STREAM]),
    "gatsspg_attn_layer": (c_int, [F32, c_int, c_int] + _STATE + [c_int, RAW, c_size_t, STREAM]),
    "gatsspg_final_proj_norm": (c_int, [F32] + _STATE + [RAW, c_size_t, STREAM]),
    "gatsspg_score_dual_softmax_match": (c_int, _STATE + [c_float, c_float] + _FWD_OUT),
    "gatsspg_kenc_scratch_bytes": (c_size_t, [c_int, c_int]),
    "gatsspg_keypoint_encoder": (c_int, [POINTER(KencWeights), F32, F32, c_int, c_int, F32, RAW, c_size_t, STREAM]),
}

_lib = None
load, check, call = bind(globals(), "GATsSPG", "gatsspg")
