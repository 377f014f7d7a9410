"""ctypes binding of libspp_hip.so (C ABI declared in include/superpoint.h).

Built in-tree by ``python -m onepose_amd.build_ext`` (hipcc, gfx950).  No fallback: if the shared
object is missing, ``load()`` raises.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int, c_size_t, c_void_p

from ._binding import F32, I32, RAW, STREAM, bind
from .build_ext import SPP_LIB_PATH as LIB_PATH

NUM_LAYERS = 12
LAYER_NAMES = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b",
               "convPa", "convPb", "convDa", "convDb")
KERNEL_IDS = {"conv1a": 0, "conv1b": 1, "pool": 2, "conv2": 3, "conv3a": 4, "conv3b": 5, "conv4": 6, "heads": 7,
              "convPb": 8, "convDb": 9, "score_map": 10, "nms": 11, "rowcount": 12, "rowscan": 13, "compact": 14,
              "select": 15, "cellnorm": 16, "sample": 17, "rank": 18, "scatter": 19}


class RawWeights(ctypes.Structure):
    """struct spp_raw_weights (device pointers, forward order)."""
    _fields_ = [("weight", c_void_p * NUM_LAYERS), ("bias", c_void_p * NUM_LAYERS)]


FLAG_PREC_FP16X4 = 0x800
PRECISIONS = {"fp32": 0, "fp16x4": FLAG_PREC_FP16X4}   # arithmetic of the GEMM convolutions, a `flags` bit per call

# spp_dense_stage: (channels, log2 of the down-sampling) of stage 0 .. 10
DENSE_STAGES = ((64, 0), (64, 1), (64, 1), (64, 2), (128, 2), (128, 3), (128, 3), (128, 3), (512, 3), (65, 3), (256, 3))

_DETECT = [c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int, F32, F32, F32, I32]   # b, H, W, nms_radius .. counts
_WS = [RAW, c_size_t, STREAM]
_FWD = [F32, F32] + _DETECT + _WS + [c_int]

# name -> (restype, parameters); every symbol include/superpoint.h declares
SYMBOLS = {
    "spp_version": (c_int, []),
    "spp_last_error": (c_char_p, []),
    "spp_packed_weights_bytes": (c_size_t, []),
    "spp_pack_weights": (c_int, [POINTER(RawWeights), F32, STREAM]),
    "spp_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "spp_dense": (c_int, [F32, F32, c_int, c_int, c_int, F32, F32] + _WS + [c_int]),
    "spp_dense_stage": (c_int, [F32, F32, c_int, c_int, c_int, c_int, F32] + _WS + [c_int]),      # ... stage, out (stage tests)
    "spp_detect": (c_int, [F32, F32] + _DETECT + [F32] + _WS),
    "spp_forward": (c_int, _FWD),
    "spp_forward_profiled": (c_int, _FWD + [c_int, c_int, c_void_p, c_void_p]),      # ... kernel_id, occurrence, two hipEvent_t
}

_lib = None
load, check, call = bind(globals(), "SuperPoint", "spp")
