"""ctypes binding of libsuperglue_hip.so (C ABI declared in include/superglue/superglue.h).

Built in-tree by ``python -m onepose_amd.build_ext`` (hipcc, gfx950).  No fallback: if the shared
object is missing, ``load()`` raises.
"""
from __future__ import annotations

from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_size_t, c_void_p

from ._binding import bind
from .build_ext import SG_LIB_PATH as LIB_PATH

LAYER_SELF, LAYER_CROSS = 0, 1
MAX_ITEMS = 64          # SG_MAX_ITEMS: items of one ragged batch


def num_raw(n_layers):
    """Float tensors of the reference state_dict (num_batches_tracked skipped): SG_NUM_RAW."""
    return 29 + 16 * n_layers


_P = c_void_p
_I = POINTER(c_int32)   # a HOST int32 array
# name -> (restype, argtypes); every symbol include/superglue/superglue.h declares
SYMBOLS = {
    "sg_version": (c_int, []),
    "sg_last_error": (c_char_p, []),
    "sg_packed_weights_bytes": (c_size_t, [c_int]),
    "sg_pack_weights": (c_int, [POINTER(c_void_p), c_int, _P, _P]),
    "sg_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sg_forward": (c_int, [_P, c_int, POINTER(c_int32), c_int, c_float, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int,
                           c_int, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "sg_keypoint_encode": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P,
                                   c_size_t, _P]),
    "sg_layer": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "sg_attention": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P]),
    "sg_sinkhorn": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "sg_match_tail": (c_int, [_P, c_int, c_int, c_int, c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
    "sg_ragged_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sg_forward_ragged": (c_int, [_P, c_int, POINTER(c_int32), c_int, c_float, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _I, _I, _I,
                                  _I, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "sg_attention_ragged": (c_int, [_P, _P, c_int, c_int, c_int, _I, _I, _P, _P]),
    "sg_sinkhorn_ragged": (c_int, [_P, _P, c_int, c_int, c_int, _I, _I, c_int, _P, _P, c_size_t, _P]),
    "sg_match_tail_ragged": (c_int, [_P, c_int, c_int, c_int, _I, _I, c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
}

_lib = None
load, check = bind(globals(), "SuperGlue", "sg")
