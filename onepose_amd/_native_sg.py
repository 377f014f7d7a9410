"""ctypes binding of libsuperglue_hip.so (C ABI declared in include/superglue/superglue.h and include/superglue/nn_matcher.h).

Built in-tree by ``python -m onepose_amd.build_ext`` (hipcc, gfx950).  No fallback: if the shared
object is missing, ``load()`` raises.
"""
from __future__ import annotations

from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_size_t, c_void_p

from ._binding import F32, I64, RAW, STREAM, bind
from .build_ext import SG_LIB_PATH as LIB_PATH

LAYER_SELF, LAYER_CROSS = 0, 1
MAX_ITEMS = 64          # SG_MAX_ITEMS: items of one ragged batch
NNM_MAX_ITEMS = 64      # NNM_MAX_ITEMS: items of one nearest-neighbour call
NNM_TILE = (128, 64)    # NNM_TILE_ROWS x NNM_TILE_COLS: the similarity tile (tests place their shapes around it)


def num_raw(n_layers):
    """Float tensors of the reference state_dict (num_batches_tracked skipped): SG_NUM_RAW."""
    return 29 + 16 * n_layers


_I = POINTER(c_int32)   # a HOST int32 array
_SIDES = [F32, F32, F32, F32, F32, F32]                            # kpts0, scores0, desc0, kpts1, scores1, desc1
_MATCHES = [I64, I64, F32, F32]                                    # matches0 / 1, mscores0 / 1
_WS = [RAW, c_size_t, STREAM]                                      # workspace, workspace_bytes, stream
# name -> (restype, parameters); every symbol include/superglue/superglue.h declares
SYMBOLS = {
    "sg_version": (c_int, []),
    "sg_last_error": (c_char_p, []),
    "sg_packed_weights_bytes": (c_size_t, [c_int]),
    "sg_pack_weights": (c_int, [POINTER(c_void_p), c_int, F32, STREAM]),
    "sg_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sg_forward": (c_int, [F32, c_int, _I, c_int, c_float] + _SIDES + [c_int, c_int, c_int, c_int, c_int, c_int, c_int]
                   + _MATCHES + [F32] + _WS),
    "sg_keypoint_encode": (c_int, [F32, c_int] + _SIDES + [c_int, c_int, c_int, c_int, c_int, c_int, c_int, F32, F32] + _WS),
    "sg_layer": (c_int, [F32, c_int, c_int, c_int, F32, F32, c_int, c_int, c_int, F32, F32] + _WS),
    "sg_attention": (c_int, [F32, F32, c_int, c_int, c_int, F32, STREAM]),
    "sg_sinkhorn": (c_int, [F32, F32, c_int, c_int, c_int, c_int, F32] + _WS),
    "sg_match_tail": (c_int, [F32, c_int, c_int, c_int, c_float] + _MATCHES + _WS),
    "sg_ragged_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sg_forward_ragged": (c_int, [F32, c_int, _I, c_int, c_float] + _SIDES + [c_int, c_int, c_int, _I, _I, _I, _I]
                          + _MATCHES + [F32] + _WS),
    "sg_attention_ragged": (c_int, [F32, F32, c_int, c_int, c_int, _I, _I, F32, STREAM]),
    "sg_sinkhorn_ragged": (c_int, [F32, F32, c_int, c_int, c_int, _I, _I, c_int, F32] + _WS),
    "sg_match_tail_ragged": (c_int, [F32, c_int, c_int, c_int, _I, _I, c_float] + _MATCHES + _WS),
}
# every symbol include/superglue/nn_matcher.h declares (the nearest-neighbour matcher, same library): bound with the table above
_TESTS = [c_double, c_double, c_int]                               # ratio, distance, mutual
MORE_SYMBOLS = {
    "nnm_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "nnm_match": (c_int, [F32, F32, c_int, c_int, c_int] + _TESTS + _MATCHES + _WS + [c_int]),
    "nnm_match_ragged": (c_int, [F32, F32, _I, _I, c_int, c_int, c_int, c_int] + _TESTS + _MATCHES + _WS + [c_int]),
    "nnm_similarity": (c_int, [F32, F32, c_int, c_int, F32] + _WS + [c_int]),
}

_lib = None
load, check, call = bind(globals(), "SuperGlue", "sg")
