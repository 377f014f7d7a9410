"""ctypes binding of libpnp_hip.so (C ABI declared in include/pnp.h and include/pnp_batch.h).  No fallback: a missing library raises."""
from __future__ import annotations

from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_size_t, c_uint64

from ._binding import F32, F64, I32, I64, RAW, STREAM, bind
from .build_ext import PNP_LIB_PATH as LIB_PATH

MAX_ITEMS = 32                                            # PNP_MAX_ITEMS: frames of one batched call
_K = POINTER(c_double)                                    # K_host: nine HOST doubles (per frame)
_N, _SEEDS = POINTER(c_int32), POINTER(c_uint64)          # per-frame counts and seeds: HOST arrays
_OUT = [F64, I32, I32, RAW, c_size_t, STREAM]             # pose, inlier_mask, info, workspace, workspace_bytes, stream
# name -> (restype, parameters); every symbol include/pnp.h declares
SYMBOLS = {
    "pnp_version": (c_int, []),
    "pnp_last_error": (c_char_p, []),
    "pnp_workspace_bytes": (c_size_t, [c_int, c_int]),
    "pnp_ransac_epnp": (c_int, [F32, F32, _K, c_double, c_int, c_double, c_int, c_uint64] + _OUT),
    "pnp_ransac_epnp_matches": (c_int, [F32, F32, I64, c_int, _K, c_double, c_double, c_int, c_uint64] + _OUT),
    "pnp_epnp": (c_int, [F32, F32, _K, c_double, c_int, F64, RAW, c_size_t, STREAM]),
    # the stages of pnp_ransac_epnp on caller-provided buffers (stage tests)
    "pnp_hypotheses": (c_int, [F32, F32, _K, c_double, c_int, c_int, c_uint64, F64, STREAM]),
    "pnp_score_hypotheses": (c_int, [F32, F32, _K, c_double, c_int, c_double, F64, c_int, I32, STREAM]),
    "pnp_select_best": (c_int, [F32, F32, _K, c_double, c_int, c_double, F64, I32, c_int, I32, I32, I32, STREAM]),
    "pnp_refit": (c_int, [F32, F32, _K, c_double, c_int, I32, I32, I32, F64, STREAM]),
}
# every symbol include/pnp_batch.h declares (the header include/pnp.h ends with): bound with the table above
MORE_SYMBOLS = {
    "pnp_batch_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "pnp_ransac_epnp_batch": (c_int, [F32, F32, _K, _N, _SEEDS, c_int, c_int, c_double, c_double, c_int] + _OUT),
    "pnp_ransac_epnp_matches_batch": (c_int, [F32, F32, I64, _K, _N, _SEEDS, c_int, c_int, c_int, c_int, c_double, c_double, c_int] + _OUT),
}

_lib = None
load, check, call = bind(globals(), "PnP", "pnp")
