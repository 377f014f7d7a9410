"""ctypes binding of the matcher's training head in libgatsspg_hip.so (C ABI declared in include/gatsspg_train.h).  No fallback: a missing library raises."""
from __future__ import annotations

from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_size_t

import torch

from . import build_ext
from ._binding import F32, F64, I32, I64, RAW, STREAM, DevicePointer, bind

LIB_PATH = build_ext.LIB_PATH

I8 = DevicePointer("I8", torch.int8)        # the class matrix
DESC_DIM = 256                              # GTR_DESC_DIM
MAX_BATCH = 64                              # GTR_MAX_BATCH
MAX_POINTS = 1 << 22                        # GTR_MAX_POINTS
MAX_ELEMENTS = 1 << 26                      # GTR_MAX_ELEMENTS
CLASS_NEGATIVE, CLASS_POSITIVE, CLASS_IGNORED = 0, 1, 2     # GTR_CLASS_*

_WS = [RAW, c_size_t, STREAM]               # workspace, workspace_bytes, stream
_HOST_I32 = POINTER(c_int32)                # a host array of b ints
# name -> (restype, parameters); every symbol include/gatsspg_train.h declares
SYMBOLS = {
    "gtr_version": (c_int, []),
    "gtr_last_error": (c_char_p, []),
    "gtr_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    # pairs | k, n_orig, m_orig (host) | b, kcap, n, m, pad_is_negative | cls, negative_pairs
    "gtr_build_target": (c_int, [I32, _HOST_I32, _HOST_I32, _HOST_I32, c_int, c_int, c_int, c_int, c_int, I8, I32, STREAM]),
    # x, y, cls | b, n, m | alpha, gamma, pos_w, neg_w, scale | loss, counts, dx, dy
    "gtr_loss_head": (c_int, [F32, F32, I8, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_double, F32, I64, F32, F32] + _WS),
    # x, y | b, n, m, scale | E, r, c
    "gtr_scores_exp": (c_int, [F32, F32, c_int, c_int, c_int, c_double, F32, F32, F32] + _WS),
    # E, r, c, cls | b, n, m | alpha, gamma, pos_w, neg_w | loss_sums, counts, loss, rowsum_h, colsum_h
    "gtr_loss_terms": (c_int, [F32, F32, F32, I8, c_int, c_int, c_int, c_double, c_double, c_double, c_double, F64, I64, F32, F32, F32] + _WS),
    # E, r, c, cls, counts, rowsum_h, colsum_h | b, n, m | alpha, gamma, pos_w, neg_w | dS
    "gtr_score_grad": (c_int, [F32, F32, F32, I8, I64, F32, F32, c_int, c_int, c_int, c_double, c_double, c_double, c_double, F32] + _WS),
}

_lib = None
load, check, call = bind(globals(), "matcher training head", "gtr")
