"""ctypes binding of libpnp_hip.so (C ABI declared in include/pnp.h).  No fallback: a missing library raises."""
from __future__ import annotations

from ctypes import POINTER, c_char_p, c_double, c_int, c_size_t, c_uint64, c_void_p

from ._binding import bind
from .build_ext import PNP_LIB_PATH as LIB_PATH

# name -> (restype, argtypes); every symbol include/pnp.h declares
SYMBOLS = {
    "pnp_version": (c_int, []),
    "pnp_last_error": (c_char_p, []),
    "pnp_workspace_bytes": (c_size_t, [c_int, c_int]),
    "pnp_ransac_epnp": (c_int, [c_void_p, c_void_p, POINTER(c_double), c_double, c_int, c_double, c_int, c_uint64, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pnp_ransac_epnp_matches": (c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(c_double), c_double, c_double, c_int, c_uint64,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pnp_epnp": (c_int, [c_void_p, c_void_p, POINTER(c_double), c_double, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
}

_lib = None
load, check = bind(globals(), "PnP", "pnp")
