"""What the five ctypes bindings (_native*.py) and the four front ends share: loading a library and turning its return
codes into exceptions, the stream handle / current-device / intrinsics plumbing between a tensor and a C-ABI call, and the
two per-engine caches (packed weights, workspaces).
"""
from __future__ import annotations

import collections
import ctypes
import functools
import os

import numpy as np
import torch


class NativeError(RuntimeError):
    pass


def bind(ns, what, prefix, fallback="PyTorch"):
    """(load, check) of one binding module.  ``ns`` is that module's ``globals()``: ``LIB_PATH``, ``SYMBOLS`` and the cached
    ``_lib`` are read through it on every call, so assigning ``LIB_PATH`` before the first ``load()`` selects the library and
    ``_lib = None`` makes the next ``load()`` bind again.  There is no fallback: a missing shared object raises."""

    def load():
        """dlopen the HIP library and bind every entry point.  Raises if it has not been built."""
        lib = ns["_lib"]
        if lib is not None:
            return lib
        path = ns["LIB_PATH"]
        if not os.path.exists(path):
            raise NativeError(
                f"{path} is missing: the {what} HIP extension has not been built "
                f"(run `python -m onepose_amd.build_ext`; needs hipcc).  There is no CPU / {fallback} fallback.")
        lib = ctypes.CDLL(path)
        for name, (restype, argtypes) in ns["SYMBOLS"].items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = restype
            fn.argtypes = argtypes
        ns["_lib"] = lib
        return lib

    def check(rc, call):
        if rc != 0:
            msg = getattr(load(), prefix + "_last_error")()
            raise NativeError(f"{call} failed: {msg.decode() if msg else 'unknown error'}")

    return load, check


def stream_handle(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_device(fn):
    """Run an engine method with the CURRENT HIP device set to the device of its first tensor argument / `dims`: the
    C ABI takes a stream handle but launches (and sets kernel attributes) on the current device, so
    ``model.to('cuda:1')(inputs)`` must not depend on the caller having called ``torch.cuda.set_device(1)``."""

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        dev = None
        for a in args:
            if torch.is_tensor(a):
                dev = a.device
                break
            if isinstance(a, tuple) and a and isinstance(a[-1], torch.device):
                dev = a[-1]
                break
        if dev is None or dev.type != "cuda":
            return fn(self, *args, **kwargs)
        with torch.cuda.device(dev):
            return fn(self, *args, **kwargs)
    return wrapper


def k_array(K):
    """A 3x3 intrinsic matrix (tensor or array-like) as the nine host doubles the C ABIs take."""
    k = np.ascontiguousarray(np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64)).reshape(9)
    return (ctypes.c_double * 9)(*k.tolist())


class PackedWeights:
    """The device-side packed-weights blob of one engine, valid for one (device, parameter storage, parameter version).

    The blob is written once on the stream that first asks for it; an event recorded behind that write is waited on by
    every other stream before its first read, and a re-pack (weights changed) synchronises the device before the old blob
    is dropped -- so concurrent use of a module from several streams is safe including the first call on each stream."""

    def __init__(self, refusal):
        self.refusal = refusal         # message for a parameter that is not on a GPU; {} = where it is
        self.blob = None
        self.key = None
        self.event = None              # recorded on the packing stream right after the engine's *_pack_weights
        self.stream = None

    def get(self, device, params, pack):
        """``params``: the live tensors the forward reads; ``pack(tensors)``: allocate the blob and enqueue the library's
        ``*_pack_weights`` over fp32 contiguous copies of them on the current stream (called with ``device`` current)."""
        key = (str(device), [p._version for p in params], [p.data_ptr() for p in params])
        if self.blob is not None and key == self.key:
            cur = torch.cuda.current_stream(device)
            if cur.cuda_stream != self.stream:             # another stream: order its reads behind the pack kernels
                cur.wait_event(self.event)
            return self.blob
        if self.blob is not None:
            torch.cuda.synchronize(self.blob.device)       # re-pack: nobody may still be reading the blob that is dropped below
        for p in params:
            if not p.is_cuda:
                raise RuntimeError(self.refusal.format(p.device))
        # the copies may be released on return: the caching allocator is stream-ordered and the packing kernels were
        # enqueued on this stream
        keep = [p.detach().to(device=device, dtype=torch.float32).contiguous() for p in params]
        with torch.cuda.device(device):
            blob = pack(keep)
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(device))
            self.stream = torch.cuda.current_stream(device).cuda_stream
        self.blob, self.key = blob, key
        return blob


class WorkspaceCache:
    """Workspaces cached per (shape, device, STREAM): two calls of one module on two streams never share scratch.

    Least-recently-used eviction, one entry at a time (a clear-all at the cap dropped and re-allocated every workspace in
    turn for 3 database sizes x 4 streams); the byte cap keeps a pathological mix (many large batched shapes) from pinning
    HBM."""

    def __init__(self, max_entries, max_bytes=float("inf")):
        self.max_entries, self.max_bytes = max_entries, max_bytes
        self.entries = collections.OrderedDict()
        self.bytes = 0
        self.allocations = 0           # how many workspaces were ever allocated (tests: no re-allocation after warm-up)

    def get(self, shape, device, size, refusal):
        """``size(*shape)``: the library's ``*_workspace_bytes``; ``refusal()``: the message when it returns 0."""
        key = shape + (str(device), torch.cuda.current_stream(device).cuda_stream)
        ws = self.entries.get(key)
        if ws is not None:
            self.entries.move_to_end(key)
            return ws
        nbytes = size(*shape)
        if nbytes == 0:
            raise NativeError(refusal())
        # evict the least recently used entries, one at a time (the caching allocator keeps a dropped buffer alive until the
        # stream it was used on is done with it: record_stream is not needed for a buffer that only ever saw its own stream)
        while self.entries and (len(self.entries) >= self.max_entries or self.bytes + nbytes > self.max_bytes):
            _, old = self.entries.popitem(last=False)
            self.bytes -= old.numel()
        ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
        self.entries[key] = ws
        self.bytes += nbytes
        self.allocations += 1
        return ws
