"""What the six ctypes bindings (_native*.py) and the front ends share.

A binding's ``SYMBOLS`` table mirrors its header: scalars and HOST pointers are ctypes types, a DEVICE pointer is the marker
of its element type (``F32`` ``F64`` ``I32`` ``I64`` ``U8``; ``RAW`` for ``void*`` memory) and the stream slot is ``STREAM``.
A library whose ABI spans a second header lists that header's symbols in ``MORE_SYMBOLS``, bound alike.
``bind()`` lowers the markers to ``c_void_p``, so a raw ``lib.fn(int, ...)`` call (bench.py, tools/, the tests) is plain ctypes;
the front ends go through ``call(name, device, *tensors and scalars)``, which makes ``device`` current, fills the stream slot,
refuses a tensor of the wrong device / dtype / layout before the library is entered and turns a return code into
``NativeError``.  ``marshal`` is that check on its own, a pure function of a ``Signature`` (the declared parameters, sorted
once when the library is bound).  ``gpu_tensor`` is the one conversion in front of a call, ``Engine`` the packed-weights and
workspace caches the three network front ends derive from.
"""
from __future__ import annotations

import collections
import ctypes
import os

import numpy as np
import torch


class NativeError(RuntimeError):
    pass


class DevicePointer:
    """A device pointer parameter and the dtype of what it points to (None: any)."""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype

    def __repr__(self):
        return self.name


F32, F64 = DevicePointer("F32", torch.float32), DevicePointer("F64", torch.float64)
I32, I64 = DevicePointer("I32", torch.int32), DevicePointer("I64", torch.int64)
U8 = DevicePointer("U8", torch.uint8)
RAW = DevicePointer("RAW", None)
STREAM = DevicePointer("STREAM", None)      # the hipStream_t slot: filled by call(), never passed


class Signature:
    """The declared parameters of one entry point, sorted once: which of the arguments a caller passes (everything but
    the streams) are device pointers, and where the stream goes."""

    def __init__(self, params):
        self.params = list(params)
        passed = [p for p in self.params if p is not STREAM]
        self.n_args = len(passed)
        self.pointers = [(i, p) for i, p in enumerate(passed) if isinstance(p, DevicePointer)]   # (argument position, marker)
        self.streams = [i for i, p in enumerate(self.params) if p is STREAM]                      # positions in the full list


def marshal(name, sig, args, device, stream):
    """The ctypes argument list of ``name`` (``sig``: its Signature) for ``args``.  A device-pointer slot takes a contiguous
    tensor of its dtype on ``device`` (-> its address) or None (-> NULL; the C side says whether it may be); every stream
    slot gets ``stream``; scalars and host pointers pass through to ctypes."""
    if len(args) != sig.n_args:
        raise TypeError(f"{name} takes {sig.n_args} arguments besides the stream ({len(args)} given)")
    out = list(args)
    for i, p in sig.pointers:
        a = out[i]
        if a is None:
            continue
        try:        # three attribute reads per tensor: this loop is on every frame's path
            bad = a.device != device or (p.dtype is not None and a.dtype is not p.dtype) or not a.is_contiguous()
        except AttributeError:
            raise TypeError(f"{name} argument {i}: expected a {p} tensor or None, got {type(a).__name__}") from None
        if bad:
            raise TypeError(f"{name} argument {i}: expected a contiguous {p} tensor on {device}, got "
                            f"{'a contiguous' if a.is_contiguous() else 'a strided'} {a.dtype} tensor on {a.device}")
        out[i] = a.data_ptr()
    for i in sig.streams:
        out.insert(i, stream)
    return out


def bind(ns, what, prefix, fallback="PyTorch"):
    """(load, check, call) of one binding module.  ``ns`` is that module's ``globals()``: ``LIB_PATH``, ``SYMBOLS`` and the
    cached ``_lib`` are read through it on every call, so assigning ``LIB_PATH`` before the first ``load()`` selects the library
    and ``_lib = None`` makes the next ``load()`` bind again.  There is no fallback: a missing shared object raises.

    Every loaded library carries its own ``lib.call`` (an engine keeps the one of the library it was built on); the
    module-level ``call`` is that of the library ``load()`` returns now."""

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
        bound = {}          # name -> (ctypes function, Signature) of THIS library
        for name, (restype, argtypes) in {**ns["SYMBOLS"], **ns.get("MORE_SYMBOLS", {})}.items():   # MORE_SYMBOLS: of a second header
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = restype
            fn.argtypes = [ctypes.c_void_p if isinstance(t, DevicePointer) else t for t in argtypes]
            bound[name] = (fn, Signature(argtypes))
        last_error = getattr(lib, prefix + "_last_error")

        def lib_call(name, device, *args):
            """``name(*args, stream)`` with ``device`` current, on its current stream (see ``marshal``); non-zero raises."""
            fn, sig = bound[name]
            current = torch.cuda.current_device()
            if device.index is None:
                device = torch.device(device.type, current)
            argv = marshal(name, sig, args, device, torch.cuda.current_stream(device).cuda_stream)
            if device.index == current:
                rc = fn(*argv)
            else:
                with torch.cuda.device(device):     # the C ABI takes a stream but launches on the CURRENT device
                    rc = fn(*argv)
            if rc != 0:
                msg = last_error()
                raise NativeError(f"{name} failed: {msg.decode() if msg else 'unknown error'}")

        lib.call = lib_call
        ns["_lib"] = lib
        return lib

    def check(rc, call):
        if rc != 0:
            msg = getattr(load(), prefix + "_last_error")()
            raise NativeError(f"{call} failed: {msg.decode() if msg else 'unknown error'}")

    def call(name, device, *args):
        load().call(name, device, *args)

    return load, check, call


def stream_handle(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def k_array(K):
    """A 3x3 intrinsic matrix (tensor or array-like) as the nine host doubles the C ABIs take."""
    k = np.ascontiguousarray(np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64)).reshape(9)
    return (ctypes.c_double * 9)(*k.tolist())


def gpu_tensor(t, dtype, refusal):
    """The one conversion in front of a native call: ``t`` as a contiguous ``dtype`` tensor on the GPU it is on.  A tensor
    that is not on one raises RuntimeError(``refusal`` with {} = where it is): there is no CPU path."""
    if not t.is_cuda:
        raise RuntimeError(refusal.format(t.device))
    return (t if t.dtype is dtype else t.to(dtype)).contiguous()


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


class Engine:
    """What the engines of the three network front ends share: the library, the packed weights of one module (and their
    cross-stream ordering: PackedWeights) and its workspaces (WorkspaceCache).  A subclass names its binding module
    (``native``), the library's workspace query, the refusal for a parameter that is not on a GPU, and provides
    ``_raw_tensors()`` (the live tensors the forward reads, in pack order) and ``_pack(copies)``."""

    native = None
    WORKSPACE_BYTES = None              # names of the library's workspace query and of its last-error function
    LAST_ERROR = None
    PARAMETER_REFUSAL = None
    MAX_CACHED_WORKSPACES = 6
    MAX_CACHED_WORKSPACE_BYTES = float("inf")

    def __init__(self, module):
        self.module = module
        self.lib = self.native.load()
        self.call = self.lib.call       # of this library, whatever the binding module loads later
        self._packed = PackedWeights(self.PARAMETER_REFUSAL)
        self._workspaces = WorkspaceCache(self.MAX_CACHED_WORKSPACES, self.MAX_CACHED_WORKSPACE_BYTES)

    def packed_weights(self, device):
        return self._packed.get(device, self._raw_tensors(), self._pack)

    def workspace(self, *shape_device):
        """The workspace of ``(*shape, device)`` on the device's current stream."""
        *shape, device = shape_device
        return self._workspaces.get(tuple(shape), device, getattr(self.lib, self.WORKSPACE_BYTES),
                                    lambda: self.workspace_refusal(shape))

    def workspace_refusal(self, shape):
        """The message when the library's workspace query returns 0."""
        return f"{self.WORKSPACE_BYTES}: " + getattr(self.lib, self.LAST_ERROR)().decode()
