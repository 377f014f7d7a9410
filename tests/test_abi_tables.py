"""The ctypes tables against the headers, for all six libraries, what ``bind()`` makes of them, and the marshalling step of
``_binding.call``.  No GPU: the libraries are loaded (and built first if they are stale) by one test, nothing is launched."""
import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_uint64, c_void_p

import pytest
import torch

from onepose_amd import _binding, _native, _native_det, _native_map, _native_pnp, _native_sg, _native_spp
from onepose_amd._binding import F32, F64, I32, I64, RAW, STREAM, U8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBRARIES = {   # prefix -> (header under include/, binding module)
    "gatsspg": ("gatsspg.h", _native), "spp": ("superpoint.h", _native_spp), "pnp": ("pnp.h", _native_pnp),
    "sg": (os.path.join("superglue", "superglue.h"), _native_sg), "det": (os.path.join("detector", "detector.h"), _native_det),
    "map": (os.path.join("mapping", "mapping.h"), _native_map),
}
SCALARS = {"int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t, "uint64_t": c_uint64}
# element type -> what a table may say: the device marker, or the ctypes pointer of a HOST array (the C type cannot tell which)
ELEMENTS = {"float": (F32, POINTER(c_float)), "double": (F64, POINTER(c_double)), "int32_t": (I32, POINTER(c_int32)),
            "int64_t": (I64, POINTER(c_int64)), "uint8_t": (U8, POINTER(c_uint8))}
STRUCTS = {"gatsspg_raw_weights": _native.RawWeights, "gatsspg_kenc_weights": _native.KencWeights,
           "spp_raw_weights": _native_spp.RawWeights}
RETURNS = {"int": c_int, "size_t": c_size_t, "char*": c_char_p}
CPU = torch.device("cpu")


def prototypes(prefix):
    """{name: (return type, [(type without const, stars, parameter name)])} of every function a header declares."""
    with open(os.path.join(ROOT, "include", LIBRARIES[prefix][0])) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(%s_\w+)\s*\(([^()]*)\)\s*;" % prefix, text):
        plist = []
        for p in (q.strip() for q in params.split(",")):
            if p == "void":
                continue
            words = re.findall(r"\w+|\*", p)
            pname = words.pop()
            words = [w for w in words if w != "const"]
            plist.append((" ".join(w for w in words if w != "*"), words.count("*"), pname))
        assert name not in out, f"{name} declared twice"
        out[name] = ("".join(w for w in ret.split() if w != "const"), plist)
    return out


def allowed(ctype, stars, pname):
    """What the table may hold for one C parameter."""
    if ctype.endswith("_stream_t") or (ctype, stars, pname) == ("void", 1, "stream"):
        return (STREAM,)
    if ctype.endswith("_event_t") or (ctype, stars, pname[:3]) == ("void", 1, "ev_"):
        return (c_void_p,)                      # a hipEvent_t handle (the matcher's header passes it as void* ev_start / ev_stop)
    if stars == 0:
        return (SCALARS[ctype],)
    if stars == 2:
        return (RAW, POINTER(c_void_p))         # an array of device pointers: on the device, or on the host
    if ctype == "void":
        return (RAW,)
    if ctype in STRUCTS:
        return (POINTER(STRUCTS[ctype]),)
    return ELEMENTS[ctype]


@pytest.mark.parametrize("prefix", sorted(LIBRARIES))
def test_table_mirrors_the_header(prefix):
    """Same names, same arity, and parameter by parameter the same kind.  Host and device pointers cannot be told apart from
    the C type: a pointer to float may be F32 or POINTER(c_float), nothing else."""
    symbols = LIBRARIES[prefix][1].SYMBOLS
    protos = prototypes(prefix)
    assert len(protos) >= 6 and set(protos) == set(symbols), "ctypes binding table out of sync with the header"
    for name, (ret, params) in protos.items():
        restype, table = symbols[name]
        assert restype is RETURNS[ret], f"{name}: returns {ret}, the table says {restype}"
        assert len(table) == len(params), f"{name}: {len(params)} parameters in the header, {len(table)} in the table"
        for i, ((ctype, stars, pname), entry) in enumerate(zip(params, table)):
            assert any(entry is a for a in allowed(ctype, stars, pname)), \
                f"{name} parameter {i} ({ctype}{'*' * stars} {pname}): the table says {entry!r}"


def test_the_header_parser_reads_what_it_should():
    p = prototypes("det")["det_crop_resize"][1]
    assert [x[:2] for x in p[:5]] == [("uint8_t", 1), ("int", 0), ("int", 0), ("int32_t", 1), ("double", 1)] and p[4][2] == "K_host"
    assert prototypes("map")["map_gather_descriptors"][1][0] == ("float", 2, "desc_table")
    assert prototypes("gatsspg")["gatsspg_version"] == ("int", []) and prototypes("sg")["sg_last_error"][0] == "char*"
    assert len(prototypes("gatsspg")["gatsspg_forward_profiled"][1]) == 23


def test_bind_lowers_the_markers_to_void_pointers():
    """A raw lib.fn(...) call sees plain ctypes: every marker becomes c_void_p, everything else stays what the table says."""
    from onepose_amd import build_ext
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    for prefix, (_, mod) in LIBRARIES.items():
        lib = mod.load()
        for name, (restype, table) in mod.SYMBOLS.items():
            fn = getattr(lib, name)
            assert fn.restype is restype and len(fn.argtypes) == len(table)
            for got, entry in zip(fn.argtypes, table):
                assert got is (c_void_p if isinstance(entry, _binding.DevicePointer) else entry)
            assert getattr(fn, "errcheck", None) is None


def test_build_table_lists_the_headers_the_sources_include():
    """Every library's ``headers`` are exactly the project headers its sources reach through ``#include "..."``, directly or
    through another header: an entry that is missing would let a change to that header go without a rebuild."""
    from onepose_amd import build_ext

    def reach(path, seen):
        with open(path) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), flags=re.M):
                target = os.path.normpath(os.path.join(os.path.dirname(path), inc))
                assert os.path.isfile(target), f"{path} includes {inc}, which is not there"
                if target not in seen:
                    seen.add(target)
                    reach(target, seen)
        return seen

    assert len(build_ext.LIBRARIES) == 6
    for lib in build_ext.LIBRARIES:
        reached = set()
        for s in lib.sources:
            reach(os.path.join(build_ext.CSRC, s), reached)
        listed = {os.path.normpath(os.path.join(build_ext.CSRC, h)) for h in lib.headers}
        assert len(listed) == len(lib.headers) and reached == listed, \
            f"{os.path.basename(lib.path)}: not listed {sorted(reached - listed)}, listed but not included {sorted(listed - reached)}"


def test_every_loaded_library_has_its_own_call(monkeypatch):
    """An engine keeps ``lib.call`` of the library it was built on: re-binding the module (``_lib = None``, as the A/B tools do
    after assigning LIB_PATH) gives the new library a call table of its own and leaves the old one alone."""
    from onepose_amd import build_ext
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    first = _native_pnp.load()
    monkeypatch.setattr(_native_pnp, "_lib", None)
    second = _native_pnp.load()
    assert second is not first and second.call is not first.call and _native_pnp.load() is second


# ---- marshalling: CPU tensors, device = cpu ----
PARAMS = [F32, c_int, I64, RAW, POINTER(c_int32), STREAM]


def marshal(*args, params=PARAMS):
    return _binding.marshal("fn", _binding.Signature(params), args, CPU, 0x5EED)


def test_marshal_passes_good_tensors_and_fills_the_stream():
    x, m, ws = torch.zeros(3, 2), torch.zeros(4, dtype=torch.int64), torch.zeros(7, dtype=torch.uint8)
    host = (ctypes.c_int32 * 2)(1, 2)
    assert marshal(x, 5, m, ws, host) == [x.data_ptr(), 5, m.data_ptr(), ws.data_ptr(), host, 0x5EED]
    assert marshal(None, 5, None, None, host)[:4] == [None, 5, None, None]                  # None -> NULL
    for any_dtype in (torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int16), x):
        assert marshal(x, 5, m, any_dtype, host)[3] == any_dtype.data_ptr()                 # RAW takes any dtype
    assert marshal(x, params=[STREAM, F32, STREAM]) == [0x5EED, x.data_ptr(), 0x5EED]
    assert marshal(x, 7, params=[F32, STREAM, c_int]) == [x.data_ptr(), 0x5EED, 7]       # a stream in the middle (spp_forward)


@pytest.mark.parametrize("bad,position", [
    (lambda x, m: (x, 5, m.to(torch.int32)), 2),                    # int32 where the kernel stores int64
    (lambda x, m: (x[:, 0], 5, m), 0),                              # a strided column view
    (lambda x, m: (x.double(), 5, m), 0),
    (lambda x, m: (torch.empty(3, 2, device="meta"), 5, m), 0),     # a tensor on another device
    (lambda x, m: (x.data_ptr(), 5, m), 0),                         # an address is not a tensor
])
def test_marshal_refuses_bad_tensors(bad, position):
    x, m = torch.zeros(3, 2), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError, match=f"fn argument {position}:"):
        marshal(*bad(x, m), None, None)


def test_marshal_refuses_a_wrong_argument_count():
    x, m = torch.zeros(3, 2), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError, match="fn takes 5 arguments"):
        marshal(x, 5, m, None)
    with pytest.raises(TypeError, match="fn takes 5 arguments"):
        marshal(x, 5, m, None, None, 0x5EED)                        # the stream is filled, not passed


def test_gpu_tensor_refuses_the_host_with_the_modules_message():
    with pytest.raises(RuntimeError, match=r"module X \(on cpu\); there is no CPU fallback"):
        _binding.gpu_tensor(torch.zeros(2), torch.float32, "module X (on {}); there is no CPU fallback")
