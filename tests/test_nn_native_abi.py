"""C ABI of the nearest-neighbour matcher (include/superglue/nn_matcher.h, part of libsuperglue_hip.so): every prototype is exported
and bound, the ctypes table mirrors the header parameter by parameter, and the host-side refusals return their codes with text --
all without a GPU: every argument is validated before the first launch."""
import ctypes
import os
import re
from ctypes import POINTER, c_double, c_int, c_int32, c_size_t

import pytest

import nn_cases
from onepose_amd import _native_sg, build_ext
from onepose_amd._binding import F32, I64, RAW, STREAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "superglue", "nn_matcher.h")
SCALARS = {"int": c_int, "double": c_double, "size_t": c_size_t}
POINTERS = {"float": (F32,), "int64_t": (I64,), "int32_t": (POINTER(c_int32),), "void": (RAW,)}     # int32_t*: the HOST count arrays
RETURNS = {"int": c_int, "size_t": c_size_t}


def prototypes():
    """{name: (return type, [(type without const, stars, parameter name)])} of every function the header declares."""
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(nnm_\w+)\s*\(([^()]*)\)\s*;", text):
        plist = []
        for p in (q.strip() for q in params.split(",")):
            words = [w for w in re.findall(r"\w+|\*", p) if w != "const"]
            pname = words.pop()
            plist.append((" ".join(w for w in words if w != "*"), words.count("*"), pname))
        out[name] = (ret.strip(), plist)
    return out


@pytest.fixture(scope="module")
def lib():
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    return _native_sg.load()


def test_every_prototype_is_exported_and_bound(lib):
    protos = prototypes()
    assert set(protos) == {"nnm_workspace_bytes", "nnm_match", "nnm_match_ragged", "nnm_similarity"} == set(_native_sg.MORE_SYMBOLS)
    raw = ctypes.CDLL(_native_sg.LIB_PATH)
    for name in protos:
        assert hasattr(raw, name) and getattr(lib, name).restype is _native_sg.MORE_SYMBOLS[name][0], name
    assert not set(_native_sg.MORE_SYMBOLS) & set(_native_sg.SYMBOLS)


def test_more_symbols_mirrors_the_header():
    for name, (ret, params) in prototypes().items():
        restype, table = _native_sg.MORE_SYMBOLS[name]
        assert restype is RETURNS[ret], name
        assert len(table) == len(params), f"{name}: {len(params)} parameters in the header, {len(table)} in the table"
        for i, ((ctype, stars, pname), entry) in enumerate(zip(params, table)):
            allowed = (STREAM,) if ctype == "sg_stream_t" else (SCALARS[ctype],) if stars == 0 else POINTERS[ctype]
            assert any(entry is a for a in allowed), f"{name} parameter {i} ({ctype}{'*' * stars} {pname}): the table says {entry!r}"


def test_constants_and_build_table():
    with open(HEADER) as f:
        text = f.read()
    defs = dict(re.findall(r"#define (NNM_\w+) (\d+)", text))
    assert int(defs["NNM_MAX_ITEMS"]) == _native_sg.NNM_MAX_ITEMS == 64
    assert (int(defs["NNM_TILE_ROWS"]), int(defs["NNM_TILE_COLS"])) == _native_sg.NNM_TILE == (nn_cases.BM, nn_cases.BN)
    assert os.path.join("superglue", "nn_matcher.hip") in build_ext.SG_SOURCES and len(build_ext.LIBRARIES) == 6
    assert any(h.endswith(os.path.join("superglue", "nn_matcher.h")) for h in build_ext.SG_HEADERS)
    assert all(os.path.exists(os.path.join(build_ext.CSRC, d)) for d in build_ext.SG_SOURCES + build_ext.SG_HEADERS)


def test_host_side_checks(lib):
    assert lib.sg_version() >= 3
    assert lib.nnm_workspace_bytes(0, 5, 5) == 0 and lib.nnm_workspace_bytes(1, 0, 5) == 0 and lib.nnm_workspace_bytes(65, 5, 5) == 0
    # planes [256][128] and [256][64], one float4 partial per row and per column
    assert lib.nnm_workspace_bytes(1, 5, 5) == 4 * 256 * 128 + 4 * 256 * 64 + 2 * 256
    up = lambda x: (x + 255) // 256 * 256       # noqa: E731  (every piece starts on a multiple of 256 bytes)
    assert lib.nnm_workspace_bytes(3, 129, 65) == 3 * (4 * 256 * 256 + 4 * 256 * 128) + up(3 * 16 * 129 * 2) + up(3 * 16 * 65 * 2)
    err = lambda: lib.sg_last_error()       # noqa: E731
    big = lib.nnm_workspace_bytes(2, 8, 8)
    ws = ctypes.create_string_buffer(big + 256)
    base = (ctypes.addressof(ws) + 255) // 256 * 256
    buf = ctypes.create_string_buffer(1 << 16)
    p = [ctypes.addressof(buf) + 4096 * i for i in range(6)]        # desc0, desc1, matches0, matches1, scores0, scores1
    tail = (base, big, None, 0)

    def match(b=2, n0=8, n1=8, ratio=0.0, distance=0.0, ptrs=p, tail=tail):
        return lib.nnm_match(ptrs[0], ptrs[1], b, n0, n1, ratio, distance, 1, *ptrs[2:], *tail)

    assert match(n0=0) == -1 and b"n0" in err()
    assert match(b=0) == -1 and b"b must" in err()
    assert match(b=65) == -1 and b"b must" in err()
    assert match(n0=1, ratio=0.8) == -1 and b"second neighbour" in err()
    assert match(n1=1, ratio=0.8) == -1 and b"second neighbour" in err()
    assert match(ratio=-0.5) == -1 and b"thresholds" in err()
    assert match(distance=float("nan")) == -1 and b"thresholds" in err()
    assert match(tail=(base, big - 1, None, 0)) == -2 and b"workspace too small" in err()
    assert match(tail=(None, big, None, 0)) == -1 and b"workspace is null" in err()
    assert match(tail=(base, big, None, 1)) == -1 and b"flags" in err()
    assert match(ptrs=p[:3] + [p[2]] + p[4:]) == -1 and b"alias" in err()             # matches1 is matches0
    assert match(ptrs=p[:4] + [p[3] + 8, p[5]]) == -1 and b"alias" in err()           # scores0 inside matches1
    assert match(ptrs=[p[2]] + p[1:]) == -1 and b"alias" in err()                     # matches0 is desc0
    assert match(ptrs=p[:5] + [base + 64]) == -1 and b"alias" in err()                # scores1 inside the workspace
    assert match(ptrs=[None] + p[1:]) == -1 and b"null" in err()
    n_ok, n_bad = (c_int32 * 2)(8, 3), (c_int32 * 2)(8, 9)

    def ragged(n0=n_ok, n1=n_ok, ratio=0.0, shared1=0, flags=0):
        return lib.nnm_match_ragged(p[0], p[1], n0, n1, 2, 8, 8, shared1, ratio, 0.0, 1, *p[2:], base, big, None, flags)

    assert ragged(n0=n_bad) == -1 and b"item 1: n0 = 9" in err()
    assert ragged(n1=None) == -1 and b"host arrays" in err()
    assert ragged(n1=(c_int32 * 2)(8, 1), ratio=0.8) == -1 and b"item 1" in err() and b"second neighbour" in err()
    assert ragged(flags=4) == -1 and b"flags" in err()
    assert lib.nnm_similarity(p[0], p[1], 8, 0, p[2], base, big, None, 0) == -1 and b"n1" in err()
    assert lib.nnm_similarity(p[0], p[1], 8, 8, p[0], base, big, None, 0) == -1 and b"alias" in err()
    assert lib.nnm_similarity(p[0], p[1], 8, 8, p[2], base, 16, None, 0) == -2 and b"workspace" in err()


def test_sources_stay_in_the_superglue_subdirectories():
    """source_hash() (top-level files only) does not move with the new sources."""
    assert os.path.exists(os.path.join(build_ext.CSRC, "superglue", "nn_matcher.hip")) and os.path.exists(HEADER)
    assert not [n for n in os.listdir(build_ext.CSRC) + os.listdir(os.path.join(ROOT, "include")) if "nn_matcher" in n]
