"""C ABI of the matcher's training head in libgatsspg_hip.so: the ``gtr_`` table of _native_train against include/gatsspg_train.h
(the parser of tests/test_abi_tables.py, restated) and the exports; the header's constants; host-side refusals (host pointers are
passed, so nothing is launched).  No GPU."""
import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t

import pytest

from onepose_amd import _binding, _native, _native_train, build_ext
from onepose_amd._binding import F32, F64, I32, I64, RAW, STREAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gatsspg_train.h")
NAMES = ["gtr_version", "gtr_last_error", "gtr_workspace_bytes", "gtr_build_target", "gtr_loss_head", "gtr_scores_exp", "gtr_loss_terms",
         "gtr_score_grad"]
SCALARS = {"int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t}
ELEMENTS = {"float": (F32, POINTER(c_float)), "double": (F64, POINTER(c_double)), "int32_t": (I32, POINTER(c_int32)),
            "int64_t": (I64, POINTER(c_int64)), "int8_t": (_native_train.I8,)}
RETURNS = {"int": c_int, "size_t": c_size_t, "char*": c_char_p}


def header_text():
    with open(HEADER) as f:
        return f.read()


def prototypes():
    """{name: (return type, [(type without const, stars, parameter name)])} of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(gtr_\w+)\s*\(([^()]*)\)\s*;", text):
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
    if (ctype, stars, pname) == ("void", 1, "stream"):
        return (STREAM,)
    if stars == 0:
        return (SCALARS[ctype],)
    if ctype == "void":
        return (RAW,)
    return ELEMENTS[ctype]


@pytest.fixture(scope="module")
def lib():
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    return _native_train.load()


def test_table_mirrors_the_header():
    protos = prototypes()
    assert sorted(protos) == sorted(NAMES) == sorted(_native_train.SYMBOLS)
    for name, (ret, params) in protos.items():
        restype, table = _native_train.SYMBOLS[name]
        assert restype is RETURNS[ret], f"{name}: returns {ret}, the table says {restype}"
        assert len(table) == len(params), f"{name}: {len(params)} parameters in the header, {len(table)} in the table"
        for i, ((ctype, stars, pname), entry) in enumerate(zip(params, table)):
            assert any(entry is a for a in allowed(ctype, stars, pname)), f"{name} parameter {i} ({ctype}{'*' * stars} {pname}): {entry!r}"
    assert len(protos["gtr_loss_head"][1]) == 18 and protos["gtr_last_error"][0] == "char*"
    assert protos["gtr_build_target"][1][1] == ("int32_t", 1, "k") and _native_train.SYMBOLS["gtr_build_target"][1][1] is POINTER(c_int32)


def test_every_declared_symbol_is_exported_and_bound(lib):
    raw = ctypes.CDLL(_native_train.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    for name, (restype, table) in _native_train.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and len(fn.argtypes) == len(table)
        for got, entry in zip(fn.argtypes, table):
            assert got is (ctypes.c_void_p if isinstance(entry, _binding.DevicePointer) else entry)
    assert not any(n.startswith("gtr_") for n in _native.SYMBOLS)


def test_library_version_and_sources(lib):
    assert lib.gtr_version() == 1 and _native.load().gatsspg_version() >= 411
    assert _native_train.LIB_PATH == build_ext.LIB_PATH and len(build_ext.LIBRARIES) == 6
    assert "gatsspg_train_kernels.hip" in build_ext.SOURCES
    assert any(h.endswith("gatsspg_train.h") for h in build_ext.LIBRARIES[0].headers)
    with open(os.path.join(build_ext.CSRC, "gatsspg_train_kernels.hip")) as f:
        src = f.read()
    assert "atomicAdd" not in src and "__hip_atomic" not in src and "hipMalloc" not in src and "Synchronize" not in src


def test_header_constants_match_the_binding_and_the_oracle():
    import train_oracle
    consts = {k: int(v) for k, v in re.findall(r"#define (GTR_[A-Z_]+) (\d+)", header_text())}
    assert consts["GTR_DESC_DIM"] == _native_train.DESC_DIM == 256
    assert consts["GTR_MAX_BATCH"] == _native_train.MAX_BATCH == 64
    assert consts["GTR_MAX_POINTS"] == _native_train.MAX_POINTS == 1 << 22
    assert consts["GTR_MAX_ELEMENTS"] == _native_train.MAX_ELEMENTS == 1 << 26
    assert (consts["GTR_CLASS_NEGATIVE"], consts["GTR_CLASS_POSITIVE"], consts["GTR_CLASS_IGNORED"]) == (0, 1, 2) \
        == (_native_train.CLASS_NEGATIVE, _native_train.CLASS_POSITIVE, _native_train.CLASS_IGNORED) \
        == (train_oracle.NEGATIVE, train_oracle.POSITIVE, train_oracle.IGNORED)


def test_workspace_refusals(lib):
    err = lib.gtr_last_error
    assert lib.gtr_workspace_bytes(0, 10, 10) == 0 and b"b must be in [1, 64]" in err()
    assert lib.gtr_workspace_bytes(65, 10, 10) == 0 and b"b must be in [1, 64]" in err()
    assert lib.gtr_workspace_bytes(1, 0, 10) == 0 and b"n, m must be >= 1" in err()
    assert lib.gtr_workspace_bytes(1, 10, -3) == 0 and b"n, m must be >= 1" in err()
    assert lib.gtr_workspace_bytes(1, 8193, 8192) == 0 and b"n * m must be <=" in err()
    assert lib.gtr_workspace_bytes(1, (1 << 22) + 1, 1) == 0 and b"points per side" in err()
    one = lib.gtr_workspace_bytes(1, 1, 1)
    train = lib.gtr_workspace_bytes(8, 1000, 2000)
    assert 0 < one < train and one % 256 == 0 and train % 256 == 0
    assert lib.gtr_workspace_bytes(1, 8192, 8192) > 0 and lib.gtr_workspace_bytes(64, 1, 1) > one
    e_bytes = 8 * 1024 * 2048 * 4                       # E, padded to the 128 x 64 tile, is the bulk of it (+ three operand planes: 40 MB)
    assert e_bytes < train < 1.8 * e_bytes


def test_loss_head_refusals(lib):
    err = lib.gtr_last_error
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 255) // 256 * 256      # host memory: nothing is launched by a refused call
    huge = 1 << 40

    def head(b=2, n=10, m=12, alpha=0.5, gamma=2.0, pos_w=0.5, neg_w=0.5, scale=0.07, x=p, cls=p, loss=p, counts=p, dx=p, dy=p, ws=p,
             ws_bytes=huge):
        return lib.gtr_loss_head(x, p, cls, b, n, m, alpha, gamma, pos_w, neg_w, scale, loss, counts, dx, dy, ws, ws_bytes, None)

    assert head(b=0) == -1 and b"b must be in" in err()
    assert head(n=0) == -1 and head(m=0) == -1 and b"n, m must be >= 1" in err()
    assert head(n=1 << 14, m=1 << 13) == -1 and b"n * m" in err()
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan"))):
        assert head(**kw) == -1 and b"alpha" in err(), kw
    for kw in (dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("inf")), dict(gamma=float("nan"))):
        assert head(**kw) == -1 and b"gamma" in err(), kw
    for kw in (dict(pos_w=-1.0), dict(neg_w=float("nan")), dict(neg_w=float("inf"))):
        assert head(**kw) == -1 and b"pos_w and neg_w" in err(), kw
    for kw in (dict(scale=0.0), dict(scale=0.01), dict(scale=float("nan")), dict(scale=float("inf"))):
        assert head(**kw) == -1 and b"scale" in err() and b"1/80" in err(), kw
    assert head(ws=None) == -1 and b"workspace is null" in err()
    assert head(ws=p + 16) == -1 and b"aligned" in err()
    assert head(ws_bytes=1024) == -2 and b"workspace too small" in err()
    for kw in (dict(x=None), dict(cls=None), dict(loss=None), dict(counts=None)):
        assert head(**kw) == -1 and b"null" in err(), kw
    assert head(dx=None) == -1 and b"both" in err() and head(dy=None) == -1 and b"both" in err()
    assert head(x=p + 2) == -1 and b"misaligned" in err()
    assert head(counts=p + 4) == -1 and b"misaligned" in err()

    # the stage entries and the target builder refuse alike
    assert lib.gtr_scores_exp(p, p, 1, 10, 10, 0.001, p, p, p, p, huge, None) == -1 and b"scale" in err()
    assert lib.gtr_scores_exp(p, p, 1, 10, 10, 0.07, None, p, p, p, huge, None) == -1 and b"null" in err()
    assert lib.gtr_loss_terms(p, p, p, p, 1, 10, 10, 0.5, 2.0, 0.5, 0.5, None, p, p, p, p, p, huge, None) == -1 and b"null" in err()
    assert lib.gtr_score_grad(p, p, p, p, p, p, p, 1, 10, 10, 0.5, 2.0, 0.5, 0.5, p, p, 16, None) == -2 and b"too small" in err()
    k = (ctypes.c_int32 * 2)(3, 9)
    no = (ctypes.c_int32 * 2)(5, 5)
    assert lib.gtr_build_target(p, k, no, no, 2, 8, 10, 10, 1, p, None, None) == -1 and b"k = 9 is outside [0, kcap = 8]" in err()
    assert lib.gtr_build_target(p, None, no, no, 2, 8, 10, 10, 1, p, None, None) == -1 and b"host arrays" in err()
    assert lib.gtr_build_target(p, k, no, no, 2, 16, 10, 10, 1, None, None, None) == -1 and b"null" in err()


def test_the_product_library_does_not_import_getenv(lib):
    import subprocess
    syms = subprocess.run(["nm", "-D", "--undefined-only", build_ext.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in syms
    defined = subprocess.run(["nm", "-D", "--defined-only", build_ext.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(gtr_\w+)", defined))) == sorted(NAMES)
