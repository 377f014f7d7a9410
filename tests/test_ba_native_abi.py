"""C ABI of the bundle adjustment in libmap_hip.so: every symbol of include/mapping/bundle_adjust.h is exported and listed in
_native_map.MORE_SYMBOLS, the header's constants are the binding's, and the host-side refusals carry text."""
import ctypes
import os
import re

import pytest

from onepose_amd import _native_map, build_ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mapping", "bundle_adjust.h")
NAMES = ["ba_workspace_bytes", "ba_solve", "ba_linearize", "ba_normal_blocks", "ba_step"]


def header_text():
    with open(HEADER) as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    return _native_map.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ba_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(NAMES)
    raw = ctypes.CDLL(_native_map.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), n
    assert set(names) == set(_native_map.MORE_SYMBOLS)
    assert not set(_native_map.MORE_SYMBOLS) & set(_native_map.SYMBOLS)


def test_library_version_and_sources():
    assert _native_map.load().map_version() >= 2
    assert len(build_ext.LIBRARIES) == 6
    assert os.path.join("mapping", "bundle_adjust.hip") in build_ext.MAP_SOURCES
    assert all(s.startswith("mapping" + os.sep) for s in build_ext.MAP_SOURCES)
    with open(os.path.join(build_ext.CSRC, "mapping", "bundle_adjust.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd" not in src


def test_header_constants_match_the_binding_and_the_cases():
    import ba_cases
    import ba_oracle
    consts = {k: int(v) for k, v in re.findall(r"#define (BA_[A-Z_]+) (\d+)", header_text())}
    assert consts["BA_MAX_CAMERAS"] == _native_map.BA_MAX_CAMERAS == 32
    assert consts["BA_MAX_POINTS"] == _native_map.BA_MAX_POINTS == 32768
    assert consts["BA_MAX_OBSERVATIONS"] == _native_map.BA_MAX_OBSERVATIONS == 262144
    assert consts["BA_MAX_ITERATIONS"] == _native_map.BA_MAX_ITERATIONS
    assert consts["BA_CAMERA_CHUNK"] == _native_map.BA_CAMERA_CHUNK == ba_cases.CAMERA_CHUNK
    assert consts["BA_TRACE_COLUMNS"] == _native_map.BA_TRACE_COLUMNS == 6
    assert consts["BA_SUMMARY_ENTRIES"] == _native_map.BA_SUMMARY_ENTRIES == 6
    assert consts["BA_STATUS_OK"] == _native_map.BA_STATUS_OK == ba_oracle.STATUS_OK
    assert consts["BA_STATUS_NONFINITE_START"] == _native_map.BA_STATUS_NONFINITE_START == ba_oracle.STATUS_NONFINITE_START


def test_host_side_refusals_carry_text(lib):
    err = lib.map_last_error
    assert lib.ba_workspace_bytes(33, 10, 10) == 0 and b"C in [1, 32]" in err()
    assert lib.ba_workspace_bytes(0, 10, 10) == 0 and lib.ba_workspace_bytes(-1, 10, 10) == 0
    assert lib.ba_workspace_bytes(3, -5, 10) == 0 and lib.ba_workspace_bytes(3, 10, -1) == 0 and b"expected" in err()
    assert lib.ba_workspace_bytes(3, _native_map.BA_MAX_POINTS + 1, 10) == 0
    assert lib.ba_workspace_bytes(3, 10, _native_map.BA_MAX_OBSERVATIONS + 1) == 0
    need = lib.ba_workspace_bytes(32, 100, 1000)
    assert need > 0 and lib.ba_workspace_bytes(32, _native_map.BA_MAX_POINTS, _native_map.BA_MAX_OBSERVATIONS) > need
    buf = ctypes.create_string_buffer(1024)
    p = (ctypes.addressof(buf) + 255) // 256 * 256          # host memory: nothing is launched by a refused call
    big = 1 << 40

    def solve(C=3, P=10, M=20, it=5, succ=5, ws=p, ws_bytes=big, cams=p, trace=p):
        return lib.ba_solve(cams, p, p, p, p, p, None, None, C, P, M, it, succ, trace, p, ws, ws_bytes, None)

    assert solve(C=33) == -1 and b"C in [1, 32]" in err()
    assert solve(P=-1) == -1 and solve(M=-3) == -1 and solve(M=0) == -1 and b"expected" in err()
    assert solve(cams=None) == -1 and b"null" in err()
    assert solve(trace=None) == -1 and b"null" in err()
    assert solve(it=0) == -1 and b"num_iterations" in err()
    assert solve(it=_native_map.BA_MAX_ITERATIONS + 1) == -1 and solve(succ=0) == -1 and b"num_success_iterations" in err()
    assert solve(ws=None) == -1 and b"null workspace" in err()
    assert solve(ws=p + 8) == -1 and b"aligned" in err()
    assert solve(ws_bytes=64) == -2 and b"workspace too small" in err()

    assert lib.ba_linearize(p, p, p, p, p, p, 33, 10, 20, p, p, p, None) == -1 and b"C in [1, 32]" in err()
    assert lib.ba_linearize(p, p, p, p, p, p, 3, 10, 20, None, p, p, None) == -1 and b"null" in err()
    blocks = lambda C, ws_bytes, U=p: lib.ba_normal_blocks(p, p, p, p, p, None, None, C, 10, 20, U, p, p, p, p, p, ws_bytes, None)  # noqa: E731
    assert blocks(33, big) == -1 and b"C in [1, 32]" in err()
    assert blocks(3, 64) == -2 and b"workspace too small" in err()
    assert blocks(3, big, None) == -1 and b"null" in err()
    step = lambda C, mu, ws_bytes: lib.ba_step(p, p, p, p, p, p, p, p, p, None, None, C, 10, 20, mu, p, p, p, p, ws_bytes, None)  # noqa: E731
    assert step(33, 1.0, big) == -1 and b"C in [1, 32]" in err()
    assert step(3, 0.0, big) == -1 and b"mu" in err()
    assert step(3, float("nan"), big) == -1 and b"mu" in err()
    assert step(3, 1.0, 64) == -2 and b"workspace too small" in err()
