"""C ABI of the tracker's map update step in libmap_hip.so: every symbol of include/mapping/track_update.h is exported and
listed in _native_trk.SYMBOLS, the header's constants are the binding's and the oracle's, and the host-side refusals carry
text (host pointers are passed, so nothing is launched)."""
import ctypes
import os
import re

import pytest

from onepose_amd import _native_map, _native_trk, build_ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mapping", "track_update.h")
NAMES = ["trk_workspace_bytes", "trk_update", "trk_triangulate_pairs", "trk_gate_median"]


def header_text():
    with open(HEADER) as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    return _native_trk.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(trk_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(NAMES)
    raw = ctypes.CDLL(_native_trk.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), n
    assert set(names) == {n for n in _native_trk.SYMBOLS if n.startswith("trk_")}
    assert set(_native_trk.SYMBOLS) - set(names) == {"map_version", "map_last_error"}
    assert not any(n.startswith("trk_") for n in {**_native_map.SYMBOLS, **_native_map.MORE_SYMBOLS})


def test_library_version_and_sources(lib):
    assert lib.map_version() >= 3
    assert _native_trk.LIB_PATH == build_ext.MAP_LIB_PATH and len(build_ext.LIBRARIES) == 6
    assert os.path.join("mapping", "track_update.hip") in build_ext.MAP_SOURCES
    assert any(h.endswith(os.path.join("mapping", "track_update.h")) for h in build_ext.MAP_HEADERS)
    assert all(s.startswith("mapping" + os.sep) for s in build_ext.MAP_SOURCES)
    with open(os.path.join(build_ext.CSRC, "mapping", "track_update.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd" not in src


def test_header_constants_match_the_binding_and_the_oracle():
    import track_oracle
    consts = {k: int(v) for k, v in re.findall(r"#define (TRK_[A-Z_]+) (\d+)", header_text())}
    assert consts["TRK_MAX_KEYPOINTS"] == _native_trk.MAX_KEYPOINTS == track_oracle.MAX_KEYPOINTS == 8192
    assert consts["TRK_SUMMARY_ENTRIES"] == _native_trk.SUMMARY_ENTRIES == track_oracle.SUMMARY_ENTRIES == 8


def test_host_side_refusals_carry_text(lib):
    err = lib.map_last_error
    big = _native_trk.MAX_KEYPOINTS
    assert lib.trk_workspace_bytes(0, 10) == 0 and b"n_kf and n_q in [1, 8192]" in err()
    assert lib.trk_workspace_bytes(10, 0) == 0 and lib.trk_workspace_bytes(-1, 10) == 0 and lib.trk_workspace_bytes(10, big + 1) == 0
    assert lib.trk_workspace_bytes(big + 1, 10) == 0 and b"expected" in err()
    need = lib.trk_workspace_bytes(100, 120)
    assert need > 0 and need % 256 == 0 and lib.trk_workspace_bytes(big, big) > need
    buf = ctypes.create_string_buffer(1024)
    p = (ctypes.addressof(buf) + 255) // 256 * 256          # host memory: nothing is launched by a refused call
    huge = 1 << 40

    def update(n_kf=10, n_q=12, n_points=5, gate=1.2, reproj=20.0, z=0.15, ws=p, ws_bytes=huge, matches0=p, points=p, summary=p):
        return lib.trk_update(matches0, p, p, p, points, p, p, p, p, n_kf, n_q, n_points, gate, reproj, z, p, p, p, p, p, p, p, summary,
                              ws, ws_bytes, None)

    assert update(n_kf=0) == -1 and b"n_kf and n_q in [1, 8192]" in err()
    assert update(n_q=big + 1) == -1 and update(n_kf=-4) == -1 and b"expected" in err()
    assert update(n_points=-1) == -1 and b"n_points" in err()
    assert update(matches0=None) == -1 and b"null" in err()
    assert update(summary=None) == -1 and b"null" in err()
    assert update(points=None) == -1 and b"null points" in err()
    for kw in (dict(gate=0.0), dict(gate=float("nan")), dict(reproj=-1.0), dict(reproj=float("inf")), dict(z=0.0), dict(z=float("nan"))):
        assert update(**kw) == -1 and b"finite and positive" in err(), kw
    assert update(ws=None) == -1 and b"null workspace" in err()
    assert update(ws=p + 8) == -1 and b"aligned" in err()
    assert update(ws_bytes=64) == -2 and b"workspace too small" in err()

    assert lib.trk_triangulate_pairs(p, p, p, p, 0, p, None) == -1 and b"n >= 1" in err()
    assert lib.trk_triangulate_pairs(None, p, p, p, 4, p, None) == -1 and b"null" in err()
    assert lib.trk_triangulate_pairs(p, p, p, p, 4, None, None) == -1 and b"null" in err()

    gate = lambda n=10, factor=1.2, dist=p, ws=p, ws_bytes=huge: lib.trk_gate_median(dist, n, factor, p, p, ws, ws_bytes, None)  # noqa: E731
    assert gate(n=0) == -1 and gate(n=big + 1) == -1 and b"n in [1, 8192]" in err()
    assert gate(dist=None) == -1 and b"null" in err()
    assert gate(factor=0.0) == -1 and gate(factor=float("nan")) == -1 and b"finite and positive" in err()
    assert gate(ws=None) == -1 and b"null workspace" in err()
    assert gate(ws_bytes=8) == -2 and b"workspace too small" in err()
