"""C ABI of libdet_hip.so: every header symbol is exported and bound; the library is built from its own subdirectories and
leaves build_ext.source_hash() alone."""
import ctypes
import os
import re

import pytest

from onepose_amd import _native_det, build_ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "detector", "detector.h")


def header_functions():
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(det_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    return _native_det.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = header_functions()
    assert names == sorted(["det_version", "det_last_error", "det_workspace_bytes", "det_affine_partial_ransac",
                            "det_affine_partial_from_matches", "det_bbox_vote", "det_crop_resize"])
    raw = ctypes.CDLL(_native_det.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), n
    assert set(names) == set(_native_det.SYMBOLS)


def test_header_constants_match_the_binding():
    with open(HEADER) as f:
        text = f.read()
    consts = dict(re.findall(r"#define (DET_[A-Z_]+) (\d+)", text))
    assert int(consts["DET_RANK_BY_MATCHES"]) == _native_det.RANK_BY["matches"]
    assert int(consts["DET_RANK_BY_INLIERS"]) == _native_det.RANK_BY["inliers"]
    assert int(consts["DET_MIN_MATCHES"]) == _native_det.MIN_MATCHES == 6


def test_host_side_checks(lib):
    assert lib.det_version() >= 1
    assert lib.det_workspace_bytes(0, 10, 2000) == 0 and lib.det_workspace_bytes(1, 0, 2000) == 0
    assert lib.det_workspace_bytes(1, 10, 0) == 0
    one, many = lib.det_workspace_bytes(1, 4096, 2000), lib.det_workspace_bytes(15, 4096, 2000)
    assert one >= 4096 * 20 and many >= 15 * 4096 * 20 and many < 16 * one
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    rc = lib.det_affine_partial_from_matches(p, p, p, p, 1, 4096, 10, 6.0, 2000, 0, p, p, p, p, 64, None)
    assert rc == -2 and b"workspace" in lib.det_last_error()
    rc = lib.det_affine_partial_from_matches(p, p, p, p, 1, 16, 10, -1.0, 2000, 0, p, p, p, p, 1 << 20, None)
    assert rc == -1 and b"reproj_threshold" in lib.det_last_error()
    rc = lib.det_affine_partial_from_matches(None, p, p, p, 1, 16, 10, 6.0, 2000, 0, p, p, p, p, 1 << 20, None)
    assert rc == -1 and b"null" in lib.det_last_error()
    rc = lib.det_affine_partial_ransac(p, p, 0, 6.0, 2000, 0, p, p, p, p, 1 << 20, None)
    assert rc == -1 and b"expected" in lib.det_last_error()
    rc = lib.det_bbox_vote(p, p, p, 3, 480, 640, 5, p, p, p, None)
    assert rc == -1 and b"rank_by" in lib.det_last_error()
    K = (ctypes.c_double * 9)(*([0.0] * 9))
    for bad in (300, 1, 0, 4096):
        rc = lib.det_crop_resize(p, 48, 64, p, K, bad, p, p, p, None)
        assert rc == -1 and b"power of two" in lib.det_last_error(), bad


def test_source_hash_is_unchanged_by_the_detector_subdirectories(monkeypatch):
    """source_hash() covers top-level csrc/ and include/ files only: the detector's sources do not move it."""
    assert os.path.isdir(os.path.join(build_ext.CSRC, "detector")) and os.path.isdir(os.path.join(ROOT, "include", "detector"))
    h = build_ext.source_hash()
    real_listdir = os.listdir
    monkeypatch.setattr(os, "listdir", lambda d: [n for n in real_listdir(d) if n != "detector"])
    assert build_ext.source_hash() == h
    monkeypatch.undo()
    assert build_ext.source_hash() == h


def test_library_is_built_from_the_subdirectory_and_judged_stale_from_its_own_sources():
    assert all(s.startswith("detector" + os.sep) for s in build_ext.DET_SOURCES)
    assert os.path.basename(build_ext.DET_LIB_PATH) == "libdet_hip.so"
    deps = build_ext.DET_SOURCES + build_ext.DET_HEADERS
    assert all(os.path.exists(os.path.join(build_ext.CSRC, d)) for d in deps)
    assert not build_ext._stale(build_ext.DET_LIB_PATH, deps)


def test_sources_name_no_scalar_memory_stores_and_no_inline_assembly():
    pat = re.compile(r"s_(store|buffer_store|scratch_store|atomic|buffer_atomic|dcache_wb|dcache_discard)|\basm\b", re.I)
    for d in (os.path.join(build_ext.CSRC, "detector"), os.path.join(ROOT, "include", "detector")):
        for n in os.listdir(d):
            with open(os.path.join(d, n)) as f:
                assert not pat.search(f.read()), n
