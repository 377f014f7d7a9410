"""C ABI of libsuperglue_hip.so: every header symbol is exported and bound; the new sources leave build_ext.source_hash() alone."""
import ctypes
import os
import re

import pytest

from onepose_amd import _native_sg, build_ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "superglue", "superglue.h")


def header_functions():
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sg_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    return _native_sg.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = header_functions()
    assert "sg_forward" in names and "sg_sinkhorn" in names and "sg_attention" in names
    raw = ctypes.CDLL(_native_sg.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), n
    assert set(names) == set(_native_sg.SYMBOLS)


def test_host_side_checks(lib):
    assert lib.sg_version() >= 1
    assert lib.sg_packed_weights_bytes(18) == 4 * (4 + 111_296 + 18 * 659_200 + 65_792)
    assert lib.sg_packed_weights_bytes(-1) == 0
    assert lib.sg_workspace_bytes(0, 5, 5) == 0 and lib.sg_workspace_bytes(1, 5, 5) > 0
    rc = lib.sg_sinkhorn(None, None, 1, 0, 5, 10, None, None, 0, None)
    assert rc < 0 and b"n0" in lib.sg_last_error()
    ws = ctypes.create_string_buffer(16)
    rc = lib.sg_match_tail(None, 1, 8, 8, 0.2, None, None, None, None, ctypes.addressof(ws), 16, None)
    assert rc == -2 and b"workspace" in lib.sg_last_error()
    rc = lib.sg_attention(None, None, 1, 5, 0, None, None)
    assert rc == -1 and b"M" in lib.sg_last_error()
    buf = ctypes.create_string_buffer(16)
    rc = lib.sg_attention(ctypes.addressof(buf), ctypes.addressof(buf), 1, 1, 1, ctypes.addressof(buf), None)
    assert rc == -1 and b"alias" in lib.sg_last_error()
    kinds = (ctypes.c_int32 * 1)(7)
    big = lib.sg_workspace_bytes(1, 4, 4)
    buf = ctypes.create_string_buffer(big)
    rc = lib.sg_forward(None, 1, kinds, 10, 0.2, *([None] * 6), 1, 4, 4, 8, 8, 8, 8, *([None] * 5), ctypes.addressof(buf), big, None)
    assert rc == -1 and b"kind" in lib.sg_last_error()


def test_source_hash_ignores_superglue_subdirectories(monkeypatch, tmp_path):
    """source_hash() covers top-level csrc/ and include/ files only: adding or editing files under the superglue/ subdirectories
    does not change it (bench.py keeps calling the committed PMC profile 'THIS build')."""
    assert os.path.isdir(os.path.join(build_ext.CSRC, "superglue"))
    assert os.path.isdir(os.path.join(ROOT, "include", "superglue"))
    h = build_ext.source_hash()
    real_listdir = os.listdir
    monkeypatch.setattr(os, "listdir", lambda d: [n for n in real_listdir(d) if n != "superglue"])
    assert build_ext.source_hash() == h
    monkeypatch.undo()
    assert build_ext.source_hash() == h


def test_library_is_built_from_the_subdirectory():
    assert all(s.startswith("superglue" + os.sep) for s in build_ext.SG_SOURCES)
    assert os.path.basename(build_ext.SG_LIB_PATH) == "libsuperglue_hip.so"


def test_sources_name_no_scalar_memory_stores():
    pat = re.compile(r"s_(store|buffer_store|scratch_store|atomic|buffer_atomic|dcache_wb|dcache_discard)", re.I)
    for d in (os.path.join(build_ext.CSRC, "superglue"), os.path.join(ROOT, "include", "superglue")):
        for n in os.listdir(d):
            with open(os.path.join(d, n)) as f:
                assert not pat.search(f.read()), n
