"""The batched pose solver without a GPU: its entry points are declared, exported and bound, they validate every argument before the
first HIP call, and the Python wrappers refuse what the library cannot take."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from onepose_amd import _binding, _native_pnp, build_ext, pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ("pnp_batch_workspace_bytes", "pnp_ransac_epnp_batch", "pnp_ransac_epnp_matches_batch")
K9 = (ctypes.c_double * (9 * 33))(*([600.0, 0, 256, 0, 600.0, 256, 0, 0, 1] * 33))


@pytest.fixture(scope="module")
def lib():
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    return _native_pnp.load()


def i32(*values):
    return (ctypes.c_int32 * len(values))(*values)


def u64(*values):
    return (ctypes.c_uint64 * len(values))(*values)


def test_batch_symbols_are_declared_exported_and_bound(lib):
    """The batched entry points are part of the ABI of include/pnp.h through include/pnp_batch.h, which it includes, and are bound from
    _native_pnp.MORE_SYMBOLS: tests/test_pnp.py and tests/test_abi_tables.py pin the functions pnp.h ITSELF declares, and SYMBOLS, to the
    nine of pnp_version() 1 and pnp_refit of pnp_version() 3."""
    with open(os.path.join(ROOT, "include", "pnp.h")) as f:
        assert re.search(r'^#include "pnp_batch.h"', f.read(), flags=re.M)
    with open(os.path.join(ROOT, "include", "pnp_batch.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    raw = ctypes.CDLL(_native_pnp.LIB_PATH)
    assert set(re.findall(r"\b(pnp_[a-z0-9_]+)\s*\(", text)) == set(BATCH) == set(_native_pnp.MORE_SYMBOLS)
    for name in BATCH:
        assert hasattr(raw, name) and name not in _native_pnp.SYMBOLS, name
        fn = getattr(lib, name)                                            # bound by load(), markers lowered like the first table's
        restype, table = _native_pnp.MORE_SYMBOLS[name]
        assert fn.restype is restype and len(fn.argtypes) == len(table)
        assert all(got is (ctypes.c_void_p if isinstance(entry, _binding.DevicePointer) else entry) for got, entry in zip(fn.argtypes, table))
    assert re.search(r"#define\s+PNP_MAX_ITEMS\s+32\b", text) and _native_pnp.MAX_ITEMS == 32
    assert lib.pnp_version() == 3                                          # 3: the flatness guard, pnp_refit and the one NO MODEL state


def test_batch_table_mirrors_its_header():
    """Parameter by parameter, with typed pointers: tests/test_abi_tables.py's rule (a pointer to T is the device marker of T or the
    ctypes pointer of a HOST array of T, nothing else) applied to include/pnp_batch.h."""
    from ctypes import POINTER, c_double, c_int, c_int32, c_int64, c_size_t, c_uint64
    from onepose_amd._binding import F32, F64, I32, I64, RAW, STREAM
    scalars = {"int": c_int, "double": c_double, "size_t": c_size_t}
    elements = {"float": (F32, POINTER(ctypes.c_float)), "double": (F64, POINTER(c_double)), "int32_t": (I32, POINTER(c_int32)),
                "int64_t": (I64, POINTER(c_int64)), "uint64_t": (POINTER(c_uint64),)}           # no device marker for uint64: host only
    with open(os.path.join(ROOT, "include", "pnp_batch.h")) as f:
        text = re.sub(r"^\s*#.*$", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(pnp_\w+)\s*\(([^()]*)\)\s*;", text)
    assert {name for _, name, _ in protos} == set(BATCH)
    for ret, name, params in protos:
        restype, table = _native_pnp.MORE_SYMBOLS[name]
        assert restype is {"int": c_int, "size_t": c_size_t}[ret.strip()]
        plist = [q.strip() for q in params.split(",")]
        assert len(plist) == len(table), name
        for q, entry in zip(plist, table):
            words = [w for w in re.findall(r"\w+|\*", q)[:-1] if w != "const"]
            ctype, stars = " ".join(w for w in words if w != "*"), words.count("*")
            ok = ((STREAM,) if ctype == "pnp_stream_t" else (scalars[ctype],) if stars == 0 else (RAW,) if ctype == "void" else elements[ctype])
            assert any(entry is a for a in ok), f"{name}: {q}: the table says {entry!r}"
    # what the host passes per frame is typed as the issue states it
    seeds = [q for _, name, params in protos for q in params.split(",") if "seeds" in q]
    assert len(seeds) == 2 and all(re.fullmatch(r"\s*const uint64_t\* seeds\s*", q) for q in seeds)


def test_batch_workspace_bytes_is_positive_and_monotone(lib):
    size = lib.pnp_batch_workspace_bytes
    by_b = [size(b, 500, 1000) for b in range(1, 33)]
    assert by_b[0] > 0 and all(a < c for a, c in zip(by_b, by_b[1:]))
    # a frame's slice does not depend on b: frame i starts at i slices
    assert by_b == [b * by_b[0] for b in range(1, 33)]
    # pieces are rounded to 256 bytes: strictly more from one 256-byte step to the next, never less in between
    by_cap = [size(4, cap, 1000) for cap in (1, 2, 64, 65, 500, 1000, 2049)]
    by_it = [size(4, 500, it) for it in (1, 2, 64, 65, 1000, 10000)]
    assert all(a <= c for a, c in zip(by_cap, by_cap[1:])) and by_cap[0] < by_cap[2] < by_cap[4] < by_cap[6]
    assert all(a <= c for a, c in zip(by_it, by_it[1:])) and by_it[0] < by_it[2] < by_it[4] < by_it[5]
    assert size(1, 500, 1000) >= lib.pnp_workspace_bytes(500, 1000)
    for b, cap, it in ((0, 500, 1000), (33, 500, 1000), (4, 0, 1000), (4, 500, 0)):
        assert size(b, cap, it) == 0, (b, cap, it)


def solve_batch(lib, b=2, cap=10, n=(5, 10), ws=1, ws_bytes=None, scale=1000.0, thr=5.0, iterations=64, p3=1, p2=1, K=K9, seeds=True,
                pose=1, mask=1, info=1, n_null=False):
    """Every device pointer is 1 (never dereferenced on the host) or None: each call here must be refused before anything is launched."""
    need = lib.pnp_batch_workspace_bytes(max(1, min(b, 32)), max(cap, 1), max(1, min(iterations, 1 << 24)))
    rc = lib.pnp_ransac_epnp_batch(p3, p2, K, None if n_null else i32(*n), u64(*([7] * max(b, 1))) if seeds else None, b, cap, scale, thr,
                                   iterations, pose, mask, info, ws, need if ws_bytes is None else ws_bytes, None)
    return rc, lib.pnp_last_error().decode()


def solve_matches_batch(lib, b=2, cap1=10, n1=(5, 10), n3=20, shared3d=1, ws=1, ws_bytes=None, scale=1000.0, thr=5.0, iterations=64, k2=1,
                        k3=1, m0=1, K=K9, seeds=True, pose=1, mask=1, info=1, n_null=False):
    need = lib.pnp_batch_workspace_bytes(max(1, min(b, 32)), max(cap1, 1), max(1, min(iterations, 1 << 24)))
    rc = lib.pnp_ransac_epnp_matches_batch(k2, k3, m0, K, None if n_null else i32(*n1), u64(*([7] * max(b, 1))) if seeds else None, b, cap1,
                                           n3, shared3d, scale, thr, iterations, pose, mask, info, ws, need if ws_bytes is None else ws_bytes,
                                           None)
    return rc, lib.pnp_last_error().decode()


COMMON_REFUSALS = [
    (dict(b=0), "b must be"), (dict(b=33), "b must be"),
    (dict(iterations=0), "iterations"), (dict(iterations=(1 << 24) + 1), "iterations"),
    (dict(scale=0.0), "positive"), (dict(scale=-1.0), "positive"), (dict(scale=float("nan")), "positive"),
    (dict(thr=0.0), "positive"), (dict(thr=-5.0), "positive"),
    (dict(K=None), "null"), (dict(seeds=False), "null"), (dict(n_null=True), "null"),
    (dict(pose=None), "null"), (dict(mask=None), "null"), (dict(info=None), "null"), (dict(ws=None), "workspace is null"),
]


def test_batch_refuses_bad_arguments_without_a_gpu(lib):
    cases = COMMON_REFUSALS + [(dict(n=(5, -1)), "n = -1"), (dict(n=(11, 5)), "n = 11"), (dict(cap=0, n=(0, 0)), "cap"),
                               (dict(p3=None), "null"), (dict(p2=None), "null")]
    for kw, word in cases:
        rc, msg = solve_batch(lib, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    n33 = [5] * 33
    rc, msg = solve_batch(lib, b=33, n=n33)
    assert rc == -1 and "b must be" in msg
    need = lib.pnp_batch_workspace_bytes(2, 10, 64)
    rc, msg = solve_batch(lib, ws_bytes=need - 1)
    assert rc == -2 and "workspace too small" in msg
    rc, msg = solve_batch(lib, ws_bytes=0)
    assert rc == -2 and "workspace too small" in msg
    # a bad argument is named before the workspace is looked at
    rc, msg = solve_batch(lib, n=(5, 11), ws_bytes=0)
    assert rc == -1 and "n = 11" in msg


def test_matches_batch_refuses_bad_arguments_without_a_gpu(lib):
    cases = COMMON_REFUSALS + [(dict(n1=(5, -1)), "n = -1"), (dict(n1=(11, 5)), "n = 11"), (dict(cap1=0, n1=(0, 0)), "cap1"),
                               (dict(k2=None), "null"), (dict(k3=None), "null"), (dict(m0=None), "null"),
                               (dict(shared3d=2), "shared3d"), (dict(shared3d=-1), "shared3d"), (dict(n3=0), "n3")]
    for kw, word in cases:
        rc, msg = solve_matches_batch(lib, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    need = lib.pnp_batch_workspace_bytes(2, 10, 64)
    rc, msg = solve_matches_batch(lib, ws_bytes=need - 1)
    assert rc == -2 and "workspace too small" in msg
    rc, msg = solve_matches_batch(lib, shared3d=0, ws_bytes=need - 1)
    assert rc == -2 and "workspace too small" in msg


def test_wrappers_refuse_cpu_tensors_wrong_dtypes_and_a_wrong_k():
    K = np.array([[600.0, 0, 256], [0, 600.0, 256], [0, 0, 1]])
    p2, p3 = torch.zeros(2, 8, 2), torch.zeros(2, 8, 3)
    m0 = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pnp.ransac_pnp_batch(K, p2, p3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pnp.ransac_pnp_from_matches_batch(K, p2, torch.zeros(20, 3), m0)
    # shapes are checked before anything else
    for bad2, bad3 in ((torch.zeros(8, 2), torch.zeros(8, 3)), (torch.zeros(2, 8, 3), p3), (p2, torch.zeros(2, 7, 3)), (p2, torch.zeros(3, 8, 3))):
        with pytest.raises(ValueError, match="pts_2d must be"):
            pnp.ransac_pnp_batch(K, bad2, bad3)
    with pytest.raises(ValueError, match="matches0"):
        pnp.ransac_pnp_from_matches_batch(K, p2, torch.zeros(20, 3), torch.zeros(2, 7, dtype=torch.int64))
    with pytest.raises(ValueError, match="kpts3d must be"):
        pnp.ransac_pnp_from_matches_batch(K, p2, torch.zeros(3, 20, 3), m0)
    # dtypes: coordinates are floating point, matches0 is the matcher's int64
    with pytest.raises(TypeError, match="floating-point"):
        pnp.ransac_pnp_batch(K, p2.to(torch.int32), p3)
    with pytest.raises(TypeError, match="floating-point"):
        pnp.ransac_pnp_batch(K, p2, p3.to(torch.int64))
    for bad in (m0.to(torch.int32), m0.to(torch.float32)):
        with pytest.raises(TypeError, match="matches0 int64"):
            pnp.ransac_pnp_from_matches_batch(K, p2, torch.zeros(20, 3), bad)
    with pytest.raises(TypeError, match="floating-point"):
        pnp.ransac_pnp_from_matches_batch(K, p2, torch.zeros(20, 3, dtype=torch.int32), m0)
    # the host arguments
    check = pnp._batch_host_arguments
    for bad_k in (np.zeros((2, 2)), np.zeros((3, 3, 3)), np.zeros((1, 3, 3)), np.zeros(9)):
        with pytest.raises(ValueError, match="K must be"):
            check(bad_k, None, 0, 2, 8)
    for bad_counts in ([8], [8, 9], [-1, 8], [1, 2, 3]):
        with pytest.raises(ValueError, match="counts must be"):
            check(K, bad_counts, 0, 2, 8)
    with pytest.raises(ValueError, match="seeds must be"):
        check(K, None, [1, 2, 3], 2, 8)
    k, n, s = check(np.stack([K, 2 * K]), [0, 8], [2 ** 63 + 1, 2 ** 24 + 3], 2, 8)
    assert k.shape == (2, 9) and k.dtype == np.float64 and k[1, 0] == 1200.0 and n.dtype == np.int32 and n.tolist() == [0, 8]
    assert s.dtype == np.uint64 and s.tolist() == [2 ** 63 + 1, 2 ** 24 + 3]
    k, n, s = check(torch.from_numpy(K), None, 5, 3, 8)
    assert k.shape == (3, 9) and (k == K.reshape(9)).all() and n.tolist() == [8, 8, 8] and s.tolist() == [5, 5, 5]


class Recorder:
    """Stands in for the library's call table: records the arguments of every native call instead of launching."""

    def __init__(self):
        self.calls = []

    def __call__(self, name, device, *args):
        self.calls.append((name, args))


def test_thirty_three_frames_are_chunked_thirty_two_plus_one(lib, monkeypatch):
    assert [(r.start, r.stop) for r in pnp.frame_chunks(33)] == [(0, 32), (32, 33)]
    assert [(r.start, r.stop) for r in pnp.frame_chunks(32)] == [(0, 32)] and [len(r) for r in pnp.frame_chunks(9, 4)] == [4, 4, 1]
    for bad in (0, 33):
        with pytest.raises(ValueError, match="max_items"):
            pnp.frame_chunks(5, bad)
    # the wrapper itself, on meta tensors (no storage, nothing launched): two native calls, 32 frames and 1
    rec = Recorder()
    monkeypatch.setattr(_native_pnp, "call", rec)
    monkeypatch.setattr(pnp, "gpu_tensor", lambda t, dtype, refusal: t)
    p2, p3 = torch.empty(33, 8, 2, device="meta"), torch.empty(33, 8, 3, device="meta")
    K = np.array([[600.0, 0, 256], [0, 600.0, 256], [0, 0, 1]])
    pose, mask, info = pnp.ransac_pnp_batch(K, p2, p3, counts=list(range(8)) * 4 + [3], iterations=64, seeds=list(range(33)))
    assert pose.shape == (33, 3, 4) and mask.shape == (33, 8) and info.shape == (33, 4)
    assert [name for name, _ in rec.calls] == ["pnp_ransac_epnp_batch"] * 2
    for (_, a), (b, first) in zip(rec.calls, ((32, 0), (1, 32))):
        assert a[5] == b and a[6] == 8 and a[0].shape[0] == b and a[10].shape == (b, 3, 4) and a[11].shape == (b, 8)
        assert a[3][0] == (0 if first == 0 else 3)                                                   # counts and seeds start at the chunk
        assert a[4][0] == first and a[14] == lib.pnp_batch_workspace_bytes(b, 8, 64)
    rec.calls.clear()
    m0 = torch.empty(33, 8, dtype=torch.int64, device="meta")
    pnp.ransac_pnp_from_matches_batch(K, p2, torch.empty(20, 3, device="meta"), m0, iterations=64)
    assert [(name, a[6], a[7], a[8], a[9]) for name, a in rec.calls] == [("pnp_ransac_epnp_matches_batch", 32, 8, 20, 1),
                                                                          ("pnp_ransac_epnp_matches_batch", 1, 8, 20, 1)]
    rec.calls.clear()
    pnp.ransac_pnp_from_matches_batch(K, p2, torch.empty(33, 20, 3, device="meta"), m0, iterations=64)
    assert [(a[6], a[9], a[1].shape[0]) for _, a in rec.calls] == [(32, 0, 32), (1, 0, 1)]
