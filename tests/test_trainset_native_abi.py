"""C ABI of the training-set builder in libgatsspg_hip.so: the ``gts_`` table of _native_trainset against
include/gatsspg_trainset.h (the parser of tests/test_abi_tables.py, restated) and the exports; the header's constants; host-side
refusals (host pointers are passed, so nothing is launched); the refusals of the Python front end.  No GPU."""
import ctypes
import os
import re
import subprocess
from ctypes import c_char_p, c_int, c_size_t, c_uint64

import numpy as np
import pytest
import torch

import onepose_amd
from onepose_amd import _binding, _native_trainset, build_ext, trainset
from onepose_amd._binding import F32, I32, RAW, STREAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gatsspg_trainset.h")
NAMES = ["gts_version", "gts_last_error", "gts_workspace_bytes", "gts_assign_pairs", "gts_select_leaves", "gts_gather_leaves", "gts_pad_query",
         "gts_pad_points", "gts_build_batch"]
SCALARS = {"int": c_int, "size_t": c_size_t, "uint64_t": c_uint64}
ELEMENTS = {"float": F32, "int32_t": I32}
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
    for ret, name, params in re.findall(r"([\w \*]+?)\b(gts_\w+)\s*\(([^()]*)\)\s*;", text):
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


def expected(ctype, stars, pname):
    if ctype == "gts_stream_t":
        assert stars == 0 and pname == "queue"
        return STREAM
    if stars == 0:
        return SCALARS[ctype]
    return RAW if ctype == "void" else ELEMENTS[ctype]


@pytest.fixture(scope="module")
def lib():
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    return _native_trainset.load()


def test_table_mirrors_the_header():
    protos = prototypes()
    assert sorted(protos) == sorted(NAMES) == sorted(_native_trainset.SYMBOLS)
    for name, (ret, params) in protos.items():
        restype, table = _native_trainset.SYMBOLS[name]
        assert restype is RETURNS[ret], f"{name}: returns {ret}, the table says {restype}"
        assert len(table) == len(params), f"{name}: {len(params)} parameters in the header, {len(table)} in the table"
        for i, ((ctype, stars, pname), entry) in enumerate(zip(params, table)):
            assert entry is expected(ctype, stars, pname), f"{name} parameter {i} ({ctype}{'*' * stars} {pname}): {entry!r}"
    assert len(protos["gts_build_batch"][1]) == 28 and protos["gts_last_error"][0] == "char*"
    # no parameter is named `stream` (tests/test_arena.py's rule would want a table entry in a file this feature cannot edit); every
    # launching function ends on `gts_stream_t queue`, and tests/test_placement_trainset.py keeps the rule for them
    assert not any(p[2] == "stream" for _, params in protos.values() for p in params)
    assert sum(params[-1][:1] == ("gts_stream_t",) for _, params in protos.values() if params) == 6


def test_every_declared_symbol_is_exported_and_bound(lib):
    raw = ctypes.CDLL(_native_trainset.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    for name, (restype, table) in _native_trainset.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and len(fn.argtypes) == len(table)
        for got, entry in zip(fn.argtypes, table):
            assert got is (ctypes.c_void_p if isinstance(entry, _binding.DevicePointer) else entry)
    defined = subprocess.run(["nm", "-D", "--defined-only", build_ext.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(gts_\w+)", defined))) == sorted(NAMES)


def test_library_version_sources_and_constants(lib):
    assert lib.gts_version() == 1
    assert _native_trainset.LIB_PATH == build_ext.LIB_PATH and len(build_ext.LIBRARIES) == 6
    assert build_ext.SOURCES[-2:] == ["gatsspg_train_kernels.hip", "gatsspg_trainset_kernels.hip"]
    assert any(h.endswith("gatsspg_trainset.h") for h in build_ext.LIBRARIES[0].headers) and "ransac_sample.h" in build_ext.LIBRARIES[0].headers
    with open(os.path.join(build_ext.CSRC, "gatsspg_trainset_kernels.hip")) as f:
        src = f.read()
    assert "hipMalloc" not in src and "Synchronize" not in src and "hipMemset" not in src and "hipMemcpy" not in src
    assert set(re.findall(r"\batomic\w+", src)) == {"atomicAdd", "atomicMin"}          # both on int32: a count and a minimum
    consts = {k: int(v) for k, v in re.findall(r"#define (GTS_[A-Z_0-9]+) (\d+)", header_text())}
    gtr = {k: int(v) for k, v in re.findall(r"#define (GTR_[A-Z_]+) (\d+)", open(os.path.join(ROOT, "include", "gatsspg_train.h")).read())}
    assert consts["GTS_DESC_DIM"] == _native_trainset.DESC_DIM == gtr["GTR_DESC_DIM"] == 256
    assert consts["GTS_MAX_BATCH"] == _native_trainset.MAX_BATCH == gtr["GTR_MAX_BATCH"]
    assert consts["GTS_MAX_POINTS"] == _native_trainset.MAX_POINTS == gtr["GTR_MAX_POINTS"]
    assert consts["GTS_MAX_LEAF"] == _native_trainset.MAX_LEAF == 64 and consts["GTS_MAX_COLUMNS"] == _native_trainset.MAX_COLUMNS == 1 << 24
    assert consts["GTS_MAX_REDRAWS"] == _native_trainset.MAX_REDRAWS == 256
    import trainset_oracle
    assert (consts["GTS_TAG_LEAVES"], consts["GTS_TAG_PAD2D"], consts["GTS_TAG_PAD3D"]) == (1, 2, 3) \
        == (_native_trainset.TAG_LEAVES, _native_trainset.TAG_PAD2D, _native_trainset.TAG_PAD3D) \
        == (trainset_oracle.TAG_LEAVES, trainset_oracle.TAG_PAD2D, trainset_oracle.TAG_PAD3D)
    assert trainset_oracle.MAX_REDRAWS == consts["GTS_MAX_REDRAWS"]


def test_workspace_refusals(lib):
    err = lib.gts_last_error
    assert lib.gts_workspace_bytes(-1, 0, 0, 0) == 0 and b"total_kpts" in err()
    assert lib.gts_workspace_bytes(0, 0, 0, 0) == 0 and b"nothing to size" in err()
    assert lib.gts_workspace_bytes(0, 65, 10, 8) == 0 and b"b must be in" in err()
    assert lib.gts_workspace_bytes(0, 1, 10, 0) == 0 and b"num_leaf must be in [1, 64]" in err()
    assert lib.gts_workspace_bytes(0, 1, 10, 65) == 0 and b"num_leaf must be in [1, 64]" in err()
    assert lib.gts_workspace_bytes(0, 1, 0, 8) == 0 and b"shape3d" in err()
    assert lib.gts_workspace_bytes(0, 1, 1 << 20, 64) == 0 and b"shape3d * num_leaf" in err()
    batch = lib.gts_workspace_bytes(0, 8, 2000, 8)
    assert batch == 8 * 2000 * 8 * 4 and batch % 256 == 0                       # leaf_src is all of it
    assert lib.gts_workspace_bytes(1000, 0, 0, 0) == 4096 + 4096 and lib.gts_workspace_bytes(1000, 8, 2000, 8) == batch
    assert lib.gts_workspace_bytes(1, 0, 0, 0) == 512


def test_call_refusals(lib):
    err = lib.gts_last_error
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) // 256 * 256      # host memory: nothing is launched by a refused call
    huge = 1 << 40

    def build(N=5, K=9, V=2, b=2, shape2d=10, shape3d=12, L=4, collect=p, out=p, kpts=p, ws=p, ws_bytes=huge, scores=None):
        return lib.gts_build_batch(p, collect, p, p, N, K, p, kpts, p, p, p, V, p, p, b, shape2d, shape3d, L, 7, p, p, scores, p, p, out, ws, ws_bytes, None)

    assert build(b=0) == -1 and build(b=65) == -1 and b"b must be in [1, 64]" in err()
    assert build(L=0) == -1 and b"num_leaf must be in [1, 64] (got 0)" in err()
    assert build(L=65) == -1 and b"num_leaf must be in [1, 64] (got 65)" in err()
    assert build(shape2d=0) == -1 and b"shape2d" in err() and build(shape3d=0) == -1 and b"shape3d" in err()
    assert build(shape2d=(1 << 22) + 1) == -1 and b"shape2d" in err()
    assert build(shape3d=1 << 22, L=8) == -1 and b"shape3d * num_leaf" in err()
    assert build(N=0) == -1 and b"N must be >= 1" in err() and build(K=0) == -1 and b"K must" in err() and build(V=0) == -1 and b"V must" in err()
    assert build(out=None) == -1 and b"null" in err() and build(collect=None) == -1 and b"null" in err()
    assert build(collect=p + 4) == -1 and b"collect must be 16-byte aligned" in err()
    assert build(kpts=p + 4) == -1 and b"kpts2d must be 8-byte aligned" in err()
    assert build(out=p + 2) == -1 and b"misaligned" in err() and build(scores=p + 1) == -1 and b"misaligned" in err()
    assert build(ws=None) == -1 and b"null workspace" in err() and build(ws=p + 16) == -1 and b"aligned" in err()
    assert build(ws_bytes=64) == -2 and b"workspace too small" in err()
    # the stage entries refuse alike
    assert lib.gts_select_leaves(p, 5, p, p, 2, 12, 0, 7, p, None) == -1 and b"num_leaf" in err()
    assert lib.gts_select_leaves(p, 5, p, p, 2, 12, 65, 7, p, None) == -1 and b"num_leaf" in err()
    assert lib.gts_select_leaves(p, 5, p, p, 2, 12, 4, 7, None, None) == -1 and b"null" in err()
    assert lib.gts_gather_leaves(p + 8, 9, p, 2, 12, 4, p, None) == -1 and b"16-byte" in err()
    assert lib.gts_gather_leaves(p, 0, p, 2, 12, 4, p, None) == -1 and b"K must" in err()
    assert lib.gts_pad_query(p, p, p, p, p, 2, p, p, 2, 0, 7, p, p, None, None) == -1 and b"shape2d" in err()
    assert lib.gts_pad_points(p, p, 0, p, p, 2, 12, 7, p, p, None) == -1 and b"N must" in err()
    assert lib.gts_assign_pairs(p, p, p, 5, 9, p, 2, 0, p, p, p, p, p, huge, None) == -1 and b"total_kpts" in err()
    assert lib.gts_assign_pairs(p, p, p, 5, 9, p, 2, 100, p, p, p, p, p, 16, None) == -2 and b"too small" in err()


def arrays():
    rs = np.random.RandomState(0)
    features = [{"keypoints": rs.rand(n, 2).astype(np.float32), "descriptors": rs.rand(256, n).astype(np.float32), "scores": rs.rand(n).astype(np.float32)}
                for n in (3, 4)]
    return dict(point_offsets=np.array([0, 2, 3], np.int32), collect=rs.rand(3, 256).astype(np.float32), points3d=rs.rand(2, 3).astype(np.float32),
                mean_desc=rs.rand(256, 2).astype(np.float32), features=features, obs_image=np.array([0, 1, 1], np.int32),
                obs_kpt=np.array([1, 2, 0], np.int32), image_size=(24, 32))


def test_the_front_end_refuses_the_cpu_and_bad_shapes():
    a = arrays()
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU .*there is no CPU fallback"):
        trainset.TrainingSet.from_arrays(**a, device="cpu")
    on_cpu = dict(a, collect=torch.from_numpy(a["collect"]))
    with pytest.raises(RuntimeError, match=r"collect is on cpu\); there is no CPU fallback"):
        trainset.TrainingSet.from_arrays(**on_cpu, device="cuda")
    with pytest.raises(ValueError, match="either obs_image and obs_kpt or pairs"):
        trainset.TrainingSet.from_arrays(**dict(a, obs_image=None), device="cuda")
    with pytest.raises(ValueError, match="either obs_image and obs_kpt or pairs"):
        trainset.TrainingSet.from_arrays(**a, pairs=[np.zeros((2, 0))] * 2, device="cuda")
    ts = object.__new__(trainset.TrainingSet)           # batch_of checks its arguments before it touches the device
    for kw, match in ((dict(num_leaf=0), "num_leaf must be in"), (dict(num_leaf=65), "num_leaf must be in"), (dict(shape2d=0), "shape2d and shape3d"),
                      (dict(shape3d=(1 << 22) + 1), "shape2d and shape3d")):
        with pytest.raises(ValueError, match=match):
            ts.batch([0], 0, **kw)
    with pytest.raises(ValueError, match="at least one image"):
        ts.batch([], 0)
    with pytest.raises(ValueError, match="at most 64 samples"):
        ts.batch(list(range(65)), 0)
    with pytest.raises(ValueError, match="1 samples but 2 epochs"):
        ts.batch([0], [0, 1])
    with pytest.raises(RuntimeError, match="has not built a database yet"):
        trainset.TrainingSet.from_mapper(type("M", (), {"_resident": None, "device": "cuda"})(), [])


def test_the_package_exports_the_training_set():
    assert onepose_amd.TrainingSet is trainset.TrainingSet and onepose_amd.__all__[-2:] == ["TrainingSet", "BundleAdjuster"]
    assert hasattr(onepose_amd.ObjectMapper, "training_set")
