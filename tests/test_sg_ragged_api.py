"""The ragged batch of the SuperGlue matcher, without a GPU: the four entry points are declared, exported and bound, they
validate every argument before the first HIP call, and pack_ragged / unpack_ragged / ragged_chunks are exact bookkeeping."""
import ctypes
import os
import re

import pytest
import torch

from onepose_amd import _native_sg, build_ext
from onepose_amd.superglue import IN_KEYS, pack_ragged, ragged_chunks, unpack_ragged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ("sg_ragged_workspace_bytes", "sg_forward_ragged", "sg_attention_ragged", "sg_sinkhorn_ragged", "sg_match_tail_ragged")


@pytest.fixture(scope="module")
def lib():
    if build_ext.is_stale():
        build_ext.build(verbose=False)
    return _native_sg.load()


def i32(*values):
    return (ctypes.c_int32 * len(values))(*values)


def test_ragged_symbols_are_declared_exported_and_bound(lib):
    with open(os.path.join(ROOT, "include", "superglue", "superglue.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    raw = ctypes.CDLL(_native_sg.LIB_PATH)
    for name in RAGGED:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(raw, name) and name in _native_sg.SYMBOLS, name
    assert re.search(r"#define\s+SG_MAX_ITEMS\s+64\b", text) and _native_sg.MAX_ITEMS == 64
    assert lib.sg_version() >= 2


def test_ragged_workspace_bytes_is_positive_and_monotone_in_b(lib):
    sizes = [lib.sg_ragged_workspace_bytes(b, 257, 130) for b in range(1, 65)]
    assert sizes[0] > 0 and all(a < c for a, c in zip(sizes, sizes[1:]))
    assert lib.sg_ragged_workspace_bytes(0, 257, 130) == 0 and lib.sg_ragged_workspace_bytes(65, 257, 130) == 0
    assert lib.sg_ragged_workspace_bytes(4, 0, 130) == 0


def forward_ragged(lib, b, n0, n1, ws, ws_bytes, cap0=10, cap1=12):
    """No pointer is valid: every call here must be refused before anything is launched."""
    hw = i32(*([480, 640] * max(b, 1)))
    kinds = i32(0)
    rc = lib.sg_forward_ragged(None, 0, kinds, 10, 0.2, *([None] * 6), b, cap0, cap1, i32(*n0), i32(*n1), hw, hw, *([None] * 5),
                               ws, ws_bytes, None)
    return rc, lib.sg_last_error().decode()


def test_forward_ragged_refuses_bad_arguments_without_a_gpu(lib):
    need = lib.sg_ragged_workspace_bytes(2, 10, 12)
    buf = ctypes.create_string_buffer(need)
    ws = ctypes.addressof(buf)
    for b, n0, n1, word in ((0, [1], [1], "b must be"), (65, [1] * 65, [1] * 65, "b must be"), (2, [3, 0], [1, 1], "n0 = 0"),
                            (2, [3, 10], [1, 13], "n1 = 13")):
        rc, msg = forward_ragged(lib, b, n0, n1, ws, need)
        assert rc == -1 and word in msg, (b, n0, n1, msg)
    rc, msg = forward_ragged(lib, 2, [3, 10], [12, 1], None, need)
    assert rc == -1 and "workspace is null" in msg
    rc, msg = forward_ragged(lib, 2, [3, 10], [12, 1], ws, need - 1)
    assert rc == -2 and "workspace too small" in msg
    # the counts are fine here: the next check (null tensors) is the one that answers
    rc, msg = forward_ragged(lib, 2, [3, 10], [12, 1], ws, need)
    assert rc == -1 and "null argument" in msg


def test_ragged_stages_refuse_bad_arguments_without_a_gpu(lib):
    assert lib.sg_attention_ragged(None, None, 2, 8, 8, i32(8, 9), i32(1, 1), None, None) == -1 and b"n0 = 9" in lib.sg_last_error()
    assert lib.sg_sinkhorn_ragged(None, None, 2, 8, 8, i32(8, 1), i32(0, 1), 3, None, None, 0, None) == -1
    assert b"n1 = 0" in lib.sg_last_error()
    buf = ctypes.create_string_buffer(16)
    rc = lib.sg_match_tail_ragged(None, 2, 8, 8, i32(8, 1), i32(8, 1), 0.2, None, None, None, None, ctypes.addressof(buf), 16, None)
    assert rc == -2 and b"workspace" in lib.sg_last_error()


def item(n0, n1, hw0, hw1, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, generator=g) + 0.5       # noqa: E731  (never zero: padding is told from data)
    return {"keypoints0": r(1, n0, 2), "scores0": r(1, n0), "descriptors0": r(1, 256, n0), "keypoints1": r(1, n1, 2),
            "scores1": r(1, n1), "descriptors1": r(1, 256, n1), "image0": torch.empty(1, 1, *hw0, device="meta"),
            "image1": torch.empty(1, 1, *hw1, device="meta")}


def test_pack_and_unpack_round_trip_on_cpu_tensors():
    shapes = [(5, 9), (0, 4), (12, 1), (7, 0), (12, 9)]
    sizes = [((480, 640), (640, 480)), ((700, 300), (1, 1)), ((1, 1), (480, 640)), ((640, 480), (700, 300)), ((480, 640), (480, 640))]
    items = [item(n0, n1, hw0, hw1, 10 + k) for k, ((n0, n1), (hw0, hw1)) in enumerate(zip(shapes, sizes))]
    p = pack_ragged(items)
    assert p["n0"] == [s[0] for s in shapes] and p["n1"] == [s[1] for s in shapes]
    assert p["hw0"] == [s[0] for s in sizes] and p["hw1"] == [s[1] for s in sizes]
    assert p["keypoints0"].shape == (5, 12, 2) and p["scores1"].shape == (5, 9) and p["descriptors1"].shape == (5, 256, 9)
    assert all(p[k].dtype == torch.float32 and p[k].is_contiguous() for k in IN_KEYS)
    back = unpack_ragged({k: p[k] for k in IN_KEYS}, p["n0"], p["n1"])
    for i, (d, u) in enumerate(zip(items, back)):
        for k in IN_KEYS:
            assert u[k].shape == d[k].shape and torch.equal(u[k], d[k]), (i, k)
            assert u[k].numel() == 0 or u[k].data_ptr() == p[k][i:i + 1].data_ptr()   # a view of the padded tensor
    # the padding is zero
    assert float(p["scores0"][1].abs().sum()) == 0 and float(p["descriptors1"][3].abs().sum()) == 0
    assert float(p["keypoints0"][0, 5:].abs().sum()) == 0
    # both sides empty everywhere still gives capacity 1
    q = pack_ragged([item(0, 0, (4, 4), (4, 4), 1)])
    assert q["keypoints0"].shape == (1, 1, 2) and q["descriptors1"].shape == (1, 256, 1)
    with pytest.raises(ValueError):
        pack_ragged([])


def test_seventeen_items_are_chunked_sixteen_plus_one():
    items = [item(1 + k % 5, 2 + k % 3, (480, 640), (640, 480), 100 + k) for k in range(17)]
    chunks = ragged_chunks(items, 16)
    assert [len(c) for c in chunks] == [16, 1] and [d for c in chunks for d in c] == items
    seen = 0
    for c in chunks:
        p = pack_ragged(c)
        for d, u in zip(c, unpack_ragged({k: p[k] for k in IN_KEYS}, p["n0"], p["n1"])):
            assert all(torch.equal(u[k], d[k]) for k in IN_KEYS)
            seen += 1
    assert seen == 17
    assert [len(c) for c in ragged_chunks(items, 64)] == [17] and [len(c) for c in ragged_chunks(items, 4)] == [4, 4, 4, 4, 1]
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_items"):
            ragged_chunks(items, bad)


def test_match_pairs_refuses_training_mode_and_cpu_inputs():
    from onepose_amd import SuperGlue
    model = SuperGlue({"GNN_layers": ["self", "cross"]})
    with pytest.raises(RuntimeError, match="inference only"):
        model.train().match_pairs([item(3, 3, (8, 8), (8, 8), 0)])
    model.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.match_pairs([item(3, 3, (8, 8), (8, 8), 0), item(4, 2, (8, 8), (8, 8), 1)])
    # pairs with an empty side never reach the library: the reference's empty result, also on the CPU
    out = model.match_pairs([item(0, 3, (8, 8), (8, 8), 0), item(4, 0, (8, 8), (8, 8), 1)])
    assert out[0]["matches0"].shape == (1, 0) and out[0]["matches1"].tolist() == [[-1, -1, -1]]
    assert out[1]["matches0"].tolist() == [[-1] * 4] and out[1]["matching_scores0"].tolist() == [[0.0] * 4]
