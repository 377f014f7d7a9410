"""Placement tests of the GATsSPG matcher (include/gatsspg.h): gatsspg_pack_weights, gatsspg_forward, gatsspg_prepare_database +
gatsspg_forward_cached and gatsspg_forward_frames with every device argument an exact piece of a guarded arena (tests/arena.py) under
the fills 0xFF and 0x00, in all five arithmetics (the workspace layout depends on the arithmetic): the blob is exactly
gatsspg_packed_weights_bytes, the cache exactly gatsspg_db_cache_bytes, every workspace exactly the gatsspg_workspace_bytes the header
names for that call; and gatsspg_keypoint_encoder, which no forward calls.  Every case runs a second time with each call captured and
replayed (arena.run_captured).  Bitwise comparisons only; the oracle comparisons stay in tests/test_hip_parity.py, tests/test_gats_*.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from arena import captured_twin, run_placement
from onepose_amd import _native, synthetic
from onepose_amd.gats_superglue import GNN_LAYER_NAMES

BINDING = _native
_OUT = dict(conf="out", matches0="out", matches1="out", mscores0="out", mscores1="out", ws="scratch")
ROLES = {
    "gatsspg_pack_weights": dict(packed="scratch"),       # (raw is a HOST struct of device pointers: the tensors it names are pieces)
    "gatsspg_forward": dict(packed="in", desc2d_query="in", desc3d_db="in", desc2d_db="in", **_OUT),
    "gatsspg_prepare_database": dict(packed="in", desc3d_db="in", desc2d_db="in", cache="scratch", ws="scratch"),
    "gatsspg_forward_cached": dict(packed="in", desc2d_query="in", desc2d_db="in", cache="in", **_OUT),
    "gatsspg_forward_frames": dict(packed="in", desc2d_query="in", desc2d_db="in", cache="in", **_OUT),
    "gatsspg_keypoint_encoder": dict(kpts="in", scores="in", out="out", scratch="scratch"),     # (w is a HOST struct of device pointers)
}
SHAPES = [(2, 7, 65, 8), (1, 129, 129, 3)]            # (b, n1, n2, num_leaf)
SCALE, THRESHOLD = 0.07, 0.2
CAPACITY = 192 << 20                                  # the packed blob alone is 64 MiB
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
I64, F32 = torch.int64, torch.float32


def flags(precision):
    return _native.FLAG_INCLUDE_SELF | _native.PRECISIONS[precision]         # the shipped hyper-parameters: include_self only


@functools.lru_cache(maxsize=None)
def raw_weights():
    """the tensors the forward reads, in the order of the struct's fields as onepose_amd.gats_superglue packs them"""
    sd = synthetic.make_state_dict(0)
    keys = []
    for i, kind in enumerate(GNN_LAYER_NAMES):
        p = f"gnn.layers.{i}."
        if kind == "GATs":
            keys += [p + "W", p + "a"]
        else:
            keys += [p + sub + end for sub in ("attn.proj.0", "attn.proj.1", "attn.proj.2", "attn.merge", "mlp.0", "mlp.3") for end in (".weight", ".bias")]
    keys += ["final_proj.weight", "final_proj.bias"]
    assert len(keys) == 2 * _native.NUM_GATS + 12 * _native.NUM_ATTN + 2
    return [torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)) for k in keys]


def packed_weights(mem):
    """every raw tensor a piece of its own; the blob exactly gatsspg_packed_weights_bytes, written by gatsspg_pack_weights"""
    keep = [mem.place(t, "in", f"raw[{i}]") for i, t in enumerate(raw_weights())]      # alive until the pack has been enqueued
    it = iter([t.data_ptr() for t in keep])
    raw = _native.RawWeights()
    gi = ai = 0
    for kind in GNN_LAYER_NAMES:
        if kind == "GATs":
            raw.gats_W[gi], raw.gats_a[gi] = next(it), next(it)
            gi += 1
        else:
            for j in range(3):
                raw.proj_w[ai][j], raw.proj_b[ai][j] = next(it), next(it)
            raw.merge_w[ai], raw.merge_b[ai] = next(it), next(it)
            raw.mlp0_w[ai], raw.mlp0_b[ai] = next(it), next(it)
            raw.mlp3_w[ai], raw.mlp3_b[ai] = next(it), next(it)
            ai += 1
    raw.final_w, raw.final_b = next(it), next(it)
    nbytes = BINDING.load().gatsspg_packed_weights_bytes()
    assert nbytes > 0 and nbytes % 4 == 0
    packed = mem.place(torch.empty(nbytes // 4), "scratch", "packed")
    mem.call(BINDING, "gatsspg_pack_weights", ctypes.byref(raw), packed)
    return packed


def outputs(mem, b, n1, n2):
    return {nm: mem.place(torch.empty(s, dtype=t), "out", nm) for nm, s, t in
            (("conf", (b, n1, n2), F32), ("matches0", (b, n1), I64), ("matches1", (b, n2), I64), ("mscores0", (b, n1), F32), ("mscores1", (b, n2), F32))}


def workspace(mem, name, *shape):
    nbytes = BINDING.load().gatsspg_workspace_bytes(*shape)
    assert nbytes > 0
    return mem.place(nbytes, "scratch", name)


def inputs(b, n1, n2, num_leaf):
    data = synthetic.make_inputs(b=b, n1=n1, n2=n2, num_leaf=num_leaf, seed=n1 + n2)
    return {k: torch.from_numpy(data[k]) for k in ("descriptors2d_query", "descriptors3d_db", "descriptors2d_db")}


@pytest.mark.parametrize("precision", sorted(_native.PRECISIONS))
@pytest.mark.parametrize("b,n1,n2,num_leaf", SHAPES)
def test_pack_weights_and_forward(b, n1, n2, num_leaf, precision, run=run_placement):
    data = inputs(b, n1, n2, num_leaf)

    def body(mem):
        packed = packed_weights(mem)
        dq, d3, d2 = (mem.place(data[k], "in", k) for k in ("descriptors2d_query", "descriptors3d_db", "descriptors2d_db"))
        out = outputs(mem, b, n1, n2)
        ws = workspace(mem, "ws", b, n1, n2, num_leaf)
        mem.call(BINDING, "gatsspg_forward", packed, dq, d3, d2, b, n1, n2, num_leaf, flags(precision), SCALE, THRESHOLD, *out.values(), ws, ws.numel())
        return out                                         # (the blob is opaque: what it holds shows in the outputs)

    got = run(body, DEV, ROLES, capacity=CAPACITY)
    assert not torch.isnan(got["conf"]).any() and float(got["conf"].max()) > 0


@pytest.mark.parametrize("precision", sorted(_native.PRECISIONS))
@pytest.mark.parametrize("b,n1,n2,num_leaf", SHAPES)
def test_prepare_database_and_forward_cached(b, n1, n2, num_leaf, precision, run=run_placement):
    """The cache is written by gatsspg_prepare_database (its workspace: gatsspg_workspace_bytes(b, 2, n2, num_leaf), as the header says)
    and ``const`` in gatsspg_forward_cached, which gets a workspace of its own."""
    data = inputs(b, n1, n2, num_leaf)
    cache_bytes = BINDING.load().gatsspg_db_cache_bytes(b, n2)
    assert cache_bytes > 0 and cache_bytes % 4 == 0

    def body(mem):
        packed = packed_weights(mem)
        dq, d3, d2 = (mem.place(data[k], "in", k) for k in ("descriptors2d_query", "descriptors3d_db", "descriptors2d_db"))
        cache = mem.place(torch.empty(cache_bytes // 4), "scratch", "cache")
        ws_db = workspace(mem, "ws of prepare_database", b, 2, n2, num_leaf)
        mem.call(BINDING, "gatsspg_prepare_database", packed, d3, d2, b, n2, num_leaf, flags(precision), cache, cache_bytes, ws_db, ws_db.numel())
        out = outputs(mem, b, n1, n2)
        ws = workspace(mem, "ws", b, n1, n2, num_leaf)
        mem.call(BINDING, "gatsspg_forward_cached", packed, dq, d2, cache, cache_bytes, b, n1, n2, num_leaf, flags(precision), SCALE, THRESHOLD,
                 *out.values(), ws, ws.numel())
        return out

    got = run(body, DEV, ROLES, capacity=CAPACITY)
    assert not torch.isnan(got["conf"]).any() and float(got["conf"].max()) > 0


@pytest.mark.parametrize("precision", sorted(_native.PRECISIONS))
def test_forward_frames(precision, run=run_placement):
    """Frames of 2, 64 and 65 keypoints in one ragged call against a database of 65 points with 8 leaves.  The header refuses a
    count below 2 (as gatsspg_forward does: the reference raises for a single point), so the frame of 1 keypoint is replaced by the
    nearest the entry point takes.  The conf rows past a frame's count are "NOT WRITTEN"; matches0 / mscores0 there are -1 / 0."""
    counts, cap1, n2, num_leaf = (2, 64, 65), 65, 65, 8
    b = len(counts)
    data = inputs(b, cap1, n2, num_leaf)
    d3, d2 = data["descriptors3d_db"][:1].contiguous(), data["descriptors2d_db"][:1].contiguous()
    n1 = (ctypes.c_int32 * b)(*counts)
    cache_bytes = BINDING.load().gatsspg_db_cache_bytes(1, n2)
    assert cache_bytes > 0

    def body(mem):
        packed = packed_weights(mem)
        dq, db3, db2 = mem.place(data["descriptors2d_query"], "in", "desc2d_query"), mem.place(d3, "in", "desc3d_db"), mem.place(d2, "in", "desc2d_db")
        cache = mem.place(torch.empty(cache_bytes // 4), "scratch", "cache")
        ws_db = workspace(mem, "ws of prepare_database", 1, 2, n2, num_leaf)
        mem.call(BINDING, "gatsspg_prepare_database", packed, db3, db2, 1, n2, num_leaf, flags(precision), cache, cache_bytes, ws_db, ws_db.numel())
        out = outputs(mem, b, cap1, n2)
        ws = workspace(mem, "ws", b, cap1, n2, num_leaf)
        mem.call(BINDING, "gatsspg_forward_frames", packed, dq, n1, db2, cache, cache_bytes, b, cap1, n2, num_leaf, flags(precision), SCALE, THRESHOLD,
                 *out.values(), ws, ws.numel())
        return out, {"conf": torch.cat([out["conf"][i, :k].reshape(-1) for i, k in enumerate(counts)])}

    got = run(body, DEV, ROLES, capacity=CAPACITY)
    for i, k in enumerate(counts):
        assert not torch.isnan(got["conf"][i, :k]).any()
        assert bool((got["matches0"][i, k:] == -1).all()) and bool((got["mscores0"][i, k:] == 0).all())
        assert bool((got["conf"][i, k:].reshape(-1).view(torch.int32) == -1).all())          # still the first fill: every byte 0xFF


@pytest.mark.parametrize("name,inp_dim", [("kenc_2d", 3), ("kenc_3d", 4)])
@pytest.mark.parametrize("b,n", [(2, 7), (1, 257)])
def test_keypoint_encoder(b, n, name, inp_dim, run=run_placement):
    """gatsspg_keypoint_encoder, which no forward calls: both encoders of the module at 7 keypoints and at one over a block of 256.
    The weights are pieces of their own, reached through the host struct; the scratch is exactly gatsspg_kenc_scratch_bytes."""
    sd = synthetic.make_state_dict(0)
    weights = [torch.from_numpy(np.ascontiguousarray(sd[f"{name}.encoder.{j}.{kind}"])) for j in (0, 3, 6, 9) for kind in ("weight", "bias")]
    rs = np.random.RandomState(n + inp_dim)
    kpts, scores = rs.uniform(-1, 1, (b, n, inp_dim - 1)).astype(np.float32), rs.uniform(0, 1, (b, n)).astype(np.float32)
    nbytes = BINDING.load().gatsspg_kenc_scratch_bytes(b, n)
    assert nbytes > 0

    def body(mem):
        keep = [mem.place(t, "in", f"weights[{i}]") for i, t in enumerate(weights)]
        kw = _native.KencWeights()
        for j in range(4):
            kw.w[j], kw.b[j] = keep[2 * j].data_ptr(), keep[2 * j + 1].data_ptr()
        kw.inp_dim = inp_dim
        k, s = mem.place(torch.from_numpy(kpts), "in", "kpts"), mem.place(torch.from_numpy(scores), "in", "scores")
        out = mem.place(torch.empty(b, 256, n), "out", "out")
        scratch = mem.place(nbytes, "scratch", "scratch")
        mem.call(BINDING, "gatsspg_keypoint_encoder", ctypes.byref(kw), k, s, b, n, out, scratch, nbytes)
        return dict(out=out)

    got = run(body, DEV, ROLES, capacity=CAPACITY)
    assert not torch.isnan(got["out"]).any() and got["out"].any()


# every case again with each library call captured in a graph and replayed (arena.run_captured): the stream contract
test_pack_weights_and_forward_captured = captured_twin(test_pack_weights_and_forward)
test_prepare_database_and_forward_cached_captured = captured_twin(test_prepare_database_and_forward_cached)
test_forward_frames_captured = captured_twin(test_forward_frames)
test_keypoint_encoder_captured = captured_twin(test_keypoint_encoder)
