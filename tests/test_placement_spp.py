"""Placement tests of the SuperPoint extractor (include/superpoint.h): spp_pack_weights and spp_forward with every device argument
an exact piece of a guarded arena (tests/arena.py) under the fills 0xFF and 0x00; the blob is exactly spp_packed_weights_bytes, the
workspace exactly spp_workspace_bytes.  Image shapes: the smallest map shapes of tests/spp_cases.py -- 8 x 8 (DESC_SHAPES), 16 x 24
with b = 2 (border_case), 72 x 104 and 88 x 80 (QUANT_SHAPES: more than one NMS tile on both axes) -- in both arithmetics of the GEMM
convolutions; the split form spp_dense -> spp_detect at the two smallest.  Every case runs a second time with each call captured and
replayed (arena.run_captured).  Bitwise comparisons only; the oracle comparisons stay in tests/test_spp_*.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import spp_cases as sc
from arena import captured_twin, run_placement
from onepose_amd import _native_spp, synthetic

BINDING = _native_spp
ROLES = {
    "spp_pack_weights": dict(packed="scratch"),           # (raw is a HOST struct of device pointers: the tensors it names are pieces)
    "spp_forward": dict(packed="in", image="in", keypoints="out", scores="out", descriptors="out", counts="out", workspace="scratch"),
    "spp_dense": dict(packed="in", image="in", score_map="out", dense_desc="out", workspace="scratch"),
    "spp_detect": dict(score_map="in", dense_desc="in", keypoints="out", scores="out", descriptors="out", counts="out", nms_out="out",
                       workspace="scratch"),
}
SHAPES = [(1,) + sc.DESC_SHAPES[0], (2, 16, 24), (1,) + sc.QUANT_SHAPES[0], (1,) + sc.QUANT_SHAPES[1]]
NMS_RADIUS, THRESHOLD, BORDER = 3, 0.005, 4           # the reference's defaults (superpoint.py:104-110)
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32 = torch.float32


@functools.lru_cache(maxsize=None)
def raw_weights():
    sd = synthetic.make_spp_state_dict(0)
    return [torch.from_numpy(np.ascontiguousarray(sd[f"{n}.{kind}"])) for kind in ("weight", "bias") for n in _native_spp.LAYER_NAMES]


def packed_weights(mem):
    """every raw tensor a piece of its own; the blob exactly spp_packed_weights_bytes, written by spp_pack_weights"""
    keep = [mem.place(t, "in", f"raw[{i}]") for i, t in enumerate(raw_weights())]
    raw = _native_spp.RawWeights()
    for i in range(_native_spp.NUM_LAYERS):
        raw.weight[i], raw.bias[i] = keep[i].data_ptr(), keep[_native_spp.NUM_LAYERS + i].data_ptr()
    nbytes = BINDING.load().spp_packed_weights_bytes()
    assert nbytes > 0 and nbytes % 4 == 0
    packed = mem.place(torch.empty(nbytes // 4), "scratch", "packed")
    mem.call(BINDING, "spp_pack_weights", ctypes.byref(raw), packed)
    return packed


@pytest.mark.parametrize("precision", sorted(_native_spp.PRECISIONS))
@pytest.mark.parametrize("max_keypoints", [-1, 16], ids=["keep_all", "top16"])
@pytest.mark.parametrize("b,H,W", SHAPES)
def test_pack_weights_and_forward(b, H, W, max_keypoints, precision, run=run_placement):
    """keep-all at a capacity of H W (every pixel could be a keypoint) and the top 16 at a capacity of 16.  Border 4 leaves nothing of
    an 8 x 8 image: counts [0, 0] and no slot written."""
    image = torch.from_numpy(synthetic.make_image(b, H, W, 5))
    cap = H * W if max_keypoints < 0 else max_keypoints
    nbytes = BINDING.load().spp_workspace_bytes(b, H, W)
    assert nbytes > 0

    def body(mem):
        packed = packed_weights(mem)
        img = mem.place(image, "in", "image")
        out = {nm: mem.place(torch.empty(s, dtype=t), "out", nm) for nm, s, t in
               (("keypoints", (b, cap, 2), F32), ("scores", (b, cap), F32), ("descriptors", (b, 256, cap), F32), ("counts", (b, 2), torch.int32))}
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "spp_forward", packed, img, b, H, W, NMS_RADIUS, THRESHOLD, max_keypoints, BORDER, 1, cap, *out.values(), ws, nbytes,
                 _native_spp.PRECISIONS[precision])
        n = out["counts"][:, 0].tolist()
        # only the first counts[i][0] slots of image i are defined (the header: "keypoints written")
        part = {"keypoints": torch.cat([out["keypoints"][i, :k].reshape(-1) for i, k in enumerate(n)]),
                "scores": torch.cat([out["scores"][i, :k] for i, k in enumerate(n)]),
                "descriptors": torch.cat([out["descriptors"][i, :, :k].reshape(-1) for i, k in enumerate(n)])}
        return out, part                                   # (the blob is opaque: what it holds shows in the outputs)

    got = run(body, DEV, ROLES)
    counts = got["counts"].tolist()
    assert all(0 <= k <= min(cap, c) for k, c in counts) and (min(H, W) <= 2 * BORDER or all(k > 0 for k, _ in counts))


@pytest.mark.parametrize("precision", sorted(_native_spp.PRECISIONS))
@pytest.mark.parametrize("max_keypoints", [-1, 16], ids=["keep_all", "top16"])
@pytest.mark.parametrize("b,H,W", SHAPES[:2])
def test_dense_then_detect(b, H, W, max_keypoints, precision, run=run_placement):
    """The split form of spp_forward at the two smallest shapes: spp_dense writes the score map and the dense descriptors, spp_detect
    takes them as ``const`` and writes the NMS map as well.  One workspace of spp_workspace_bytes(b, H, W) serves both."""
    image = torch.from_numpy(synthetic.make_image(b, H, W, 5))
    cap = H * W if max_keypoints < 0 else max_keypoints
    Hs, Ws = H // 8 * 8, W // 8 * 8
    nbytes = BINDING.load().spp_workspace_bytes(b, H, W)
    assert nbytes > 0

    def body(mem):
        packed = packed_weights(mem)
        img = mem.place(image, "in", "image")
        dense = {nm: mem.place(torch.empty(s, dtype=F32), "out", nm) for nm, s in (("score_map", (b, Hs, Ws)), ("dense_desc", (b, 256, H // 8, W // 8)))}
        out = {nm: mem.place(torch.empty(s, dtype=t), "out", nm) for nm, s, t in
               (("keypoints", (b, cap, 2), F32), ("scores", (b, cap), F32), ("descriptors", (b, 256, cap), F32), ("counts", (b, 2), torch.int32),
                ("nms_out", (b, Hs, Ws), F32))}
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "spp_dense", packed, img, b, H, W, *dense.values(), ws, nbytes, _native_spp.PRECISIONS[precision])
        mem.call(BINDING, "spp_detect", *dense.values(), b, Hs, Ws, NMS_RADIUS, THRESHOLD, max_keypoints, BORDER, 1, cap, *out.values(), ws, nbytes)
        n = out["counts"][:, 0].tolist()
        part = {"keypoints": torch.cat([out["keypoints"][i, :k].reshape(-1) for i, k in enumerate(n)]),
                "scores": torch.cat([out["scores"][i, :k] for i, k in enumerate(n)]),
                "descriptors": torch.cat([out["descriptors"][i, :, :k].reshape(-1) for i, k in enumerate(n)])}
        return {**dense, **out}, part

    got = run(body, DEV, ROLES)
    counts = got["counts"].tolist()
    assert all(0 <= k <= min(cap, c) for k, c in counts) and (min(H, W) <= 2 * BORDER or all(k > 0 for k, _ in counts))
    assert not torch.isnan(got["score_map"]).any() and float(got["score_map"].min()) >= 0


# every case again with each library call captured in a graph and replayed (arena.run_captured): the stream contract
test_pack_weights_and_forward_captured = captured_twin(test_pack_weights_and_forward)
test_dense_then_detect_captured = captured_twin(test_dense_then_detect)
