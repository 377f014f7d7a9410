"""MI355X-native nearest-neighbour matcher: host-side mirror of the reference module.

Drop-in for ``src/models/matchers/nn/nearest_neighbour.py::NearestNeighbour`` (reference :26-63): same constructor
(``NearestNeighbour(conf)``, the reference ``default_conf`` with ``conf`` merged over it), same ``forward(data) -> dict``
contract, no parameters.  The similarity, the top-2 selection of both directions, the ratio and distance tests and the
mutual check run as hand-written HIP kernels behind the C ABI of ``include/superglue/nn_matcher.h``; the n0 x n1 similarity
matrix is never written.  There is no PyTorch compute path and no CPU fallback.

Where the reference leaves the result open this module does not: on exactly equal similarities the lowest index wins
(``torch.topk`` does not say).  As in the reference, the mutual check rewrites ``matches0`` only -- ``matches1`` and both
score vectors keep what ``find_nn`` gave -- and ``match_threshold`` is accepted and unused.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _native_sg
from ._binding import Engine, gpu_tensor
from .superglue import OUT_KEYS, SuperGlueEngine, _host_i32, ragged_chunks, unpack_ragged

D = 256
NO_CPU = "onepose_amd.NearestNeighbour runs only on a ROCm GPU ({} on {}); there is no CPU fallback"


def _gpu(t, name):
    return gpu_tensor(t, torch.float32, NO_CPU.format(name + " is", "{}"))


class NearestNeighbourEngine(Engine):
    """Raw-tensor entry to the HIP matcher of one module: workspaces cached per (shape, device, stream), outputs may be
    preallocated (``out=``).  The uniform and the ragged entry points share one workspace cache under one key,
    (b, n0 | cap0, n1 | cap1); there are no weights to pack."""

    native = _native_sg
    WORKSPACE_BYTES, LAST_ERROR = "nnm_workspace_bytes", "sg_last_error"
    PARAMETER_REFUSAL = NO_CPU.format("a parameter is", "{}")
    MAX_CACHED_WORKSPACES = 12

    def workspace_refusal(self, shape):
        return "nnm_workspace_bytes({}, {}, {}) refused the shape".format(*shape)

    outputs = staticmethod(SuperGlueEngine.outputs)     # (matches0 int64, matches1 int64, matching_scores0, matching_scores1)

    def _tests(self):
        ratio, distance = self.module.thresholds()
        return ratio, distance, int(bool(self.module.conf["do_mutual_check"]))

    @staticmethod
    def _check_out(out, b, n0, n1):
        for x, cap, name in zip(out, (n0, n1, n0, n1), OUT_KEYS):
            if x.shape != (b, cap) or not x.is_contiguous():
                raise ValueError(f"out: {name} must be a contiguous [{b}, {cap}] tensor")
        return tuple(out)

    def forward(self, desc0, desc1, out=None):
        """desc0 [b,256,n0], desc1 [b,256,n1] on one GPU -> (matches0 int64 [b,n0], matches1 int64 [b,n1], matching_scores0
        [b,n0], matching_scores1 [b,n1]).  A batch of more than 64 pairs goes through the library 64 at a time."""
        d0, d1 = _gpu(desc0, "descriptors0"), _gpu(desc1, "descriptors1")
        self.module.check_shapes(d0, d1)
        if d1.device != d0.device:
            raise ValueError(f"descriptors1 is on {d1.device}, expected {d0.device}")
        b, n0, n1 = d0.shape[0], d0.shape[2], d1.shape[2]
        dev = d0.device
        out = self._check_out(out, b, n0, n1) if out is not None else self.outputs(b, n0, n1, dev)
        step = _native_sg.NNM_MAX_ITEMS
        for k in range(0, b, step):
            c = min(step, b - k)
            ws = self.workspace(c, n0, n1, dev)
            self.call("nnm_match", dev, d0[k:k + c], d1[k:k + c], c, n0, n1, *self._tests(), *(o[k:k + c] for o in out), ws, ws.numel(), 0)
        return out

    def match_ragged(self, desc0, desc1, n0, n1, out=None):
        """b <= 64 pairs in one chain of launches: desc0 [b,256,cap0]; desc1 [b,256,cap1], or ONE plane [256,cap1] that every
        item reads (the detector's query frame); host lists n0, n1 (1 <= n <= cap).  Returns the four outputs padded to
        [b,cap0] / [b,cap1], -1 / 0 past an item's count; every item is bitwise what ``forward`` gives on that pair alone."""
        d0, d1 = _gpu(desc0, "descriptors0"), _gpu(desc1, "descriptors1")
        shared = d1.dim() == 2
        if d0.dim() != 3 or d0.shape[1] != D or d1.shape[-2] != D or (not shared and (d1.dim() != 3 or d1.shape[0] != d0.shape[0])):
            raise ValueError("descriptors0 must be [b,256,cap0] and descriptors1 [b,256,cap1] or one shared [256,cap1]")
        if d1.device != d0.device:
            raise ValueError(f"descriptors1 is on {d1.device}, expected {d0.device}")
        b, cap0, cap1 = d0.shape[0], d0.shape[2], d1.shape[-1]
        dev = d0.device
        sizes = (_host_i32(n0, b, 1, "n0"), _host_i32(n1, b, 1, "n1"))
        ratio = self._tests()[0]
        if ratio and (min(sizes[0]) < 2 or min(sizes[1]) < 2):
            raise ValueError(self.module.ONE_POINT)
        out = self._check_out(out, b, cap0, cap1) if out is not None else self.outputs(b, cap0, cap1, dev)
        ws = self.workspace(b, cap0, cap1, dev)
        self.call("nnm_match_ragged", dev, d0, d1, *sizes, b, cap0, cap1, int(shared), *self._tests(), *out, ws, ws.numel(), 0)
        return out

    def similarity(self, desc0, desc1):
        """Stage (tests): desc0 [256,n0], desc1 [256,n1] -> desc0^T desc1 [n0,n1] through the pack and the main loop of the matcher."""
        d0, d1 = _gpu(desc0, "descriptors0"), _gpu(desc1, "descriptors1")
        if d0.dim() != 2 or d1.dim() != 2 or d0.shape[0] != D or d1.shape[0] != D:
            raise ValueError("similarity takes descriptors [256,n0] and [256,n1]")
        n0, n1 = d0.shape[1], d1.shape[1]
        ws = self.workspace(1, n0, n1, d0.device)
        sim = torch.empty(n0, n1, device=d0.device, dtype=torch.float32)
        self.call("nnm_similarity", d0.device, d0, d1, n0, n1, sim, ws, ws.numel(), 0)
        return sim


class NearestNeighbour(nn.Module):
    """Nearest-neighbour descriptor matching (reference :26-63) on HIP kernels."""

    default_conf = {
        "match_threshold": None,
        "ratio_threshold": None,
        "distance_threshold": None,
        "do_mutual_check": True,
    }
    ONE_POINT = "the ratio test needs a second neighbour: both sides must have at least 2 points (topk(2) raises in the reference)"

    def __init__(self, conf=None):
        super().__init__()
        self.conf = {**self.default_conf, **conf} if conf else dict(self.default_conf)
        self.thresholds()
        self._engine = None

    def thresholds(self):
        """(ratio, distance) as the library takes them: 0.0 where the reference's ``if ratio_thresh:`` skips the test."""
        out = []
        for key in ("ratio_threshold", "distance_threshold"):
            v = self.conf[key]
            v = float(v) if v else 0.0
            if math.isnan(v) or math.isinf(v) or v < 0:
                raise ValueError(f"{key} must be a finite number >= 0 or None (got {self.conf[key]!r})")
            out.append(v)
        return tuple(out)

    @property
    def engine(self):
        if self._engine is None:
            self._engine = NearestNeighbourEngine(self)
        return self._engine

    def check_shapes(self, d0, d1):
        """What can be refused from the shapes alone, on any device."""
        if d0.dim() != 3 or d1.dim() != 3 or d0.shape[0] != d1.shape[0]:
            raise ValueError("descriptors0 must be [b,256,n] and descriptors1 [b,256,m] with one b")
        if d0.shape[1] != D or d1.shape[1] != D:
            raise ValueError(f"onepose_amd.NearestNeighbour supports descriptor dimension {D} only (got {d0.shape[1]} and {d1.shape[1]})")
        if d0.shape[0] == 0 or d0.shape[2] == 0 or d1.shape[2] == 0:
            raise ValueError("a side with no point has no nearest neighbour (the reference's topk raises too)")
        if self.thresholds()[0] and (d0.shape[2] < 2 or d1.shape[2] < 2):
            raise ValueError(self.ONE_POINT)

    @torch.no_grad()
    def forward(self, data):
        """Match descriptors0 [b,256,n] against descriptors1 [b,256,m] (reference :41-63)."""
        d0, d1 = data["descriptors0"], data["descriptors1"]
        self.check_shapes(d0, d1)
        if not d0.is_cuda:
            raise RuntimeError(NO_CPU.format("the inputs are", d0.device))
        return dict(zip(OUT_KEYS, self.engine.forward(d0, d1)))

    @torch.no_grad()
    def match_pairs(self, items, max_items=16):
        """``forward`` on a list of pairs (``data`` dicts with b = 1 and any point counts; only the descriptors are read) ->
        list of the dicts ``forward`` returns, bitwise the same values.  The pairs go through the ragged batch ``max_items``
        (at most 64) at a time; a chunk of one pair goes through ``forward``."""
        items = list(items)
        for i, data in enumerate(items):
            if data["descriptors0"].shape[0] != 1 or data["descriptors1"].shape[0] != 1:
                raise ValueError(f"item {i}: match_pairs takes pairs with batch size 1")
            self.check_shapes(data["descriptors0"], data["descriptors1"])
            if not data["descriptors0"].is_cuda:
                raise RuntimeError(NO_CPU.format(f"item {i} is", data["descriptors0"].device))
        results = [None] * len(items)
        for chunk in ragged_chunks(list(range(len(items))), max_items):
            if len(chunk) == 1:
                results[chunk[0]] = self.forward(items[chunk[0]])
                continue
            n0 = [int(items[i]["descriptors0"].shape[2]) for i in chunk]
            n1 = [int(items[i]["descriptors1"].shape[2]) for i in chunk]
            ref = items[chunk[0]]["descriptors0"]
            p0 = ref.new_zeros((len(chunk), D, max(n0)), dtype=torch.float32)
            p1 = ref.new_zeros((len(chunk), D, max(n1)), dtype=torch.float32)
            for k, i in enumerate(chunk):
                p0[k, :, :n0[k]].copy_(items[i]["descriptors0"][0])
                p1[k, :, :n1[k]].copy_(items[i]["descriptors1"][0])
            out = self.engine.match_ragged(p0, p1, n0, n1)
            for i, res in zip(chunk, unpack_ragged(dict(zip(OUT_KEYS, out)), n0, n1)):
                results[i] = res
        return results
