"""MI355X-native SuperPoint extractor: host-side mirror of the reference module.

Drop-in for ``src/models/extractors/SuperPoint/superpoint.py::SuperPoint`` (reference :96-197): same
constructor (``SuperPoint(config)``), same parameter names / shapes (``conv1a.weight`` ...
``convDb.bias``; a reference ``superpoint_v1.pth`` loads with ``strict=True``), same ``forward(image)``
contract -- ``{'keypoints': [ [n,2] (x,y) float ], 'scores': [ [n] ], 'descriptors': [ [256,n] ]}``, one
list entry per image -- with every stage running as hand-written HIP kernels behind the C ABI of
``include/superpoint.h``.  The modules below are parameter containers; there is no PyTorch compute
path and no CPU fallback.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _native_spp
from ._binding import Engine, gpu_tensor

LAYERS = (  # (name, out, in, k) -- reference :115-133
    ("conv1a", 64, 1, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3),
    ("conv3a", 128, 64, 3), ("conv3b", 128, 128, 3), ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3),
    ("convPa", 256, 128, 3), ("convPb", 65, 256, 1), ("convDa", 256, 128, 3), ("convDb", 256, 256, 1),
)


NO_CPU = "onepose_amd.SuperPoint runs only on a ROCm GPU ({} is on {}); there is no CPU fallback"


class SuperPointEngine(Engine):
    """The packed weights and the workspaces (keyed (b, H, W), device; per stream, so one module can be used from several
    streams at once) of one module."""

    native = _native_spp
    WORKSPACE_BYTES, LAST_ERROR = "spp_workspace_bytes", "spp_last_error"
    PARAMETER_REFUSAL = NO_CPU.format("a parameter", "{}") + " -- move the module to the GPU"

    def _raw_tensors(self):
        m = self.module
        return [getattr(m, n).weight for n, *_ in LAYERS] + [getattr(m, n).bias for n, *_ in LAYERS]

    def _pack(self, keep):
        raw = _native_spp.RawWeights()
        for i in range(_native_spp.NUM_LAYERS):
            raw.weight[i], raw.bias[i] = keep[i].data_ptr(), keep[_native_spp.NUM_LAYERS + i].data_ptr()
        packed = torch.empty(self.lib.spp_packed_weights_bytes() // 4, device=keep[0].device, dtype=torch.float32)
        self.call("spp_pack_weights", packed.device, ctypes.byref(raw), packed)
        return packed

    def flags(self):
        return _native_spp.PRECISIONS[self.module.precision]

    # ---- stages (tests) ----
    def dense(self, image, workspace=None):
        b, _, h, w = image.shape
        dev = image.device
        ws = self.workspace(b, h, w, dev) if workspace is None else workspace
        score = torch.empty(b, h // 8 * 8, w // 8 * 8, device=dev, dtype=torch.float32)
        dense = torch.empty(b, 256, h // 8, w // 8, device=dev, dtype=torch.float32)
        self.call("spp_dense", dev, self.packed_weights(dev), image, b, h, w, score, dense, ws, ws.numel(), self.flags())
        return score, dense

    def dense_stage(self, image, stage, workspace=None, out=None):
        """One activation of the dense stack ([b, C, H >> k, W >> k]; ``_native_spp.DENSE_STAGES``) after exactly the launches
        ``dense`` makes up to it.  ``workspace``: a uint8 tensor of at least ``spp_workspace_bytes`` in place of the cached one."""
        b, _, h, w = image.shape
        dev = image.device
        ws = self.workspace(b, h, w, dev) if workspace is None else workspace
        c, k = _native_spp.DENSE_STAGES[stage]
        if out is None:
            out = torch.empty(b, c, h >> k, w >> k, device=dev, dtype=torch.float32)
        self.call("spp_dense_stage", dev, self.packed_weights(dev), image, b, h, w, stage, out, ws, ws.numel(), self.flags())
        return out

    def _outputs(self, b, capacity, dev):
        return (torch.empty(b, capacity, 2, device=dev, dtype=torch.float32),
                torch.empty(b, capacity, device=dev, dtype=torch.float32),
                torch.empty(b, 256, capacity, device=dev, dtype=torch.float32),
                torch.empty(b, 2, device=dev, dtype=torch.int32))

    def _capacity(self, cfg, h, w, capacity):
        if capacity is not None:
            return int(capacity)
        mk = cfg["max_keypoints"]
        # -1 = keep everything: NMS survivors are more than `radius` apart (plateaus aside); retried at H*W on overflow
        return mk if mk >= 0 else max(1024, (h * w) // ((cfg["nms_radius"] + 1) ** 2))

    def detect(self, score, dense, cfg, align_corners, capacity=None, return_nms=False):
        b, h, w = score.shape
        dev = score.device
        ws = self.workspace(b, h, w, dev)
        cap = self._capacity(cfg, h, w, capacity)
        kp, sc, de, cnt = self._outputs(b, cap, dev)
        nms = torch.empty_like(score) if return_nms else None
        self.call("spp_detect", dev, score, dense, b, h, w, cfg["nms_radius"], cfg["keypoint_threshold"], cfg["max_keypoints"],
                  cfg["remove_borders"], int(align_corners), cap, kp, sc, de, cnt, nms, ws, ws.numel())
        return kp, sc, de, cnt, nms

    def forward(self, image, cfg, align_corners, capacity=None):
        b, _, h, w = image.shape
        dev = image.device
        ws = self.workspace(b, h, w, dev)
        cap = self._capacity(cfg, h, w, capacity)
        kp, sc, de, cnt = self._outputs(b, cap, dev)
        self.call("spp_forward", dev, self.packed_weights(dev), image, b, h, w, cfg["nms_radius"], cfg["keypoint_threshold"],
                  cfg["max_keypoints"], cfg["remove_borders"], int(align_corners), cap, kp, sc, de, cnt, ws, ws.numel(), self.flags())
        return kp, sc, de, cnt


class SuperPoint(nn.Module):
    """SuperPoint detector / descriptor (reference :96-197) on HIP kernels.

    ``align_corners``: the reference picks it from ``int(torch.__version__[2]) > 2`` (:87) -- True on the torch
    1.x builds OnePose pins (its environment.yaml), which is the default here; pass False to reproduce what the
    same line yields on torch >= 1.10 / 2.x.

    ``precision`` (keyword, not part of the reference signature; also settable as an attribute): arithmetic of the GEMM
    convolutions -- ``"fp32"`` (default: exact fp32 MFMA, the reference's arithmetic) or ``"fp16x4"`` (two fp16 terms per operand,
    all four products: fp32-class results at a quarter of the matrix-pipe time; the matcher's mode of the same name).  It travels
    to the library as a bit of the ``flags`` argument of the C ABI; nothing is read from the environment."""

    default_config = {
        "descriptor_dim": 256,
        "nms_radius": 4,
        "keypoint_threshold": 0.005,
        "max_keypoints": -1,
        "remove_borders": 4,
    }

    def __init__(self, config=None, align_corners=True, precision="fp32"):
        super().__init__()
        self.precision = precision
        self.config = {**self.default_config, **(config or {})}
        if self.config["descriptor_dim"] != 256:
            raise ValueError("onepose_amd.SuperPoint supports descriptor_dim=256 (the reference default and the matcher's input)")
        for name, oc, ic, k in LAYERS:
            setattr(self, name, nn.Conv2d(ic, oc, kernel_size=k, stride=1, padding=k // 2))
        mk = self.config["max_keypoints"]
        if mk == 0 or mk < -1:
            raise ValueError('"max_keypoints" must be positive or "-1"')       # reference :135-137
        self.align_corners = bool(align_corners)
        self._engine = None

    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, value):
        if value not in _native_spp.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_native_spp.PRECISIONS)} (got {value!r})")
        self._precision = value

    @property
    def engine(self):
        if self._engine is None:
            self._engine = SuperPointEngine(self)
        return self._engine

    def _check_image(self, inp):
        if not isinstance(inp, torch.Tensor) or inp.dim() != 4 or inp.shape[1] != 1:
            raise ValueError("expected a grayscale image batch [b, 1, H, W]")
        return gpu_tensor(inp, torch.float32, NO_CPU.format("the image", "{}"))

    @torch.no_grad()
    def forward_device(self, inp, capacity=None):
        """Batched outputs left on the GPU without a host round trip: (keypoints [b,cap,2], scores [b,cap],
        descriptors [b,256,cap], counts int32 [b,2]); only the first counts[i,0] slots of image i are defined."""
        img = self._check_image(inp)
        return self.engine.forward(img, self.config, self.align_corners, capacity)

    @torch.no_grad()
    def forward(self, inp):
        """Compute keypoints, scores, descriptors for image (reference :140-197)."""
        img = self._check_image(inp)
        kp, sc, de, cnt = self.engine.forward(img, self.config, self.align_corners)
        counts = cnt.cpu()                       # the reference synchronises here too (torch.nonzero, :165)
        cap = kp.shape[1]
        if self.config["max_keypoints"] < 0 and int(counts[:, 1].max()) > cap:
            kp, sc, de, cnt = self.engine.forward(img, self.config, self.align_corners, capacity=img.shape[2] * img.shape[3])
            counts = cnt.cpu()
        out = {"keypoints": [], "scores": [], "descriptors": []}
        for i in range(img.shape[0]):
            n = int(counts[i, 0])
            out["keypoints"].append(kp[i, :n])
            out["scores"].append(sc[i, :n])
            out["descriptors"].append(de[i, :, :n])
        return out
