"""MI355X-native SuperGlue 2D-2D matcher: host-side mirror of the reference module.

Drop-in for ``src/models/matchers/SuperGlue/superglue.py::SuperGlue`` (reference :173-276): same constructor
(``SuperGlue(config)``, the reference ``default_config`` merged with ``config``), same submodule tree and
``state_dict`` keys (``superglue_outdoor.pth`` loads with ``strict=True``), same ``forward(data) -> dict`` contract.
Every stage runs as hand-written HIP kernels behind the C ABI of ``include/superglue/superglue.h``; the
modules below are parameter containers.  There is no PyTorch compute path and no CPU fallback.
Inference only: BatchNorm uses its running statistics and ``forward`` in training mode raises.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _native_sg
from ._binding import Engine, gpu_tensor

D = 256
HEADS = 4
KENC_LAYERS = [32, 64, 128, 256]


def _mlp(channels):
    """Conv1d(k=1) + BatchNorm1d + ReLU between every pair of widths, a bare Conv1d last (reference MLP layout, :47-59)."""
    mods = []
    for i in range(1, len(channels)):
        mods.append(nn.Conv1d(channels[i - 1], channels[i], kernel_size=1, bias=True))
        if i < len(channels) - 1:
            mods += [nn.BatchNorm1d(channels[i]), nn.ReLU()]
    return nn.Sequential(*mods)


class _KeypointEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = _mlp([3] + KENC_LAYERS + [D])


class _MultiHeadedAttention(nn.Module):
    def __init__(self):
        super().__init__()
        self.merge = nn.Conv1d(D, D, kernel_size=1)
        self.proj = nn.ModuleList([nn.Conv1d(D, D, kernel_size=1) for _ in range(3)])


class _AttentionalPropagation(nn.Module):
    def __init__(self):
        super().__init__()
        self.attn = _MultiHeadedAttention()
        self.mlp = _mlp([2 * D, 2 * D, D])


class _AttentionalGNN(nn.Module):
    def __init__(self, names):
        super().__init__()
        self.layers = nn.ModuleList([_AttentionalPropagation() for _ in names])
        self.names = list(names)


NO_CPU = "onepose_amd.SuperGlue runs only on a ROCm GPU ({} on {}); there is no CPU fallback"


def _gpu(t, name):
    return gpu_tensor(t, torch.float32, NO_CPU.format(name + " is", "{}"))


IN_KEYS = ("keypoints0", "scores0", "descriptors0", "keypoints1", "scores1", "descriptors1")
OUT_KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1")


def _point_axis(key):
    return 2 if key.startswith("descriptors") else 1


def pack_ragged(items):
    """A list of reference-shaped ``data`` dicts with b = 1 (keypoints [1,n,2], scores [1,n], descriptors [1,256,n], image
    [1,1,H,W] per side) -> one dict for ``SuperGlueEngine.forward_ragged``: the six inputs zero-padded to the largest count
    of each side (at least 1), plus the host lists ``n0`` / ``n1`` (counts) and ``hw0`` / ``hw1`` ((H, W) per item).
    Pure tensor bookkeeping: works on CPU tensors, launches nothing."""
    if not items:
        raise ValueError("pack_ragged needs at least one item")
    b = len(items)
    out = {"n0": [int(d["keypoints0"].shape[1]) for d in items], "n1": [int(d["keypoints1"].shape[1]) for d in items],
           "hw0": [tuple(int(x) for x in d["image0"].shape[-2:]) for d in items],
           "hw1": [tuple(int(x) for x in d["image1"].shape[-2:]) for d in items]}
    ref = items[0]["keypoints0"]
    for key in IN_KEYS:
        cap = max(1, max(out["n" + key[-1]]))
        shape = {"keypoints": (b, cap, 2), "scores": (b, cap), "descriptors": (b, D, cap)}[key[:-1]]
        padded = ref.new_zeros(shape, dtype=torch.float32)
        for i, d in enumerate(items):
            t = d[key]
            if t.shape[0] != 1:
                raise ValueError(f"item {i}: {key} must have batch size 1 (got {t.shape[0]})")
            padded[i].narrow(_point_axis(key) - 1, 0, out["n" + key[-1]][i]).copy_(t[0])
        out[key] = padded
    return out


def unpack_ragged(padded, n0, n1):
    """Per-item views of padded tensors, cut to each item's own counts: ``padded`` maps names ending in 0 / 1 (the inputs of
    ``pack_ragged``, the outputs of ``forward_ragged``) to [b, ...] tensors -> list of b dicts of [1, ...] views."""
    counts = {"0": n0, "1": n1}
    return [{key: t[i:i + 1].narrow(_point_axis(key), 0, counts[key[-1]][i]) for key, t in padded.items()}
            for i in range(len(n0))]


def ragged_chunks(items, max_items):
    """``items`` in order, in lists of at most ``max_items`` (itself at most SG_MAX_ITEMS)."""
    if not 1 <= max_items <= _native_sg.MAX_ITEMS:
        raise ValueError(f"max_items must be in [1, {_native_sg.MAX_ITEMS}] (got {max_items})")
    return [items[k:k + max_items] for k in range(0, len(items), max_items)]


def _host_i32(values, b, width, name):
    flat = [int(x) for row in values for x in (row if width > 1 else (row,))]
    if len(flat) != b * width:
        raise ValueError(f"{name} must have {b} entries" + (f" of {width}" if width > 1 else ""))
    return (ctypes.c_int32 * len(flat))(*flat)


class SuperGlueEngine(Engine):
    """Raw-tensor entry to the HIP matcher of one module: packed weights once per weight version and device, workspaces
    cached per (shape, device, stream) so one module serves several streams at once.  Outputs may be preallocated
    (``out=``) by callers that keep frames in flight.  The uniform and the ragged entry points share their validation and
    one workspace cache."""

    native = _native_sg
    WORKSPACE_BYTES, LAST_ERROR = "sg_workspace_bytes", "sg_last_error"
    PARAMETER_REFUSAL = NO_CPU.format("a parameter is", "{}") + " -- move the module to the GPU"
    MAX_CACHED_WORKSPACES = 12          # six uniform and six ragged shapes: one key, (b, n0 | cap0, n1 | cap1), and one size

    def _raw_tensors(self):
        """Every float tensor of the state_dict in its order, read through getattr on every call."""
        return [getattr(sub, name) for sub, name in self.module._raw_slots]

    def _pack(self, keep):
        n_layers = self.module.n_layers
        ptrs = (ctypes.c_void_p * len(keep))(*[k.data_ptr() for k in keep])
        packed = torch.empty(self.lib.sg_packed_weights_bytes(n_layers) // 4, device=keep[0].device, dtype=torch.float32)
        self.call("sg_pack_weights", packed.device, ptrs, n_layers, packed)
        return packed

    def workspace_refusal(self, shape):
        return "sg_workspace_bytes({}, {}, {}) refused the shape".format(*shape)

    def ragged_workspace(self, b, cap0, cap1, device):
        """``workspace`` under the ragged limits (b <= 64): the same bytes in the same cache under the same key."""
        return self._workspaces.get((b, cap0, cap1), device, self.lib.sg_ragged_workspace_bytes,
                                    lambda: f"sg_ragged_workspace_bytes({b}, {cap0}, {cap1}) refused the shape")

    @staticmethod
    def outputs(b, n0, n1, device):
        """(matches0 int64 [b,n0], matches1 int64 [b,n1], matching_scores0 [b,n0], matching_scores1 [b,n1])."""
        return (torch.empty(b, n0, device=device, dtype=torch.int64), torch.empty(b, n1, device=device, dtype=torch.int64),
                torch.empty(b, n0, device=device, dtype=torch.float32), torch.empty(b, n1, device=device, dtype=torch.float32))

    def _validate(self, inputs, out, z_out, n):
        """The six inputs, ``out=`` and ``z_out`` of ``forward`` (n = "n") and ``forward_ragged`` (n = "cap"): the inputs as fp32
        contiguous tensors of one GPU and of consistent shapes, the buffers of the right shape and contiguous.  The dtype of
        the ``out=`` buffers is checked where they enter the library.  -> (the six tensors, b, n0 | cap0, n1 | cap1)."""
        t = [_gpu(x, key) for x, key in zip(inputs, IN_KEYS)]
        k0, s0, d0, k1, s1, d1 = t
        for x, key in zip(t, IN_KEYS):
            if x.device != k0.device:
                raise ValueError(f"{key} is on {x.device}, expected {k0.device}")
        b, n0, n1 = k0.shape[0], k0.shape[1], k1.shape[1]
        if d0.shape != (b, D, n0) or d1.shape != (b, D, n1) or s0.shape != (b, n0) or s1.shape != (b, n1) or k1.shape[0] != b:
            raise ValueError(f"inconsistent shapes: keypoints [b,{n},2], scores [b,{n}], descriptors [b,256,{n}] with one b")
        for x, cap, name in zip(out or (), (n0, n1, n0, n1), OUT_KEYS):
            if x.shape != (b, cap) or not x.is_contiguous():
                raise ValueError(f"out: {name} must be a contiguous [{b}, {cap}] tensor")
        if z_out is not None and (z_out.shape != (b, n0 + 1, n1 + 1) or z_out.dtype != torch.float32 or not z_out.is_contiguous()):
            raise ValueError(f"z_out must be a contiguous fp32 [b, {n}0+1, {n}1+1] tensor")
        return t, b, n0, n1

    def _head(self, dev, t, b, n0, n1):
        """The arguments sg_forward and sg_forward_ragged begin with."""
        cfg = self.module.config
        kinds = (ctypes.c_int32 * max(1, self.module.n_layers))(*self.module.layer_kinds)
        return (self.packed_weights(dev), self.module.n_layers, kinds, int(cfg["sinkhorn_iterations"]), float(cfg["match_threshold"]),
                *t, b, n0, n1)

    def forward(self, kpts0, scores0, desc0, kpts1, scores1, desc1, hw0, hw1, out=None, z_out=None):
        """kpts [b,n,2], scores [b,n], desc [b,256,n] on one GPU; hw = (H, W) of each image.  Returns the four outputs."""
        t, b, n0, n1 = self._validate((kpts0, scores0, desc0, kpts1, scores1, desc1), out, z_out, "n")
        dev = t[0].device
        ws = self.workspace(b, n0, n1, dev)
        out = tuple(out) if out is not None else self.outputs(b, n0, n1, dev)
        self.call("sg_forward", dev, *self._head(dev, t, b, n0, n1), int(hw0[0]), int(hw0[1]), int(hw1[0]), int(hw1[1]), *out, z_out,
                  ws, ws.numel())
        return out

    def forward_ragged(self, kpts0, scores0, desc0, kpts1, scores1, desc1, n0, n1, hw0, hw1, out=None, z_out=None):
        """b pairs in one chain of launches: inputs padded to [b,cap0,2] / [b,cap0] / [b,256,cap0] (and cap1), host lists
        n0, n1 (1 <= n <= cap) and hw0, hw1 ((H, W) per item).  Returns the four outputs padded to [b,cap0] / [b,cap1], -1 / 0
        past an item's count; every item is bitwise what ``forward`` gives on that pair alone.  z_out: [b,cap0+1,cap1+1]."""
        t, b, cap0, cap1 = self._validate((kpts0, scores0, desc0, kpts1, scores1, desc1), out, z_out, "cap")
        dev = t[0].device
        sizes = (_host_i32(n0, b, 1, "n0"), _host_i32(n1, b, 1, "n1"), _host_i32(hw0, b, 2, "hw0"), _host_i32(hw1, b, 2, "hw1"))
        out = tuple(out) if out is not None else self.outputs(b, cap0, cap1, dev)
        ws = self.ragged_workspace(b, cap0, cap1, dev)
        self.call("sg_forward_ragged", dev, *self._head(dev, t, b, cap0, cap1), *sizes, *out, z_out, ws, ws.numel())
        return out

    # ---- stages (tests): a uniform stage and its ragged variant (per-item counts as host lists) share their validation ----
    def keypoint_encode(self, kpts0, scores0, desc0, kpts1, scores1, desc1, hw0, hw1):
        t = [_gpu(x, "input") for x in (kpts0, scores0, desc0, kpts1, scores1, desc1)]
        dev = t[0].device
        b, n0, n1 = t[0].shape[0], t[0].shape[1], t[3].shape[1]
        ws = self.workspace(b, n0, n1, dev)
        o0, o1 = torch.empty_like(t[2]), torch.empty_like(t[5])
        self.call("sg_keypoint_encode", dev, self.packed_weights(dev), self.module.n_layers, *t, b, n0, n1, int(hw0[0]), int(hw0[1]),
                  int(hw1[0]), int(hw1[1]), o0, o1, ws, ws.numel())
        return o0, o1

    def layer(self, index, desc0, desc1):
        d0, d1 = _gpu(desc0, "desc0"), _gpu(desc1, "desc1")
        dev = d0.device
        b, n0, n1 = d0.shape[0], d0.shape[2], d1.shape[2]
        ws = self.workspace(b, n0, n1, dev)
        o0, o1 = torch.empty_like(d0), torch.empty_like(d1)
        self.call("sg_layer", dev, self.packed_weights(dev), self.module.n_layers, index, self.module.layer_kinds[index], d0, d1,
                  b, n0, n1, o0, o1, ws, ws.numel())
        return o0, o1

    @staticmethod
    def _q_kv(q, kv, n, m):
        qq, kk = _gpu(q, "q"), _gpu(kv, "kv")
        if qq.dim() != 3 or kk.dim() != 3 or qq.shape[1] != D or kk.shape[1] != 2 * D or kk.shape[0] != qq.shape[0]:
            raise ValueError(f"q must be [b,256,{n}] and kv [b,512,{m}] with one b")
        return qq, kk, qq.shape[0]

    def attention(self, q, kv):
        """Softmax attention of the layers' kernel on head-contiguous q [b,256,N] and kv [b,512,M] (k rows, then v rows);
        returns [b,256,N]: per head h, out[h*64+d] = sum_m softmax_m(q_h . k_h[:, m] / 8) v[h*64+d, m]."""
        qq, kk, b = self._q_kv(q, kv, "N", "M")
        out = torch.empty_like(qq)
        self.call("sg_attention", qq.device, qq, kk, b, qq.shape[2], kk.shape[2], out)
        return out

    def attention_ragged(self, q, kv, n, m):
        """``attention`` on q [b,256,capN], kv [b,512,capM] with per-item counts n, m (host lists); columns past n[i] of
        the result are not written."""
        qq, kk, b = self._q_kv(q, kv, "capN", "capM")
        out = torch.zeros_like(qq)
        self.call("sg_attention_ragged", qq.device, qq, kk, b, qq.shape[2], kk.shape[2], _host_i32(n, b, 1, "n"),
                  _host_i32(m, b, 1, "m"), out)
        return out

    @staticmethod
    def _scores(scores, bin_score):
        sc = _gpu(scores, "scores")
        return sc, torch.as_tensor(bin_score, dtype=torch.float32, device=sc.device).reshape(1), sc.device, sc.shape

    def sinkhorn(self, scores, bin_score, iters):
        sc, alpha, dev, (b, n0, n1) = self._scores(scores, bin_score)
        ws = self.workspace(b, n0, n1, dev)
        z = torch.empty(b, n0 + 1, n1 + 1, device=dev, dtype=torch.float32)
        self.call("sg_sinkhorn", dev, sc, alpha, b, n0, n1, int(iters), z, ws, ws.numel())
        return z

    def sinkhorn_ragged(self, scores, bin_score, n0, n1, iters):
        """``sinkhorn`` on scores [b,cap0,cap1] with per-item counts -> z [b,cap0+1,cap1+1] (zero outside an item's block)."""
        sc, alpha, dev, (b, cap0, cap1) = self._scores(scores, bin_score)
        ws = self.ragged_workspace(b, cap0, cap1, dev)
        z = torch.zeros(b, cap0 + 1, cap1 + 1, device=dev, dtype=torch.float32)
        self.call("sg_sinkhorn_ragged", dev, sc, alpha, b, cap0, cap1, _host_i32(n0, b, 1, "n0"), _host_i32(n1, b, 1, "n1"),
                  int(iters), z, ws, ws.numel())
        return z

    def match_tail(self, z, match_threshold):
        zz = _gpu(z, "z")
        b, n0, n1 = zz.shape[0], zz.shape[1] - 1, zz.shape[2] - 1
        ws = self.workspace(b, n0, n1, zz.device)
        out = self.outputs(b, n0, n1, zz.device)
        self.call("sg_match_tail", zz.device, zz, b, n0, n1, float(match_threshold), *out, ws, ws.numel())
        return out

    def match_tail_ragged(self, z, n0, n1, match_threshold):
        zz = _gpu(z, "z")
        b, cap0, cap1 = zz.shape[0], zz.shape[1] - 1, zz.shape[2] - 1
        ws = self.ragged_workspace(b, cap0, cap1, zz.device)
        out = self.outputs(b, cap0, cap1, zz.device)
        self.call("sg_match_tail_ragged", zz.device, zz, b, cap0, cap1, _host_i32(n0, b, 1, "n0"), _host_i32(n1, b, 1, "n1"),
                  float(match_threshold), *out, ws, ws.numel())
        return out


class SuperGlue(nn.Module):
    """SuperGlue feature matching middle-end (reference :173-276) on HIP kernels, inference only."""

    default_config = {
        "descriptor_dim": 256,
        "weights": "indoor",
        "keypoint_encoder": [32, 64, 128, 256],
        "GNN_layers": ["self", "cross"] * 9,
        "sinkhorn_iterations": 100,
        "match_threshold": 0.2,
    }

    def __init__(self, config=None):
        super().__init__()
        self.config = {**self.default_config, **(config or {})}
        cfg = self.config
        if cfg["descriptor_dim"] != D:
            raise ValueError(f"onepose_amd.SuperGlue supports descriptor_dim={D} only (got {cfg['descriptor_dim']})")
        if list(cfg["keypoint_encoder"]) != KENC_LAYERS:
            raise ValueError(f"onepose_amd.SuperGlue supports keypoint_encoder={KENC_LAYERS} only (got {cfg['keypoint_encoder']})")
        if cfg.get("num_heads", HEADS) != HEADS:
            raise ValueError(f"onepose_amd.SuperGlue supports {HEADS} attention heads only")
        names = list(cfg["GNN_layers"])
        if any(n not in ("self", "cross") for n in names):
            raise ValueError("GNN_layers entries must be 'self' or 'cross'")
        if len(names) > 64:
            raise ValueError("at most 64 GNN layers")
        if int(cfg["sinkhorn_iterations"]) < 0:
            raise ValueError("sinkhorn_iterations must be >= 0")
        self.kenc = _KeypointEncoder()
        self.gnn = _AttentionalGNN(names)
        self.final_proj = nn.Conv1d(D, D, kernel_size=1, bias=True)
        self.register_parameter("bin_score", nn.Parameter(torch.tensor(1.0)))
        self.layer_kinds = [_native_sg.LAYER_CROSS if n == "cross" else _native_sg.LAYER_SELF for n in names]
        self.n_layers = len(names)
        self._raw_slots = []
        for key, val in self.state_dict(keep_vars=True).items():
            if key.endswith("num_batches_tracked"):
                continue
            path, _, name = key.rpartition(".")
            self._raw_slots.append((self.get_submodule(path) if path else self, name))
        assert len(self._raw_slots) == _native_sg.num_raw(self.n_layers)
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            self._engine = SuperGlueEngine(self)
        return self._engine

    @torch.no_grad()
    def forward(self, data):
        """Run SuperGlue on a pair of keypoints and descriptors (reference :207-276)."""
        if self.training:
            raise RuntimeError("onepose_amd.SuperGlue is inference only (BatchNorm running statistics, no backward): call .eval()")
        kpts0, kpts1 = data["keypoints0"], data["keypoints1"]
        if kpts0.shape[1] == 0 or kpts1.shape[1] == 0:   # no keypoints: nothing is launched (:221-231)
            shape0, shape1 = kpts0.shape[:-1], kpts1.shape[:-1]
            return {
                "matches0": kpts0.new_full(shape0, -1, dtype=torch.int),
                "matches1": kpts1.new_full(shape1, -1, dtype=torch.int),
                "matching_scores0": kpts0.new_zeros(shape0),
                "matching_scores1": kpts1.new_zeros(shape1),
            }
        if not kpts0.is_cuda:
            raise RuntimeError(NO_CPU.format("the inputs are", kpts0.device))
        hw0, hw1 = data["image0"].shape[-2:], data["image1"].shape[-2:]
        m0, m1, s0, s1 = self.engine.forward(kpts0, data["scores0"], data["descriptors0"], kpts1, data["scores1"],
                                             data["descriptors1"], hw0, hw1)
        return {"matches0": m0, "matches1": m1, "matching_scores0": s0, "matching_scores1": s1}

    @torch.no_grad()
    def match_pairs(self, items, max_items=16):
        """``forward`` on a list of pairs (``data`` dicts with b = 1, any keypoint counts and image sizes) -> list of the
        dicts ``forward`` returns, bitwise the same values.  The pairs go through the ragged batch ``max_items`` (at most 64)
        at a time; a pair with an empty side gets the empty result without entering the library, a chunk of one pair
        goes through ``forward``."""
        if self.training:
            raise RuntimeError("onepose_amd.SuperGlue is inference only (BatchNorm running statistics, no backward): call .eval()")
        items = list(items)
        results = [None] * len(items)
        live = []
        for i, data in enumerate(items):
            if data["keypoints0"].shape[0] != 1:
                raise ValueError(f"item {i}: match_pairs takes pairs with batch size 1")
            if data["keypoints0"].shape[1] == 0 or data["keypoints1"].shape[1] == 0:
                results[i] = self.forward(data)
            elif not data["keypoints0"].is_cuda:
                raise RuntimeError(NO_CPU.format(f"item {i} is", data["keypoints0"].device))
            else:
                live.append(i)
        for chunk in ragged_chunks(live, max_items):
            if len(chunk) == 1:
                results[chunk[0]] = self.forward(items[chunk[0]])
                continue
            p = pack_ragged([items[i] for i in chunk])
            out = self.engine.forward_ragged(*(p[k] for k in IN_KEYS), p["n0"], p["n1"], p["hw0"], p["hw1"])
            for i, res in zip(chunk, unpack_ragged(dict(zip(OUT_KEYS, out)), p["n0"], p["n1"])):
                results[i] = res
        return results
