"""Drop-in ``GATsSuperGlue`` for the OnePose GATsSPG 2D-3D matcher, running on hand-written HIP
kernels (MI355X / gfx950) through the C ABI of libgatsspg_hip.so.

Mirrors the reference module's interface (src/models/GATsSPG_architectures/GATs_SuperGlue.py:143-241):
same constructor (``hparams`` mapping), same parameter names and shapes (so the ``matcher.*`` tensors
of a GATsSPG.ckpt load with ``strict=True``), same ``forward(data) -> (pred, conf_matrix)`` contract,
including the reference's quirks: ``pred`` carries batch element 0 only (:232-237), an empty side
returns a bare dict with int32 matches (:195-203), a single keypoint raises ``ValueError`` (what
``nn.InstanceNorm1d`` does in the reference, :126), the keypoint encoders and ``bin_score`` are
parameters that forward never uses (:150-160,176-177).

The sub-modules below are parameter containers; all arithmetic happens in the HIP library.  There is
no PyTorch / CPU fallback: tensors that are not on a ROCm device raise.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _native
from ._binding import Engine, gpu_tensor

D = 256
NUM_HEADS = 4
GNN_LAYER_NAMES = ["GATs", "self", "cross"] * 4  # GATs_SuperGlue.py:162


# --------------------------------------------------------------------------------------------------
# parameter containers (names/shapes = reference state_dict)
# --------------------------------------------------------------------------------------------------
class GraphAttentionLayer(nn.Module):
    """Parameters of GATs.py:25-28: W [in,out] (applied on the right, h @ W), a [2*out, 1]."""

    def __init__(self, in_features=D, out_features=D, alpha=0.2, include_self=True, additional=False,
                 with_linear_transform=True):
        super().__init__()
        self.alpha = alpha
        self.include_self, self.additional, self.with_linear_transform = include_self, additional, with_linear_transform
        self.W = nn.Parameter(torch.empty(in_features, out_features))
        self.a = nn.Parameter(torch.empty(2 * out_features, 1))
        nn.init.xavier_normal_(self.W.data, gain=1.414)
        nn.init.xavier_normal_(self.a.data, gain=1.414)


class MultiHeadedAttention(nn.Module):
    """merge + proj.{0,1,2} 1x1 convolutions (GATs_SuperGlue.py:85-91)."""

    def __init__(self, num_heads, d_model):
        super().__init__()
        assert d_model % num_heads == 0
        self.dim, self.num_heads = d_model // num_heads, num_heads
        self.merge = nn.Conv1d(d_model, d_model, kernel_size=1)
        self.proj = nn.ModuleList([nn.Conv1d(d_model, d_model, kernel_size=1) for _ in range(3)])
        for p in self.proj:  # the reference deep-copies merge three times (:91): identical initial values
            p.load_state_dict(self.merge.state_dict())


def _mlp(channels):
    """Conv1d / InstanceNorm1d / ReLU stack with the reference's Sequential indices (:116-128)."""
    layers = []
    for i in range(1, len(channels)):
        layers.append(nn.Conv1d(channels[i - 1], channels[i], kernel_size=1, bias=True))
        if i < len(channels) - 1:
            layers.append(nn.InstanceNorm1d(channels[i]))
            layers.append(nn.ReLU())
    return nn.Sequential(*layers)


class AttentionPropagation(nn.Module):
    def __init__(self, feature_dim, num_heads):
        super().__init__()
        self.attn = MultiHeadedAttention(num_heads, feature_dim)
        self.mlp = _mlp([feature_dim * 2, feature_dim * 2, feature_dim])
        nn.init.constant_(self.mlp[-1].bias, 0.0)


class AttentionalGNN(nn.Module):
    def __init__(self, feature_dim, layer_names, include_self, additional, with_linear_transform):
        super().__init__()
        self.layers = nn.ModuleList([
            GraphAttentionLayer(D, D, 0.2, include_self, additional, with_linear_transform) if i % 3 == 0
            else AttentionPropagation(feature_dim, NUM_HEADS) for i in range(len(layer_names))])
        self.names = layer_names


class KeypointEncoder(nn.Module):
    """MLP([inp, *layers, feature_dim]) on cat([kpts^T, scores]) (GATs_SuperGlue.py:131-140).
    Built by the reference but never called by its forward; callable here as a standalone HIP op."""

    def __init__(self, inp_dim, feature_dim, layers):
        super().__init__()
        self.inp_dim = inp_dim
        self.encoder = _mlp([inp_dim] + list(layers) + [feature_dim])
        nn.init.constant_(self.encoder[-1].bias, 0.0)

    def forward(self, kpts, scores):
        if list(self.encoder[0].weight.shape[:1]) != [32] or len(self.encoder) != 10:
            raise NotImplementedError("HIP KeypointEncoder supports the shipped layout [inp,32,64,128,256]")
        lib = _native.load()
        kpts, scores = _gpu(kpts, "kpts"), _gpu(scores, "scores")
        if scores.device != kpts.device:
            raise RuntimeError(f"kpts is on {kpts.device} but scores is on {scores.device}")
        b, n = kpts.shape[0], kpts.shape[1]
        if n < 2:
            raise ValueError(f"Expected more than 1 spatial element when training, got input size {[b, 32, n]}")
        kw = _native.KencWeights()
        keep = []
        for j, idx in enumerate((0, 3, 6, 9)):
            w = _gpu(self.encoder[idx].weight.detach(), "encoder weight")
            bb = _gpu(self.encoder[idx].bias.detach(), "encoder bias")
            keep += [w, bb]
            kw.w[j], kw.b[j] = w.data_ptr(), bb.data_ptr()
        kw.inp_dim = self.inp_dim
        out = torch.empty(b, D, n, device=kpts.device, dtype=torch.float32)
        nbytes = lib.gatsspg_kenc_scratch_bytes(b, n)
        scratch = torch.empty(nbytes, device=kpts.device, dtype=torch.uint8)
        _native.call("gatsspg_keypoint_encoder", kpts.device, ctypes.byref(kw), kpts, scores, b, n, out, scratch, nbytes)
        return out


def pack_frames(queries, out=None):
    """Per-frame descriptor tensors ([256, n_i] or [1, 256, n_i]) -> (dq [b, 256, cap1], counts): frame i in columns [0, n_i) of
    its slab, cap1 the largest count.  The columns behind a count are left UNINITIALISED on purpose (``torch.empty``): the frame
    forward never reads them.  ``out``: a [b, 256, >= cap1] buffer to fill instead."""
    qs = [q[0] if q.dim() == 3 else q for q in queries]
    if not qs:
        raise ValueError("pack_frames needs at least one frame")
    for q in qs:
        if q.dim() != 2 or q.shape[0] != D:
            raise ValueError(f"descriptors must be [256, n] or [1, 256, n] (got {list(q.shape)})")
    counts = [int(q.shape[1]) for q in qs]
    if out is None:
        out = torch.empty(len(qs), D, max(counts), device=qs[0].device, dtype=torch.float32)
    for i, q in enumerate(qs):
        out[i, :, :counts[i]] = q
    return out, counts


def trim_frames(out, counts):
    """The outputs of ``forward_frames`` per frame, trimmed to the counts: a list of dicts with ``conf`` [n_i, n2] (a VIEW of the batch
    buffer), ``matches0`` / ``matching_scores0`` [n_i], ``matches1`` / ``matching_scores1`` [n2]."""
    conf, m0, m1, s0, s1 = out
    return [{"conf": conf[i, :n], "matches0": m0[i, :n], "matches1": m1[i], "matching_scores0": s0[i, :n], "matching_scores1": s1[i]}
            for i, n in enumerate(counts)]


_NO_CPU = ("onepose_amd.GATsSuperGlue runs only on a ROCm GPU (tensor '{}' is on {}); "
           "there is no CPU fallback -- move the module and its inputs to the GPU")


def _gpu(t, name):
    return gpu_tensor(t, torch.float32, _NO_CPU.format(name, "{}"))


class Database:
    """A 3D object database kept resident on the GPU together with everything the first three GNN layers
    derive from it alone (``GATsSuperGlue.prepare_database``).  Valid for the weights it was built with."""

    def __init__(self, cache, desc3d_db, desc2d_db, b, n2, num_leaf, weights_key):
        self.cache, self.desc3d_db, self.desc2d_db = cache, desc3d_db, desc2d_db
        self.b, self.n2, self.num_leaf, self.weights_key = b, n2, num_leaf, weights_key
        # the cache is written on the stream prepare_database ran on; other streams wait on this event before reading it
        self.stream = torch.cuda.current_stream(cache.device).cuda_stream
        self.ready = torch.cuda.Event()
        self.ready.record(torch.cuda.current_stream(cache.device))

    def check(self, engine, b, n2, num_leaf, device, frames=False):
        """``frames``: the cache is consumed by ``b`` frames at once (``forward_frames``), which takes a ``b = 1`` cache."""
        if frames and self.b != 1:
            raise ValueError(f"a frame batch runs against ONE database: the cache must be prepared with b=1 (this one has b={self.b})")
        if frames:
            b = 1
        if (b, n2, num_leaf) != (self.b, self.n2, self.num_leaf) or self.cache.device != device:
            raise ValueError(f"database cache was built for b={self.b} n2={self.n2} num_leaf={self.num_leaf} on "
                             f"{self.cache.device}; got b={b} n2={n2} num_leaf={num_leaf} on {device}")
        engine.packed_weights(device)
        if (engine._packed.key, engine.flags()) != self.weights_key:
            raise ValueError("database cache was built with different weights / flags / precision; call prepare_database again")
        cur = torch.cuda.current_stream(device)
        if cur.cuda_stream != self.stream:
            cur.wait_event(self.ready)


# --------------------------------------------------------------------------------------------------
# the engine: packed weights + workspace + stage calls (also used by the per-kernel parity tests)
# --------------------------------------------------------------------------------------------------
class GATsSPGEngine(Engine):
    """The packed weights, the workspaces (keyed (b, n1, n2, num_leaf), device) and the stage calls of one module."""

    native = _native
    WORKSPACE_BYTES, LAST_ERROR = "gatsspg_workspace_bytes", "gatsspg_last_error"
    PARAMETER_REFUSAL = _NO_CPU.format("parameter", "{}")
    # 32 entries cover 8 object databases on 4 streams
    MAX_CACHED_WORKSPACES = 32
    MAX_CACHED_WORKSPACE_BYTES = 32 << 30

    def __init__(self, module):
        super().__init__(module)
        self._slots = None              # (module._parameters dict, name) of every tensor the forward reads, in pack order

    @property
    def workspace_allocations(self):
        return self._workspaces.allocations

    # ---- weights ----
    def _raw_tensors(self):
        """The 98 tensors the forward reads, in pack order.  Walking the module tree costs ~0.3 ms of nn.Module.__getattr__ per
        call -- a third of a frame -- so the walk is done once and remembered as (leaf module's _parameters dict, name) slots: the
        lookup through them is live (a Parameter that is replaced, moved by .to() or loaded over is seen), only swapping a whole
        SUB-MODULE for another object needs invalidate() (GATsSuperGlue._apply / load_state_dict call it anyway)."""
        if self._slots is None:
            m = self.module
            mods = []
            for i, name in enumerate(GNN_LAYER_NAMES):
                layer = m.gnn.layers[i]
                if name == "GATs":
                    mods += [(layer, "W"), (layer, "a")]
                else:
                    for sub in (layer.attn.proj[0], layer.attn.proj[1], layer.attn.proj[2], layer.attn.merge, layer.mlp[0], layer.mlp[3]):
                        mods += [(sub, "weight"), (sub, "bias")]
            mods += [(m.final_proj, "weight"), (m.final_proj, "bias")]
            self._slots = [(mod._parameters, name) for mod, name in mods]
        return [d[n] for d, n in self._slots]

    def invalidate(self):
        """Forget the remembered parameter slots (the packed blob is re-validated against the tensors on the next call anyway)."""
        self._slots = None

    def _pack(self, keep):
        raw = _native.RawWeights()
        it = iter(keep)
        gi = ai = 0
        for name in GNN_LAYER_NAMES:
            if name == "GATs":
                raw.gats_W[gi], raw.gats_a[gi] = next(it).data_ptr(), next(it).data_ptr()
                gi += 1
            else:
                for j in range(3):
                    raw.proj_w[ai][j], raw.proj_b[ai][j] = next(it).data_ptr(), next(it).data_ptr()
                raw.merge_w[ai], raw.merge_b[ai] = next(it).data_ptr(), next(it).data_ptr()
                raw.mlp0_w[ai], raw.mlp0_b[ai] = next(it).data_ptr(), next(it).data_ptr()
                raw.mlp3_w[ai], raw.mlp3_b[ai] = next(it).data_ptr(), next(it).data_ptr()
                ai += 1
        raw.final_w, raw.final_b = next(it).data_ptr(), next(it).data_ptr()
        packed = torch.empty(self.lib.gatsspg_packed_weights_bytes() // 4, device=keep[0].device, dtype=torch.float32)
        self.call("gatsspg_pack_weights", packed.device, ctypes.byref(raw), packed)
        return packed

    def flags(self):
        hp = self.module.hparams
        return ((_native.FLAG_INCLUDE_SELF if hp["include_self"] else 0)
                | (_native.FLAG_ADDITIONAL if hp["additional"] else 0)
                | (_native.FLAG_WITH_LINEAR_TRANSFORM if hp["with_linear_transform"] else 0)
                | _native.PRECISIONS[self.module.precision])

    def _outputs(self, b, n1, n2, dev):
        """conf [b,n1,n2], matches0 [b,n1] / matches1 [b,n2] int64, mscores0 / mscores1."""
        return (torch.empty(b, n1, n2, device=dev, dtype=torch.float32), torch.empty(b, n1, device=dev, dtype=torch.int64),
                torch.empty(b, n2, device=dev, dtype=torch.int64), torch.empty(b, n1, device=dev, dtype=torch.float32),
                torch.empty(b, n2, device=dev, dtype=torch.float32))

    # ---- whole forward, all b samples ----
    def forward(self, dq, d3, d2db, scale_factor, match_threshold, database=None):
        b, _, n1 = dq.shape
        n2 = d3.shape[2]
        num_leaf = d2db.shape[2] // n2
        dev = dq.device
        packed = self.packed_weights(dev)
        ws = self.workspace(b, n1, n2, num_leaf, dev)
        out = self._outputs(b, n1, n2, dev)
        if database is not None:
            database.check(self, b, n2, num_leaf, dev)
            self.call("gatsspg_forward_cached", dev, packed, dq, database.desc2d_db, database.cache, database.cache.numel() * 4,
                      b, n1, n2, num_leaf, self.flags(), float(scale_factor), float(match_threshold), *out, ws, ws.numel())
        else:
            self.call("gatsspg_forward", dev, packed, dq, d3, d2db, b, n1, n2, num_leaf, self.flags(), float(scale_factor),
                      float(match_threshold), *out, ws, ws.numel())
        return out

    def forward_frames(self, dq, counts, database, scale_factor, match_threshold, out=None):
        """``b <= MAX_FRAMES`` frames with their own query counts against ONE database in one chain of launches
        (``gatsspg_forward_frames``).  dq [b,256,cap1]: frame i in columns [0, counts[i]); counts: b host ints; database: a ``b = 1``
        handle of prepare_database.  Returns (conf [b,cap1,n2], matches0 [b,cap1], matches1 [b,n2], mscores0, mscores1); frame i is
        bitwise ``forward(dq[i:i+1, :, :counts[i]], ..., database)``, conf rows at or past counts[i] are not written.  ``out``: the
        five output tensors to write into (default: fresh ones)."""
        b, _, cap1 = dq.shape
        counts = [int(c) for c in counts]
        if len(counts) != b:
            raise ValueError(f"{b} frames but {len(counts)} counts")
        n2, num_leaf, dev = database.n2, database.num_leaf, dq.device
        packed = self.packed_weights(dev)
        database.check(self, b, n2, num_leaf, dev, frames=True)
        ws = self.workspace(b, cap1, n2, num_leaf, dev)
        out = self._outputs(b, cap1, n2, dev) if out is None else out
        n1 = (ctypes.c_int32 * b)(*counts)
        self.call("gatsspg_forward_frames", dev, packed, dq, n1, database.desc2d_db, database.cache, database.cache.numel() * 4,
                  b, cap1, n2, num_leaf, self.flags(), float(scale_factor), float(match_threshold), *out, ws, ws.numel())
        return out

    def prepare_database(self, d3, d2db):
        """Query-independent part of the first three GNN layers for a resident 3D database (amortised mode)."""
        b, _, n2 = d3.shape
        num_leaf = d2db.shape[2] // n2
        dev = d3.device
        packed = self.packed_weights(dev)
        nbytes = self.lib.gatsspg_db_cache_bytes(b, n2)
        cache = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
        ws = self.workspace(b, 2, n2, num_leaf, dev)
        self.call("gatsspg_prepare_database", dev, packed, d3, d2db, b, n2, num_leaf, self.flags(), cache, nbytes, ws, ws.numel())
        return Database(cache, d3, d2db, b, n2, num_leaf, (self._packed.key, self.flags()))

    # ---- stages (parity tests): ``dims`` = (b, n1, n2, num_leaf, device), what load_state returns ----
    def load_state(self, dq, d3, num_leaf):
        dims = (dq.shape[0], dq.shape[2], d3.shape[2], num_leaf, dq.device)
        ws = self.workspace(*dims)
        self.call("gatsspg_load_state", dq.device, dq, d3, *dims[:4], ws, ws.numel())
        return dims

    def store_state(self, dims, which=0):
        b, n1, n2, _, dev = dims
        ws = self.workspace(*dims)
        o2 = torch.empty(b, D, n1, device=dev, dtype=torch.float32)
        o3 = torch.empty(b, D, n2, device=dev, dtype=torch.float32)
        self.call("gatsspg_store_state", dev, which, o2, o3, *dims[:4], ws, ws.numel())
        return o2, o3

    def gats_layer(self, dims, layer, d2db, flags=None):
        ws = self.workspace(*dims)
        self.call("gatsspg_gats_layer", dims[4], self.packed_weights(dims[4]), layer, d2db, *dims[:4],
                  self.flags() if flags is None else flags, ws, ws.numel())

    def gats_layer_frames(self, dims, layer, d2db, leaf_logits=None, shared_leaf=True):
        """One GATs layer of a frame batch on the state of ``dims``: the b frames against ONE database's leaves ``d2db`` [1,256,n2*L];
        shared_leaf: the kernel that reads each leaf tile once per group of frames, or the per-frame kernel at database stride 0."""
        ws = self.workspace(*dims)
        self.call("gatsspg_gats_layer_frames", dims[4], self.packed_weights(dims[4]), layer, d2db, leaf_logits, *dims[:4], self.flags(),
                  int(shared_leaf), ws, ws.numel())

    def attn_layer(self, dims, layer, kind):
        ws = self.workspace(*dims)
        self.call("gatsspg_attn_layer", dims[4], self.packed_weights(dims[4]), layer, kind, *dims[:4], self.flags(), ws, ws.numel())

    def final_proj_norm(self, dims):
        ws = self.workspace(*dims)
        self.call("gatsspg_final_proj_norm", dims[4], self.packed_weights(dims[4]), *dims[:4], ws, ws.numel())

    def score_match(self, dims, scale_factor, match_threshold):
        b, n1, n2, _, dev = dims
        ws = self.workspace(*dims)
        out = self._outputs(b, n1, n2, dev)
        self.call("gatsspg_score_dual_softmax_match", dev, *dims[:4], float(scale_factor), float(match_threshold), *out, ws, ws.numel())
        return out


# --------------------------------------------------------------------------------------------------
# the drop-in module
# --------------------------------------------------------------------------------------------------
class GATsSuperGlue(nn.Module):
    """HIP implementation behind the reference ``GATsSuperGlue`` API (GATs_SuperGlue.py:143-241).

    ``precision`` (keyword-only, not part of the reference signature; also settable as an attribute) selects the
    arithmetic of the attention layers' GEMMs for every call of this module: ``"fp32"`` (default: exact fp32 MFMA, the
    reference's arithmetic), ``"bf16x3"`` (split-bf16 MFMA, three bf16 products per fp32 product; conf within 1e-6 of
    the fp32 forward and identical matches on every parity case) or ``"bf16x6"`` (operands split exactly into three bf16
    planes, six products per fp32 product: fp32-class arithmetic on the bf16 matrix pipe) ``"fp16x3"`` (two fp16 terms per operand,
    three fp16 MFMA products: bf16x3's speed at 100x its operand precision; operands saturate beyond +-131008) or ``"fp16x4"`` (the same
    terms, all four products: fp32-class in four MFMAs).  It travels to the library as a bit of the ``flags``
    argument of the C ABI; nothing is read from the environment."""

    def __init__(self, hparams, *, precision="fp32"):
        super().__init__()
        self.hparams = hparams
        self.precision = precision
        self.match_type = hparams["match_type"]
        if hparams["descriptor_dim"] != D:
            raise NotImplementedError("descriptor_dim must be 256 (the reference GNN hard-codes it, :35-36)")
        self.kenc_2d = KeypointEncoder(3, hparams["descriptor_dim"], hparams["keypoints_encoder"])
        self.kenc_3d = KeypointEncoder(4, hparams["descriptor_dim"], hparams["keypoints_encoder"])
        self.gnn = AttentionalGNN(hparams["descriptor_dim"], GNN_LAYER_NAMES, hparams["include_self"],
                                  hparams["additional"], hparams["with_linear_transform"])
        self.final_proj = nn.Conv1d(hparams["descriptor_dim"], hparams["descriptor_dim"], kernel_size=1, bias=True)
        self.register_parameter("bin_score", nn.Parameter(torch.tensor(1.0)))
        self._engine = None

    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, value):
        if value not in _native.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_native.PRECISIONS)} (got {value!r})")
        self._precision = value

    @property
    def engine(self):
        if self._engine is None:
            self._engine = GATsSPGEngine(self)  # loads the HIP library; raises if it is not built
        return self._engine

    def _apply(self, fn, *args, **kwargs):      # .to() / .cuda() / .float(): parameters may be replaced
        if self._engine is not None:
            self._engine.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        if self._engine is not None:
            self._engine.invalidate()
        return super().load_state_dict(*args, **kwargs)

    def _inputs(self, data):
        kpts2d, kpts3d = data["keypoints2d"].float(), data["keypoints3d"].float()
        dq = data["descriptors2d_query"].float()
        d3, d2db = data["descriptors3d_db"].float(), data["descriptors2d_db"].float()
        return kpts2d, kpts3d, dq, d3, d2db

    def prepare_database(self, data):
        """Amortised mode (not part of the reference API): keep the object's 3D database resident and precompute
        what the first three GNN layers derive from it alone.  ``data`` needs ``descriptors3d_db`` and
        ``descriptors2d_db``; pass the returned handle as ``database=`` to forward()/forward_batched() together
        with the same database tensors.  Results are bit-identical to the plain forward when every one-side window of the cached
        stages takes the kernel form the whole frame takes, otherwise within re-association noise of it with the same matches
        (include/gatsspg.h, amortised mode)."""
        d3, d2db = _gpu(data["descriptors3d_db"], "descriptors3d_db"), _gpu(data["descriptors2d_db"], "descriptors2d_db")
        if d3.shape[2] < 2 or d2db.shape[2] % d3.shape[2] != 0:
            raise ValueError("database needs >= 2 points and a whole number of leaves per point")
        with torch.no_grad():
            return self.engine.prepare_database(d3, d2db)

    def forward_batched(self, data, database=None):
        """All b samples: returns (conf [b,n1,n2], matches0 [b,n1], matches1 [b,n2], mscores0, mscores1).
        The reference has no such path (its ``pred`` is sample 0 only); used for batched throughput."""
        if self.match_type != "softmax":
            raise NotImplementedError
        if database is not None:
            data = dict(data, descriptors3d_db=database.desc3d_db, descriptors2d_db=database.desc2d_db)
        _, _, dq, d3, d2db = self._inputs(data)
        dq, d3, d2db = _gpu(dq, "descriptors2d_query"), _gpu(d3, "descriptors3d_db"), _gpu(d2db, "descriptors2d_db")
        n1, n2 = dq.shape[2], d3.shape[2]
        if n1 == 1 or n2 == 1:  # what nn.InstanceNorm1d raises inside the reference MLP (:126)
            raise ValueError(f"Expected more than 1 spatial element when training, got input size {[dq.shape[0], 512, 1]}")
        if dq.shape[1] != D or d3.shape[1] != D or d2db.shape[1] != D:
            raise ValueError("descriptors must have 256 channels")
        if d2db.shape[2] % n2 != 0 or d2db.shape[2] == 0:
            raise ValueError(f"descriptors2d_db has {d2db.shape[2]} leaves for {n2} 3D points: not a multiple")
        with torch.no_grad():
            return self.engine.forward(dq, d3, d2db, self.hparams["scale_factor"], self.hparams["match_threshold"],
                                       database)

    def match_frames(self, queries, database, max_frames=_native.MAX_FRAMES):
        """Many frames of ONE object (not part of the reference API): ``queries`` is a list of per-frame descriptor tensors
        ([256, n_i] or [1, 256, n_i], n_i >= 2, each frame its own count), ``database`` a handle of prepare_database() made with
        ONE database (b = 1) or, to prepare one here, the data dict with ``descriptors3d_db`` / ``descriptors2d_db``.  Runs
        ``max_frames`` (<= 32) frames per chain of launches and returns one dict per frame -- ``matches0``, ``matching_scores0``,
        ``matches1``, ``matching_scores1`` trimmed to the frame's count and ``conf`` [n_i, n2] as a view of the batch buffer -- each
        bitwise what ``forward(..., database=database)`` gives for that frame alone."""
        if self.match_type != "softmax":
            raise NotImplementedError
        if not 1 <= max_frames <= _native.MAX_FRAMES:
            raise ValueError(f"max_frames must be in [1, {_native.MAX_FRAMES}] (got {max_frames})")
        if not isinstance(database, Database):
            database = self.prepare_database(database)
        if database.b != 1:
            raise ValueError(f"a frame batch runs against ONE database: the cache must be prepared with b=1 (this one has b={database.b})")
        queries = [_gpu(q, "descriptors2d_query") for q in queries]
        queries = [q[0] if q.dim() == 3 and q.shape[0] == 1 else q for q in queries]
        for q in queries:
            if q.dim() != 2 or q.shape[0] != D:
                raise ValueError(f"descriptors must have 256 channels, [256, n] or [1, 256, n] (got {list(q.shape)})")
            if q.shape[1] < 2:   # an empty frame has no matcher call in the reference (:195); one point is what InstanceNorm1d refuses (:126)
                raise ValueError(f"Expected more than 1 spatial element when training, got input size {[1, 512, q.shape[1]]}")
        res = []
        with torch.no_grad():
            for i in range(0, len(queries), max_frames):
                dq, counts = pack_frames(queries[i:i + max_frames])
                out = self.engine.forward_frames(dq, counts, database, self.hparams["scale_factor"], self.hparams["match_threshold"])
                res += trim_frames(out, counts)
        return res

    def forward(self, data, database=None):
        """Keys of ``data`` as in the reference docstring (:181-189); extra keys are ignored.  ``database``:
        optional handle from prepare_database() (amortised mode)."""
        kpts2d, kpts3d, _, _, _ = self._inputs(data)
        if kpts2d.shape[1] == 0 or kpts3d.shape[1] == 0:  # :195-203
            shape0, shape1 = kpts2d.shape[:-1], kpts3d.shape[:-1]
            return {
                "matches0": kpts2d.new_full(shape0, -1, dtype=torch.int)[0],
                "matches1": kpts3d.new_full(shape1, -1, dtype=torch.int)[0],
                "matching_scores0": kpts2d.new_zeros(shape0)[0],
                "matching_scores1": kpts3d.new_zeros(shape1)[0],
                "skip_train": True,
            }
        if self.match_type != "softmax":
            raise NotImplementedError  # :238-239
        conf, m0, m1, s0, s1 = self.forward_batched(data, database)
        pred = {"matches0": m0[0], "matches1": m1[0], "matching_scores0": s0[0], "matching_scores1": s1[0]}
        return pred, conf
