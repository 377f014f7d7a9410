"""Training the GATsSPG matcher (reference: src/models/GATsSPG_lightning_model.py:39-51, src/losses/focal_loss.py,
src/utils/data_utils.py:208-230).

A training step is ``training_loss(model, data, target, criterion)``:

* ``matching_descriptors`` -- the trunk of ``onepose_amd.GATsSuperGlue`` (12 GNN layers, ``final_proj``, ``normalize``) in stock
  differentiable torch ops on the module's own parameters (plumbing; HIP backward kernels for its stages can replace it one at a
  time behind this interface);
* ``MatchingLoss`` -- the matching head: score contraction, dual softmax and focal loss over the b x n x m matrix.
  ``impl="hip"`` runs it forward AND backward as one chain of HIP launches (include/gatsspg_train.h) behind a
  ``torch.autograd.Function``; ``impl="eager"`` restates the reference head in stock torch ops (the bench baseline, and what runs
  on a CPU).  Neither is ever chosen silently.

ONE DIFFERENCE from the reference: a target with no positive and no negative entry makes the reference's FocalLoss assert; here
the loss is 0 with zero gradients (both implementations), so that no host read-back of the counts is needed.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native_train
from ._binding import NativeError, gpu_tensor

_NO_CPU = ("onepose_amd.MatchingLoss(impl='hip') runs only on a ROCm GPU (tensor '{}' is on {}); there is no CPU fallback -- "
           "move the tensors to the GPU or ask for impl='eager'")
IMPLS = ("hip", "eager")


class SparseTarget:
    """The assignment of a batch as the reference's dataset stores it: per sample a ``[2, k]`` integer tensor of (2D index, 3D
    index) pairs and the sample's unpadded shape ``n_orig x m_orig``; ``pad_val`` is what ``reshape_assign_matrix`` writes into the
    rows >= n_orig and the columns >= m_orig (0: negatives; anything else but 1: in neither mean).

    ``pairs``: a list of b ``[2, k_i]`` tensors, or one ``[b, 2, k]`` tensor.  ``n_orig`` / ``m_orig``: an int or b ints."""

    def __init__(self, pairs, n_orig, m_orig, pad_val=0):
        if isinstance(pairs, torch.Tensor):
            if pairs.dim() != 3 or pairs.shape[1] != 2:
                raise ValueError(f"pairs must be [b, 2, k] or a list of [2, k_i] (got {list(pairs.shape)})")
            pairs = list(pairs)
        self.pairs = [p.reshape(2, -1) for p in pairs]
        for p in self.pairs:
            if p.dtype.is_floating_point or p.dtype is torch.bool:
                raise TypeError(f"pairs must be integers (got {p.dtype})")
        b = len(self.pairs)
        if b == 0:
            raise ValueError("SparseTarget needs at least one sample")
        self.n_orig = [int(n_orig)] * b if isinstance(n_orig, int) else [int(v) for v in n_orig]
        self.m_orig = [int(m_orig)] * b if isinstance(m_orig, int) else [int(v) for v in m_orig]
        if len(self.n_orig) != b or len(self.m_orig) != b or min(self.n_orig + self.m_orig) < 0:
            raise ValueError("n_orig and m_orig: one non-negative int per sample")
        if pad_val == 1:
            raise ValueError("pad_val = 1 would make every padded entry a positive")
        self.pad_val = int(pad_val)
        self.negative_pairs = None      # device int32 [1] after classes(): pairs with a negative index (ignored, not wrapped around)

    def __len__(self):
        return len(self.pairs)

    def dense(self, n, m, device=None):
        """``conf_matrix_gt`` [b, n, m] int16 in stock torch ops (data_utils.py:208-230 with pad=True; a negative index is ignored)."""
        out = []
        for p, no, mo in zip(self.pairs, self.n_orig, self.m_orig):
            p = p.to(device=device if device is not None else p.device, dtype=torch.long)
            t = torch.zeros(n, m, dtype=torch.int16, device=p.device)
            keep = (p[0] >= 0) & (p[1] >= 0) & (p[0] < n) & (p[1] < m)
            t[p[0][keep], p[1][keep]] = 1
            t[no:] = self.pad_val
            t[:, mo:] = self.pad_val
            out.append(t)
        return torch.stack(out)

    def classes(self, n, m, device):
        """The int8 class matrix [b, n, m] (0 negative, 1 positive, 2 ignored) through ``gtr_build_target``."""
        b = len(self)
        kcap = max(1, max(p.shape[1] for p in self.pairs))
        packed = torch.zeros(b, 2, kcap, dtype=torch.int32, device=device)
        for i, p in enumerate(self.pairs):
            packed[i, :, :p.shape[1]] = p.to(device=device, dtype=torch.int32)
        host = [(ctypes.c_int32 * b)(*v) for v in ([p.shape[1] for p in self.pairs], self.n_orig, self.m_orig)]
        cls = torch.empty(b, n, m, dtype=torch.int8, device=device)
        self.negative_pairs = torch.empty(1, dtype=torch.int32, device=device)
        _native_train.call("gtr_build_target", device, packed, *host, b, kcap, n, m, int(self.pad_val == 0), cls, self.negative_pairs)
        return cls


def _classes_of_dense(target):
    """A dense integer target (1 positive, 0 negative, anything else in neither mean) as the int8 class matrix."""
    two = torch.full((), _native_train.CLASS_IGNORED, dtype=torch.int8, device=target.device)
    return torch.where(target == 1, two - 1, torch.where(target == 0, two - 2, two))


class _HipHead(torch.autograd.Function):
    """loss, counts = head(x, y, classes): ``gtr_loss_head``.  When an input requires grad the forward also writes dx and dy and
    keeps those two (no n x m tensor lives between forward and backward); backward scales them by grad_output."""

    @staticmethod
    def forward(ctx, x, y, cls, alpha, gamma, pos_w, neg_w, scale):
        b, _, n = x.shape
        m = y.shape[2]
        dev = x.device
        lib = _native_train.load()
        nbytes = lib.gtr_workspace_bytes(b, n, m)
        if nbytes == 0:
            raise NativeError("gtr_workspace_bytes: " + lib.gtr_last_error().decode())
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        grads = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dx, dy = (torch.empty_like(x), torch.empty_like(y)) if grads else (None, None)
        lib.call("gtr_loss_head", dev, x, y, cls, b, n, m, alpha, gamma, pos_w, neg_w, scale, loss, counts, dx, dy, ws, nbytes)
        if grads:
            ctx.save_for_backward(dx, dy)
        ctx.mark_non_differentiable(counts)
        return loss[0], counts

    @staticmethod
    def backward(ctx, grad_loss, _grad_counts):
        dx, dy = ctx.saved_tensors
        return (grad_loss * dx if ctx.needs_input_grad[0] else None, grad_loss * dy if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None)


class MatchingLoss(nn.Module):
    """The matching head of a training step: ``forward(mdesc0 [b,256,n], mdesc1 [b,256,m], target) -> loss`` with
    ``scores = <mdesc0, mdesc1> / scale_factor``, ``conf = softmax(scores, 1) * softmax(scores, 2)`` (GATs_SuperGlue.py:217-218) and
    the reference's FocalLoss (focal_loss.py:13-26; defaults of configs/experiment/train_GATsSPG.yaml).

    ``target``: a dense integer tensor [b, n, m] (the datamodule's ``conf_matrix_gt``: 1 positive, 0 negative, any other value in
    neither mean) or a ``SparseTarget``.  ``impl="hip"``: one chain of HIP launches forward and backward, GPU tensors only;
    ``impl="eager"``: stock torch ops, any device.  ``last_counts``: device int64 [3] (positives, negatives, ignored) of the last call.

    ONE DIFFERENCE from the reference: with no positive and no negative entry the reference asserts; here the loss is 0 with
    zero gradients (no host read-back)."""

    def __init__(self, alpha=0.5, gamma=2, pos_weights=0.5, neg_weights=0.5, scale_factor=0.07, impl="hip"):
        super().__init__()
        if impl not in IMPLS:
            raise ValueError(f"impl must be one of {IMPLS} (got {impl!r})")
        self.alpha, self.gamma, self.pos_weights, self.neg_weights = float(alpha), float(gamma), float(pos_weights), float(neg_weights)
        self.scale_factor, self.impl = float(scale_factor), impl
        self.last_counts = None

    def extra_repr(self):
        return (f"alpha={self.alpha}, gamma={self.gamma}, pos_weights={self.pos_weights}, neg_weights={self.neg_weights}, "
                f"scale_factor={self.scale_factor}, impl={self.impl!r}")

    def forward(self, mdesc0, mdesc1, target):
        if mdesc0.dim() != 3 or mdesc1.dim() != 3 or mdesc0.shape[:2] != mdesc1.shape[:2] or mdesc0.shape[1] != _native_train.DESC_DIM:
            raise ValueError(f"mdesc0 / mdesc1 must be [b, 256, n] / [b, 256, m] (got {list(mdesc0.shape)}, {list(mdesc1.shape)})")
        b, _, n = mdesc0.shape
        m = mdesc1.shape[2]
        if isinstance(target, SparseTarget):
            if len(target) != b:
                raise ValueError(f"the target has {len(target)} samples, the descriptors {b}")
        elif not isinstance(target, torch.Tensor) or target.dtype.is_floating_point or tuple(target.shape) != (b, n, m):
            raise ValueError(f"target must be a SparseTarget or an integer tensor [{b}, {n}, {m}]")
        return self._hip(mdesc0, mdesc1, target, b, n, m) if self.impl == "hip" else self._eager(mdesc0, mdesc1, target, n, m)

    def _hip(self, x, y, target, b, n, m):
        x, y = gpu_tensor(x, torch.float32, _NO_CPU.format("mdesc0", "{}")), gpu_tensor(y, torch.float32, _NO_CPU.format("mdesc1", "{}"))
        if y.device != x.device:
            raise RuntimeError(f"mdesc0 is on {x.device} but mdesc1 is on {y.device}")
        if isinstance(target, SparseTarget):
            cls = target.classes(n, m, x.device)
        else:
            if target.device != x.device:
                raise RuntimeError(_NO_CPU.format("target", target.device) if not target.is_cuda else f"target is on {target.device}, mdesc0 on {x.device}")
            cls = _classes_of_dense(target).contiguous()
        loss, counts = _HipHead.apply(x, y, cls, self.alpha, self.gamma, self.pos_weights, self.neg_weights, self.scale_factor)
        self.last_counts = counts
        return loss

    def _eager(self, x, y, target, n, m):
        if isinstance(target, SparseTarget):
            target = target.dense(n, m, x.device)
        scores = torch.einsum("bdn,bdm->bnm", x, y) / self.scale_factor
        conf = F.softmax(scores, 1) * F.softmax(scores, 2)
        pos, neg = target == 1, target == 0
        cp, cn = conf[pos], conf[neg]
        lp = -self.alpha * torch.pow(1 - cp, self.gamma) * cp.log()
        ln = -(1 - self.alpha) * torch.pow(cn, self.gamma) * (1 - cn).log()
        self.last_counts = torch.stack([pos.sum(), neg.sum(), (~(pos | neg)).sum()])
        loss = conf.sum() * 0                               # no positive and no negative: 0, with zero gradients
        if lp.numel():
            loss = loss + self.pos_weights * lp.mean()
        if ln.numel():
            loss = loss + self.neg_weights * ln.mean()
        return loss


# --------------------------------------------------------------------------------------------------
# the trunk, in stock differentiable torch ops on the module's own parameters
# --------------------------------------------------------------------------------------------------
def _linear_attention(q, k, v):
    """GATs_SuperGlue.py:69-80: q, k, v [b, 64, heads, points]."""
    q, k = F.elu(q) + 1, F.elu(k) + 1
    length = v.size(3)
    v = v / length
    kv = torch.einsum("bdhm,bqhm->bqdh", k, v)
    z = 1 / (torch.einsum("bdhm,bdh->bhm", q, k.sum(3)) + 1e-6)
    return torch.einsum("bdhm,bqdh,bhm->bqhm", q, kv, z) * length


def _propagate(layer, x, source):
    """AttentionPropagation (:93-113) through the module's own Conv1d / InstanceNorm1d / ReLU containers."""
    attn, b = layer.attn, x.size(0)
    q, k, v = (proj(t).view(b, attn.dim, attn.num_heads, -1) for proj, t in zip(attn.proj, (x, source, source)))
    message = attn.merge(_linear_attention(q, k, v).contiguous().view(b, attn.dim * attn.num_heads, -1))
    return layer.mlp(torch.cat([x, message], dim=1))


def _graph_attention(layer, leaves, points):
    """GraphAttentionLayer (GATs.py:35-88): leaves [b, n * num_leaf, d] aggregated into their points [b, n, d]."""
    b, n, d = points.shape
    num_leaf = leaves.shape[1] // n
    w_leaves, w_points = leaves @ layer.W, points @ layer.W
    e_leaves = (w_leaves @ layer.a[:d]).view(b, n, num_leaf, 1)
    e_points = w_points @ layer.a[d:]
    values = (w_leaves if layer.with_linear_transform else leaves).view(b, n, num_leaf, d)
    skip = w_points if layer.with_linear_transform else points
    if layer.include_self:
        e_leaves = torch.cat([e_points.unsqueeze(2), e_leaves], dim=2)
        values = torch.cat([skip.unsqueeze(2), values], dim=2)
    attention = F.softmax(F.leaky_relu(e_points.unsqueeze(2) + e_leaves, layer.alpha), dim=2)
    out = torch.einsum("bncd,bncq->bnq", attention, values)
    if layer.include_self:
        if layer.additional:
            out = out + points
    else:
        out = out / 2.0 + skip
    return F.elu(out)


def matching_descriptors(model, data):
    """The trunk of ``onepose_amd.GATsSuperGlue`` (GATs_SuperGlue.py:48-66, :209-213) up to the L2-normalised matching descriptors:
    ``(mdesc0 [b,256,n], mdesc1 [b,256,m])``, differentiable w.r.t. the module's parameters.  Honours the three GATs flags of the
    module's hparams and any ``num_leaf``; runs wherever the module and the data are."""
    x, y, leaves = (data[k].float() for k in ("descriptors2d_query", "descriptors3d_db", "descriptors2d_db"))
    if y.shape[2] == 0 or leaves.shape[2] % y.shape[2] != 0:
        raise ValueError(f"descriptors2d_db has {leaves.shape[2]} leaves for {y.shape[2]} 3D points: not a multiple")
    leaves = leaves.transpose(1, 2)
    for layer, name in zip(model.gnn.layers, model.gnn.names):
        if name == "GATs":
            y = _graph_attention(layer, leaves, y.transpose(1, 2)).transpose(1, 2)
        elif name == "self":
            x, y = x + _propagate(layer, x, x), y + _propagate(layer, y, y)
        else:
            x, y = x + _propagate(layer, x, y), y + _propagate(layer, y, x)
    return F.normalize(model.final_proj(x), p=2, dim=1), F.normalize(model.final_proj(y), p=2, dim=1)


def training_loss(model, data, target, criterion):
    """One training step's loss (GATsSPG_lightning_model.py:39-51): the trunk, then the matching head.  ``loss.backward()`` fills the
    gradients of the module's parameters; after ``optimizer.step()`` the module's HIP ``forward`` sees the new weights (its packed
    blob is keyed on the parameters' versions)."""
    mdesc0, mdesc1 = matching_descriptors(model, data)
    return criterion(mdesc0, mdesc1, target)
