"""Numpy restatement of the SuperGlue forward (src/models/matchers/SuperGlue/superglue.py:42-276), written from the math.

Stage functions mirror the stages of the C ABI (include/superglue/superglue.h): keypoint_encode, layer, sinkhorn (scores ->
log transport plan Z), match_tail.  ``dtype`` selects fp32 (the reference's arithmetic) or fp64 (the yardstick of the stage
parity tests).  ``forward_torch`` is a short stock-PyTorch restatement used only as the eager baseline of
tools/superglue_bench.py.
"""
from __future__ import annotations

import numpy as np

D, HEADS = 256, 4
BN_EPS = 1e-5
# bounds of the GPU forward-vs-golden tests (tests/test_sg_hip_parity.py): max |dZ|, matching scores relative to max(1, |s|)
FORWARD_ZTOL, FORWARD_STOL = 2e-4, 1e-4


def _w(sd, key, dt):
    return np.asarray(sd[key], dtype=dt)


def _conv(sd, prefix, x, dt):
    """Conv1d(k=1) on channel-major x [b, c, n]."""
    w = _w(sd, prefix + ".weight", dt)[:, :, 0]
    return np.einsum("oc,bcn->bon", w, x, optimize=True) + _w(sd, prefix + ".bias", dt)[None, :, None]


def _bn_relu(sd, prefix, x, dt):
    mean, var = _w(sd, prefix + ".running_mean", dt), _w(sd, prefix + ".running_var", dt)
    g, b = _w(sd, prefix + ".weight", dt), _w(sd, prefix + ".bias", dt)
    y = (x - mean[None, :, None]) / np.sqrt(var + dt(BN_EPS))[None, :, None] * g[None, :, None] + b[None, :, None]
    return np.maximum(y, dt(0))


def normalize_keypoints(kpts, h, w, dt=np.float32):
    size = np.array([w, h], dtype=dt)
    center = size / dt(2)
    scaling = size.max() * dt(0.7)
    return (kpts.astype(dt) - center) / scaling


def keypoint_encode(sd, kpts, scores, desc, h, w, dt=np.float32):
    """desc + MLP([3, 32, 64, 128, 256, 256])(cat(normalize(kpts)^T, scores)) with eval BatchNorm."""
    x = np.concatenate([normalize_keypoints(kpts, h, w, dt).transpose(0, 2, 1), scores.astype(dt)[:, None, :]], 1)
    for j in (0, 3, 6, 9):
        x = _bn_relu(sd, f"kenc.encoder.{j + 1}", _conv(sd, f"kenc.encoder.{j}", x, dt), dt)
    return desc.astype(dt) + _conv(sd, "kenc.encoder.12", x, dt)


def _softmax(x, axis):
    m = x.max(axis=axis, keepdims=True)
    e = np.exp(x - m)
    return e / e.sum(axis=axis, keepdims=True)


def _propagate(sd, p, x, src, dt):
    b = x.shape[0]
    q, k, v = (_conv(sd, f"{p}.attn.proj.{i}", t, dt) for i, t in enumerate((x, src, src)))
    q, k, v = (t.reshape(b, D // HEADS, HEADS, -1) for t in (q, k, v))   # channel c -> (dim c // 4, head c % 4)
    s = np.einsum("bdhn,bdhm->bhnm", q, k, optimize=True) / dt(8)
    msg = np.einsum("bhnm,bdhm->bdhn", _softmax(s, -1), v, optimize=True).reshape(b, D, -1)
    msg = _conv(sd, f"{p}.attn.merge", msg, dt)
    h = _bn_relu(sd, f"{p}.mlp.1", _conv(sd, f"{p}.mlp.0", np.concatenate([x, msg], 1), dt), dt)
    return _conv(sd, f"{p}.mlp.3", h, dt)


def layer(sd, index, kind, d0, d1, dt=np.float32):
    """One AttentionalGNN step: both deltas from the pre-update descriptors."""
    p = f"gnn.layers.{index}"
    s0, s1 = (d1, d0) if kind == "cross" else (d0, d1)
    return d0 + _propagate(sd, p, d0, s0, dt), d1 + _propagate(sd, p, d1, s1, dt)


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return (np.log(np.exp(x - m).sum(axis=axis, keepdims=True)) + m).squeeze(axis)


def sinkhorn(scores, alpha, iters, dt=np.float32):
    """log_optimal_transport: coupling with dustbins, `iters` log-space Sinkhorn steps, Z - norm."""
    b, m, n = scores.shape
    a = dt(alpha)
    Z = np.empty((b, m + 1, n + 1), dtype=dt)
    Z[:, :m, :n] = scores
    Z[:, :m, n] = a
    Z[:, m, :] = a
    ms, ns = dt(m), dt(n)
    norm = -np.log(ms + ns)
    log_mu = np.concatenate([np.full(m, norm, dt), [np.log(ns) + norm]]).astype(dt)
    log_nu = np.concatenate([np.full(n, norm, dt), [np.log(ms) + norm]]).astype(dt)
    u, v = np.zeros((b, m + 1), dt), np.zeros((b, n + 1), dt)
    for _ in range(iters):
        u = log_mu[None] - _lse(Z + v[:, None, :], 2)
        v = log_nu[None] - _lse(Z + u[:, :, None], 1)
    return (Z + u[:, :, None] + v[:, None, :]) - norm


def match_tail(Z, th):
    """Max / argmax along rows and columns of Z[:, :-1, :-1] (np.argmax: first index on ties), mutual check, threshold."""
    z = Z[:, :-1, :-1]
    i0, i1 = z.argmax(2), z.argmax(1)
    v0 = np.take_along_axis(z, i0[:, :, None], 2)[:, :, 0]
    b = np.arange(z.shape[0])[:, None]
    mutual0 = np.arange(z.shape[1])[None] == i1[b, i0]
    mutual1 = np.arange(z.shape[2])[None] == i0[b, i1]
    ms0 = np.where(mutual0, np.exp(v0), 0).astype(np.float32)
    ms1 = np.where(mutual1, ms0[b, i1], 0).astype(np.float32)
    valid0 = mutual0 & (ms0 > np.float32(th))
    valid1 = mutual1 & valid0[b, i1]
    return {"matches0": np.where(valid0, i0, -1).astype(np.int64), "matches1": np.where(valid1, i1, -1).astype(np.int64),
            "matching_scores0": ms0, "matching_scores1": ms1}


def score_matrix(sd, d0, d1, dt=np.float32):
    m0, m1 = _conv(sd, "final_proj", d0, dt), _conv(sd, "final_proj", d1, dt)
    return np.einsum("bdn,bdm->bnm", m0, m1, optimize=True) / dt(16)


def forward(sd, data, cfg, dt=np.float32):
    """Whole forward; returns (outputs dict, Z).  cfg: GNN_layers, sinkhorn_iterations, match_threshold."""
    h0, w0 = data["image_size0"]
    h1, w1 = data["image_size1"]
    d0 = keypoint_encode(sd, data["keypoints0"], data["scores0"], data["descriptors0"], h0, w0, dt)
    d1 = keypoint_encode(sd, data["keypoints1"], data["scores1"], data["descriptors1"], h1, w1, dt)
    for i, kind in enumerate(cfg["GNN_layers"]):
        d0, d1 = layer(sd, i, kind, d0, d1, dt)
    Z = sinkhorn(score_matrix(sd, d0, d1, dt), sd["bin_score"], cfg["sinkhorn_iterations"], dt)
    return match_tail(Z, cfg["match_threshold"]), Z


def z_stats(Z):
    """Row / column best and second-best of Z[:, :-1, :-1] plus the dustbin row and column: what the large goldens keep."""
    z = Z[:, :-1, :-1]
    rs, cs = np.sort(z, 2), np.sort(z, 1)
    return {"row_best": rs[:, :, -1], "row_second": rs[:, :, -2] if z.shape[2] > 1 else np.full(z.shape[:2], -np.inf, z.dtype),
            "col_best": cs[:, -1, :], "col_second": cs[:, -2, :] if z.shape[1] > 1 else np.full((z.shape[0], z.shape[2]), -np.inf, z.dtype),
            "dust_row": Z[:, -1, :], "dust_col": Z[:, :, -1]}


def forward_torch(params, data, cfg):
    """Stock PyTorch eager restatement (bench baseline): params = {name: tensor on the device}, data = torch tensors."""
    import torch

    def conv(p, x):
        return torch.einsum("oc,bcn->bon", params[p + ".weight"][:, :, 0], x) + params[p + ".bias"][None, :, None]

    def bn_relu(p, x):
        y = (x - params[p + ".running_mean"][None, :, None]) / torch.sqrt(params[p + ".running_var"] + BN_EPS)[None, :, None]
        return torch.relu(y * params[p + ".weight"][None, :, None] + params[p + ".bias"][None, :, None])

    def kenc(k, s, h, w):
        size = k.new_tensor([w, h])
        x = torch.cat([((k - size / 2) / (size.max() * 0.7)).transpose(1, 2), s[:, None]], 1)
        for j in (0, 3, 6, 9):
            x = bn_relu(f"kenc.encoder.{j + 1}", conv(f"kenc.encoder.{j}", x))
        return conv("kenc.encoder.12", x)

    def prop(p, x, src):
        b = x.shape[0]
        q, k, v = (conv(f"{p}.attn.proj.{i}", t).view(b, 64, 4, -1) for i, t in enumerate((x, src, src)))
        prob = torch.softmax(torch.einsum("bdhn,bdhm->bhnm", q, k) / 8, -1)
        msg = conv(f"{p}.attn.merge", torch.einsum("bhnm,bdhm->bdhn", prob, v).reshape(b, 256, -1))
        return conv(f"{p}.mlp.3", bn_relu(f"{p}.mlp.1", conv(f"{p}.mlp.0", torch.cat([x, msg], 1))))

    h0, w0 = data["image_size0"]
    h1, w1 = data["image_size1"]
    d0 = data["descriptors0"] + kenc(data["keypoints0"], data["scores0"], h0, w0)
    d1 = data["descriptors1"] + kenc(data["keypoints1"], data["scores1"], h1, w1)
    for i, kind in enumerate(cfg["GNN_layers"]):
        s0, s1 = (d1, d0) if kind == "cross" else (d0, d1)
        d0, d1 = d0 + prop(f"gnn.layers.{i}", d0, s0), d1 + prop(f"gnn.layers.{i}", d1, s1)
    sc = torch.einsum("bdn,bdm->bnm", conv("final_proj", d0), conv("final_proj", d1)) / 16
    b, m, n = sc.shape
    a = params["bin_score"]
    Z = torch.cat([torch.cat([sc, a.expand(b, m, 1)], -1), torch.cat([a.expand(b, 1, n), a.expand(b, 1, 1)], -1)], 1)
    norm = -torch.log(sc.new_tensor(m + n))
    log_mu = torch.cat([norm.expand(m), torch.log(sc.new_tensor(n))[None] + norm])
    log_nu = torch.cat([norm.expand(n), torch.log(sc.new_tensor(m))[None] + norm])
    u, v = torch.zeros_like(log_mu).expand(b, -1), torch.zeros_like(log_nu).expand(b, -1)
    for _ in range(cfg["sinkhorn_iterations"]):
        u = log_mu - torch.logsumexp(Z + v[:, None, :], 2)
        v = log_nu - torch.logsumexp(Z + u[:, :, None], 1)
    Z = Z + u[:, :, None] + v[:, None, :] - norm
    z = Z[:, :-1, :-1]
    mx0, mx1 = z.max(2), z.max(1)
    i0, i1 = mx0.indices, mx1.indices
    mutual0 = torch.arange(m, device=z.device)[None] == i1.gather(1, i0)
    mutual1 = torch.arange(n, device=z.device)[None] == i0.gather(1, i1)
    ms0 = torch.where(mutual0, mx0.values.exp(), z.new_tensor(0))
    ms1 = torch.where(mutual1, ms0.gather(1, i1), z.new_tensor(0))
    valid0 = mutual0 & (ms0 > cfg["match_threshold"])
    valid1 = mutual1 & valid0.gather(1, i1)
    return {"matches0": torch.where(valid0, i0, -1), "matches1": torch.where(valid1, i1, -1),
            "matching_scores0": ms0, "matching_scores1": ms1}
