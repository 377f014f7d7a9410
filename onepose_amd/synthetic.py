"""Seeded synthetic weights and inputs for the GATsSPG matcher.

There is no checkpoint and no dataset in the build environment, so benchmarks and parity
tests run on random-init weights of the reference architecture and synthetic unit-norm
descriptors (real SuperPoint descriptors are unit-norm).  Everything here is
generated with ``numpy.random.RandomState`` so the very same tensors can be rebuilt bit for
bit on any machine (golden-vector generation in the build container, parity tests on the GPU
box) without shipping 22 MB of weights.

Parameter names / shapes follow the reference ``state_dict`` exactly
(src/models/GATsSPG_architectures/GATs_SuperGlue.py:145-177, GATs.py:25-28).
"""
from __future__ import annotations

import numpy as np

D = 256
GATS_LAYERS = (0, 3, 6, 9)
ATTN_LAYERS = (1, 2, 4, 5, 7, 8, 10, 11)


def _conv(rs, out_c, in_c):
    """PyTorch's default Conv1d init: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias."""
    bound = 1.0 / np.sqrt(in_c)
    w = rs.uniform(-bound, bound, size=(out_c, in_c, 1)).astype(np.float32)
    b = rs.uniform(-bound, bound, size=(out_c,)).astype(np.float32)
    return w, b


def make_state_dict(seed=0, keypoints_encoder=(32, 64, 128)):
    """Random-init weights with the distributions of the reference constructors
    (xavier_normal(gain=1.414) for GATs W/a, GATs.py:25-28; Conv1d default elsewhere; the last
    bias of every MLP zero, GATs_SuperGlue.py:109,136)."""
    rs = np.random.RandomState(seed)
    sd = {}
    for name, inp in (("kenc_2d", 3), ("kenc_3d", 4)):
        chans = [inp] + list(keypoints_encoder) + [D]
        for i in range(1, len(chans)):
            w, b = _conv(rs, chans[i], chans[i - 1])
            if i == len(chans) - 1:
                b[:] = 0
            sd[f"{name}.encoder.{3 * (i - 1)}.weight"] = w
            sd[f"{name}.encoder.{3 * (i - 1)}.bias"] = b
    for i in range(12):
        p = f"gnn.layers.{i}"
        if i in GATS_LAYERS:
            sd[f"{p}.W"] = (rs.standard_normal((D, D)) * 1.414 * np.sqrt(2.0 / (D + D))).astype(np.float32)
            sd[f"{p}.a"] = (rs.standard_normal((2 * D, 1)) * 1.414 * np.sqrt(2.0 / (2 * D + 1))).astype(np.float32)
        else:
            w, b = _conv(rs, D, D)
            sd[f"{p}.attn.merge.weight"], sd[f"{p}.attn.merge.bias"] = w, b
            for j in range(3):
                w, b = _conv(rs, D, D)
                sd[f"{p}.attn.proj.{j}.weight"], sd[f"{p}.attn.proj.{j}.bias"] = w, b
            w, b = _conv(rs, 2 * D, 2 * D)
            sd[f"{p}.mlp.0.weight"], sd[f"{p}.mlp.0.bias"] = w, b
            w, b = _conv(rs, D, 2 * D)
            b[:] = 0
            sd[f"{p}.mlp.3.weight"], sd[f"{p}.mlp.3.bias"] = w, b
    w, b = _conv(rs, D, D)
    sd["final_proj.weight"], sd["final_proj.bias"] = w, b
    sd["bin_score"] = np.array(1.0, dtype=np.float32)
    return sd


def make_passthrough_state_dict(seed=0):
    """Fixture-B weights: the last MLP conv of every AttentionPropagation layer
    is zeroed (deltas vanish) and final_proj is the identity, so planted descriptor matches
    survive the network and the dual-softmax produces confidences near 1."""
    sd = make_state_dict(seed)
    for i in ATTN_LAYERS:
        sd[f"gnn.layers.{i}.mlp.3.weight"][:] = 0
        sd[f"gnn.layers.{i}.mlp.3.bias"][:] = 0
    sd["final_proj.weight"] = np.eye(D, dtype=np.float32)[:, :, None].copy()
    sd["final_proj.bias"][:] = 0
    return sd


TRAINED_BASE_SEED = 21


def make_trained_state_dict(path=None):
    """TRAINED weights (round 5; tests/golden/make_trained_golden.py): the random-init state dict of seed 21 plus a
    rank-8 update of every weight matrix on the forward path and a full update of every bias, obtained by training the
    REFERENCE module with the reference's focal loss on planted synthetic frames (every AttentionPropagation delta and
    final_proj active -- nothing zeroed, unlike the pass-through fixture).  Only the factors are committed (~1 MB):
    `W = W_init + sum_k U[:, k] V[:, k]^T`, accumulated rank by rank in float64 with elementwise numpy ops (no BLAS: the
    summation order is fixed, so the container that ran the reference and the GPU box rebuild the same fp32 bits)."""
    import os
    if path is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "trained_lowrank.npz")
    fac = np.load(path)
    sd = make_state_dict(TRAINED_BASE_SEED)
    for key in fac.files:
        kind, name = key.split("::", 1)
        if kind == "B":
            sd[name] = (sd[name].astype(np.float64) + fac[key].astype(np.float64)).astype(np.float32)
        elif kind == "U":
            u, v = fac[key].astype(np.float64), fac["V::" + name].astype(np.float64)
            w = sd[name]
            acc = w.reshape(w.shape[0], -1).astype(np.float64)
            for k in range(u.shape[1]):
                acc = acc + u[:, k:k + 1] * v[None, :, k]
            sd[name] = acc.astype(np.float32).reshape(w.shape)
    return sd


def _unit(x, axis):
    return (x / np.linalg.norm(x, axis=axis, keepdims=True)).astype(np.float32)


def make_inputs(b, n1, n2, num_leaf=8, seed=1, planted=False, noise=(0.2, 0.3), with_targets=False):
    """Synthetic forward() inputs (keys of GATs_SuperGlue.py:181-189).

    planted=False: independent unit-norm random descriptors (benchmark distribution).
    planted=True (fixture B): leaves are noisy copies (noise norm ~0.2) of their 3D descriptor and
    the first n1//2 query descriptors are noisy copies (noise norm ~0.3) of distinct random 3D
    descriptors, so well-separated ground-truth matches exist.  `noise` = (leaf, query) noise norms.
    with_targets=True additionally returns the planted ground truth `[b, k]` (query i of sample bi matches
    3D point targets[bi, i]); the dict itself never changes.
    """
    rs = np.random.RandomState(seed)
    targets = []
    d3 = _unit(rs.standard_normal((b, D, n2)), 1)
    if planted:
        leaves = np.repeat(d3, num_leaf, axis=2) + noise[0] * rs.standard_normal((b, D, n2 * num_leaf)) / np.sqrt(D)
        d2db = _unit(leaves, 1)
        dq = _unit(rs.standard_normal((b, D, n1)), 1)
        k = min(n1 // 2, n2)
        for bi in range(b):
            tgt = rs.permutation(n2)[:k]
            dq[bi, :, :k] = _unit(d3[bi][:, tgt] + noise[1] * rs.standard_normal((D, k)) / np.sqrt(D), 0)
            targets.append(tgt)
    else:
        d2db = _unit(rs.standard_normal((b, D, n2 * num_leaf)), 1)
        dq = _unit(rs.standard_normal((b, D, n1)), 1)
    data = {
        "keypoints2d": (rs.rand(b, n1, 2) * 512).astype(np.float32),
        "keypoints3d": (rs.rand(b, n2, 3) - 0.5).astype(np.float32),
        "descriptors2d_query": dq,
        "descriptors3d_db": d3,
        "descriptors2d_db": d2db,
    }
    if with_targets:
        return data, (np.stack(targets) if targets else np.zeros((b, 0), np.int64))
    return data


# ---- SuperPoint extractor (src/models/extractors/SuperPoint/superpoint.py:115-133) ---------------
# (name, out channels, in channels, kernel size) in forward order; the state_dict holds
# "<name>.weight" [out, in, k, k] and "<name>.bias" [out].
SPP_LAYERS = (
    ("conv1a", 64, 1, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3),
    ("conv3a", 128, 64, 3), ("conv3b", 128, 128, 3), ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3),
    ("convPa", 256, 128, 3), ("convPb", 65, 256, 1), ("convDa", 256, 128, 3), ("convDb", 256, 256, 1),
)


def make_spp_state_dict(seed=0, descriptor_dim=256, logit_gain=6.0):
    """Random weights of the SuperPoint architecture.  He-normal (variance-preserving through the
    ReLU stack) instead of PyTorch's default init, and a larger gain on the detector's last
    conv, so that the 65-way cell softmax has a wide spread: keypoint scores then straddle the
    0.005 threshold and NMS decisions are separated by far more than fp32 rounding."""
    rs = np.random.RandomState(seed)
    sd = {}
    for name, oc, ic, k in SPP_LAYERS:
        if name == "convDb":
            oc = descriptor_dim
        std = np.sqrt(2.0 / (ic * k * k))
        if name == "convPb":
            std *= logit_gain
        sd[f"{name}.weight"] = (rs.standard_normal((oc, ic, k, k)) * std).astype(np.float32)
        sd[f"{name}.bias"] = (rs.standard_normal((oc,)) * 0.05).astype(np.float32)
    return sd


def make_image(b=1, h=512, w=512, seed=0):
    """Synthetic grayscale image batch [b, 1, h, w] in [0, 1]: overlapping rectangles and discs on a
    smooth gradient plus a little noise (corners and edges for the detector to respond to)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((b, 1, h, w), np.float32)
    for i in range(b):
        img = 0.3 + 0.2 * np.sin(xx / w * rs.uniform(2, 6)) * np.cos(yy / h * rs.uniform(2, 6))
        for _ in range(max(4, h * w // 4096)):
            cy, cx = rs.uniform(0, h), rs.uniform(0, w)
            ry, rx = rs.uniform(3, h / 6), rs.uniform(3, w / 6)
            val = rs.uniform(-0.4, 0.4)
            if rs.rand() < 0.5:
                m = (np.abs(yy - cy) < ry) & (np.abs(xx - cx) < rx)
            else:
                m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
            img = img + val * m
        img = img + rs.standard_normal((h, w)) * 0.02
        out[i, 0] = np.clip(img, 0, 1)
    return out


# ---- PnP (src/utils/eval_utils.py:18-42) ------------------------------------------------------------------
def make_pnp_problem(n=300, outlier_frac=0.3, noise_px=0.5, seed=0):
    """A synthetic 2D-3D correspondence set like the matcher's output: object points in a ~20 cm box (metres, as in
    the OnePose annotations), a random pose 0.4-0.8 m in front of a 512x512 crop camera, Gaussian pixel noise and a
    fraction of gross outliers.  -> dict(K [3,3], pts_3d [n,3], pts_2d [n,2], pose_gt [3,4], inlier_mask [n])."""
    rs = np.random.RandomState(seed)
    k = np.array([[600.0 + rs.uniform(-50, 50), 0, 256.0 + rs.uniform(-20, 20)],
                  [0, 600.0 + rs.uniform(-50, 50), 256.0 + rs.uniform(-20, 20)], [0, 0, 1.0]])
    pts = rs.uniform(-0.1, 0.1, size=(n, 3))
    a = rs.standard_normal((3, 3))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    t = np.array([rs.uniform(-0.05, 0.05), rs.uniform(-0.05, 0.05), rs.uniform(0.4, 0.8)])
    pc = pts @ q.T + t
    uv = np.stack([k[0, 2] + k[0, 0] * pc[:, 0] / pc[:, 2], k[1, 2] + k[1, 1] * pc[:, 1] / pc[:, 2]], axis=1)
    uv = uv + rs.standard_normal(uv.shape) * noise_px
    out = rs.rand(n) < outlier_frac
    uv[out] = rs.uniform(0, 512, size=(int(out.sum()), 2))
    return {"K": k, "pts_3d": pts.astype(np.float32), "pts_2d": uv.astype(np.float32),
            "pose_gt": np.concatenate([q, t[:, None]], axis=1), "inlier_mask": ~out}


def make_pose_pairs(seed=0, n=40):
    """(pose_pred, pose_gt) pairs whose rotation / translation errors straddle the 1, 3 and 5 cm-degree thresholds of the
    reference evaluator; every 7th prediction is given as a 4x4 matrix (cmd_evaluator.py:42-45)."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        t = rs.uniform(-0.3, 0.3, 3) + np.array([0, 0, 0.6])
        ang = rs.choice([0.2, 0.8, 2.0, 4.0, 8.0]) * np.pi / 180
        ax = rs.standard_normal(3)
        ax /= np.linalg.norm(ax)
        kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        dr = np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx
        dt = rs.choice([0.002, 0.008, 0.02, 0.04, 0.08]) * ax
        gt = np.concatenate([q, t[:, None]], 1)
        pred = np.concatenate([dr @ q, (t + dt)[:, None]], 1)
        if i % 7 == 0:
            pred = np.concatenate([pred, [[0, 0, 0, 1.0]]], 0)
        out.append((pred, gt))
    return out


# ---- object annotation files (src/sfm/postprocess/feature_process.py:191-194,357-363) --------------
def make_annotation(n=50, dim=256, seed=0, max_views=15):
    """Synthetic content of anno_3d_average.npz / anno_3d_collect.npz / idxs.npy: every 3D point has 1..max_views-1
    collected per-view descriptors (some fewer than num_leaf = 8, some more), concatenated point after point."""
    rs = np.random.RandomState(seed)
    idxs = rs.randint(1, max_views, size=n)
    k = int(idxs.sum())
    collect = rs.standard_normal((dim, k)).astype(np.float32)
    owner = np.repeat(np.arange(n), idxs)
    avg = np.stack([collect[:, owner == i].mean(axis=1) for i in range(n)], axis=1).astype(np.float32)
    return {"keypoints3d": (rs.rand(n, 3) - 0.5).astype(np.float32), "idxs": idxs, "owner": owner,
            "collect_descriptors": collect, "collect_scores": rs.rand(k, 1).astype(np.float32),
            "avg_descriptors": avg, "avg_scores": rs.rand(n, 1).astype(np.float32)}


def write_annotation(dirname, anno):
    """The three files inference.py:113-115 loads, in the reference's layout."""
    import os
    np.savez(os.path.join(dirname, "anno_3d_average.npz"), keypoints3d=anno["keypoints3d"], descriptors3d=anno["avg_descriptors"],
             scores3d=anno["avg_scores"])
    np.savez(os.path.join(dirname, "anno_3d_collect.npz"), keypoints3d=anno["keypoints3d"],
             descriptors3d=anno["collect_descriptors"], scores3d=anno["collect_scores"])
    np.save(os.path.join(dirname, "idxs.npy"), anno["idxs"])


# ---- SuperGlue 2D-2D matcher (src/models/matchers/SuperGlue/superglue.py:173-205) ----
SG_KENC = (3, 32, 64, 128, 256, 256)


def _bn(rs, prefix, c, sd):
    """BatchNorm1d in eval mode: random affine and running statistics with positive variance."""
    sd[prefix + ".weight"] = rs.uniform(0.5, 1.5, size=(c,)).astype(np.float32)
    sd[prefix + ".bias"] = rs.normal(0.0, 0.1, size=(c,)).astype(np.float32)
    sd[prefix + ".running_mean"] = rs.normal(0.0, 0.1, size=(c,)).astype(np.float32)
    sd[prefix + ".running_var"] = rs.uniform(0.5, 1.5, size=(c,)).astype(np.float32)
    sd[prefix + ".num_batches_tracked"] = np.array(0, dtype=np.int64)


def make_superglue_state_dict(seed=0, n_layers=18, delta_gain=0.3, kenc_gain=0.3, proj_gain=6.0, attn_gain=1.0):
    """Random SuperGlue weights in the reference state_dict order.  The last conv of every residual branch (kenc.encoder.12,
    gnn.layers.i.mlp.3) is scaled by kenc_gain / delta_gain so that activations stay O(1) through 18 residual layers; final_proj
    by proj_gain so that the score matrix is peaked enough for mutual matches above the thresholds; nonzero bin_score.
    attn_gain scales weight and bias of the q and k projections (attn.proj.0 / .1), so the attention logits scale by attn_gain^2:
    at 1 a row of logits spans ~0.02 and the softmax is flat; about 30 gives spreads of ~10 and peaked rows."""
    rs = np.random.RandomState(seed)
    sd = {"bin_score": np.array(rs.uniform(0.5, 1.5), dtype=np.float32)}
    j = 0
    for i in range(5):
        w, b = _conv(rs, SG_KENC[i + 1], SG_KENC[i])
        if i == 4:
            w, b = w * np.float32(kenc_gain), np.zeros_like(b)     # the reference zero-inits this bias (:77)
        sd[f"kenc.encoder.{j}.weight"], sd[f"kenc.encoder.{j}.bias"] = w, b
        if i < 4:
            _bn(rs, f"kenc.encoder.{j + 1}", SG_KENC[i + 1], sd)
        j += 3
    for li in range(n_layers):
        p = f"gnn.layers.{li}"
        sd[f"{p}.attn.merge.weight"], sd[f"{p}.attn.merge.bias"] = _conv(rs, D, D)
        for k in range(3):
            w, b = _conv(rs, D, D)
            if k < 2 and attn_gain != 1.0:
                w, b = w * np.float32(attn_gain), b * np.float32(attn_gain)
            sd[f"{p}.attn.proj.{k}.weight"], sd[f"{p}.attn.proj.{k}.bias"] = w, b
        sd[f"{p}.mlp.0.weight"], sd[f"{p}.mlp.0.bias"] = _conv(rs, 2 * D, 2 * D)
        _bn(rs, f"{p}.mlp.1", 2 * D, sd)
        w, _ = _conv(rs, D, 2 * D)
        sd[f"{p}.mlp.3.weight"], sd[f"{p}.mlp.3.bias"] = w * np.float32(delta_gain), np.zeros(D, np.float32)
    w, b = _conv(rs, D, D)
    sd["final_proj.weight"], sd["final_proj.bias"] = w * np.float32(proj_gain), b
    return sd


def make_superglue_passthrough_state_dict(seed=0, n_layers=18, proj_gain=16.0, bin_score=8.0):
    """Every delta is zero (kenc.encoder.12 and every mlp.3 are zero) and final_proj is proj_gain * identity, so the scores are
    proj_gain^2 / 16 * desc0^T desc1: with unit-norm inputs a planted pair (equal descriptors) scores 16, distractors ~ N(0, 1)."""
    sd = make_superglue_state_dict(seed, n_layers)
    for k in list(sd):
        if k.startswith("kenc.encoder.12.") or (k.startswith("gnn.layers.") and ".mlp.3." in k):
            sd[k] = np.zeros_like(sd[k])
    sd["final_proj.weight"] = (np.eye(D, dtype=np.float32) * np.float32(proj_gain))[:, :, None]
    sd["final_proj.bias"] = np.zeros(D, np.float32)
    sd["bin_score"] = np.array(bin_score, dtype=np.float32)
    return sd


def make_superglue_inputs(b, n0, n1, h, w, seed=1, planted=None, h1=None, w1=None):
    """Keypoints inside an h x w image (side 0) and an h1 x w1 image (side 1; default h x w), scores in (0, 1), unit-norm
    descriptors [b, 256, n].  planted = k: in each image k random pairs (planted0[:, t], planted1[:, t]) share a descriptor,
    every other point is a random distractor."""
    rs = np.random.RandomState(seed)
    h1 = h if h1 is None else h1
    w1 = w if w1 is None else w1
    out = {}
    for s, n, hh, ww in ((0, n0, h, w), (1, n1, h1, w1)):
        out[f"keypoints{s}"] = np.stack([rs.uniform(0, ww - 1, size=(b, n)), rs.uniform(0, hh - 1, size=(b, n))], -1).astype(np.float32)
        out[f"scores{s}"] = rs.uniform(0.01, 0.99, size=(b, n)).astype(np.float32)
        out[f"descriptors{s}"] = _unit(rs.normal(size=(b, D, n)).astype(np.float32), 1)
    out["image_size0"] = np.array([h, w], dtype=np.int64)
    out["image_size1"] = np.array([h1, w1], dtype=np.int64)
    if planted:
        k = int(planted)
        p0 = np.stack([rs.permutation(n0)[:k] for _ in range(b)])
        p1 = np.stack([rs.permutation(n1)[:k] for _ in range(b)])
        for i in range(b):
            out["descriptors1"][i][:, p1[i]] = out["descriptors0"][i][:, p0[i]]
        out["planted0"], out["planted1"] = p0.astype(np.int64), p1.astype(np.int64)
    return out


# ---- object database builder (run.py:80-163): a posed scan of a planted object ---------------------------------
def make_box_corners(half=(0.1, 0.1, 0.1)):
    """box3d_corners [8,3] in the reference's corner order as far as filter_points.py:43-45 uses it: the three edges
    that leave corner 4 end at the corners 5, 0 and 7."""
    hx, hy, hz = half
    c4 = np.array([-hx, -hy, -hz])
    ex, ey, ez = np.array([2 * hx, 0, 0]), np.array([0, 2 * hy, 0]), np.array([0, 0, 2 * hz])
    c = np.zeros((8, 3))
    c[4], c[5], c[0], c[7] = c4, c4 + ex, c4 + ey, c4 + ez
    c[1], c[6], c[3], c[2] = c4 + ex + ey, c4 + ex + ez, c4 + ey + ez, c4 + ex + ey + ez
    return c


def make_ring_poses(n_views, rs, radius=0.5):
    """World->camera poses [n,3,4] of cameras on a jittered ring around the origin, looking at it (x right, y down, z forward)."""
    poses = []
    for v in range(n_views):
        az = 2 * np.pi * v / n_views + rs.uniform(-0.05, 0.05)
        el = rs.uniform(0.2, 0.7)
        r = radius * rs.uniform(0.9, 1.1)
        c = r * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
        z = -c / np.linalg.norm(c)
        x = np.cross(z, np.array([0.0, 0.0, 1.0]))
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        rot = np.stack([x, y, z])
        poses.append(np.concatenate([rot, (-rot @ c)[:, None]], axis=1))
    return np.stack(poses)


def make_map_scene(n_points=300, n_views=12, hw=(96, 128), seed=0, noise_px=0.0, wrong_frac=0.0, dim=256, n_distract=20,
                   pairs_per_view=3, dropout=0.2, outside_frac=0.0):
    """A synthetic scan for the object database builder: points planted in a 20 cm box (``outside_frac`` of them outside it),
    ``n_views`` posed pinhole views on a ring, per view the fp32 keypoints of the visible points (plus ``noise_px`` Gaussian
    noise) and ``n_distract`` unmatched ones in random order, unit descriptors [dim, n_v], scores, and SuperGlue-like
    ``matches0`` for each view and its next ``pairs_per_view`` neighbours, ``wrong_frac`` of them redirected to a wrong keypoint
    more than 8 px away from the right one, whose own point projects more than 8 px away from the match's first keypoint.
    -> dict(points, box, Ks [V,3,3], poses [V,3,4], features [V] of dict(keypoints, descriptors, scores), kp_point [V] (planted
    point of each keypoint or -1), pair_matches [(i, j, matches0 int64 [n_i])], wrong [(pair, keypoint of i)])."""
    rs = np.random.RandomState(seed)
    h, w = hw
    pts = rs.uniform(-0.08, 0.08, size=(n_points, 3))
    n_out = int(round(outside_frac * n_points))
    if n_out:
        pts[:n_out, 2] = rs.uniform(0.11, 0.13, size=n_out)
    poses = make_ring_poses(n_views, rs)
    f = 2.2 * w
    Ks = np.stack([np.array([[f + rs.uniform(-3, 3), 0, w / 2 + rs.uniform(-2, 2)], [0, f + rs.uniform(-3, 3), h / 2 + rs.uniform(-2, 2)],
                             [0, 0, 1.0]]) for _ in range(n_views)])
    base = rs.standard_normal((n_points, dim))
    features, kp_point, proj = [], [], []
    for v in range(n_views):
        pc = pts @ poses[v, :, :3].T + poses[v, :, 3]
        uv = np.stack([Ks[v, 0, 0] * pc[:, 0] / pc[:, 2] + Ks[v, 0, 2], Ks[v, 1, 1] * pc[:, 1] / pc[:, 2] + Ks[v, 1, 2]], axis=1)
        uv = uv + rs.standard_normal(uv.shape) * noise_px
        proj.append(uv)
        vis = (uv[:, 0] > 1) & (uv[:, 0] < w - 2) & (uv[:, 1] > 1) & (uv[:, 1] < h - 2) & (rs.rand(n_points) > dropout)
        ids = np.concatenate([np.nonzero(vis)[0], np.full(n_distract, -1)])
        kp = np.concatenate([uv[vis], rs.uniform(2, [w - 3, h - 3], size=(n_distract, 2))])
        perm = rs.permutation(len(ids))
        ids, kp = ids[perm], kp[perm].astype(np.float32)
        d = np.where(ids[:, None] >= 0, base[np.maximum(ids, 0)], 0) + 0.1 * rs.standard_normal((len(ids), dim))
        d[ids < 0] = rs.standard_normal((int((ids < 0).sum()), dim))
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).T.astype(np.float32)
        features.append({"keypoints": kp, "descriptors": np.ascontiguousarray(d), "scores": rs.uniform(0.05, 1.0, len(ids)).astype(np.float32)})
        kp_point.append(ids)
    pairs = sorted({tuple(sorted((v, (v + k) % n_views))) for v in range(n_views) for k in range(1, pairs_per_view + 1)} - {(v, v) for v in range(n_views)})
    pair_matches, wrong = [], []
    for p, (i, j) in enumerate(pairs):
        where_j = {int(q): k for k, q in enumerate(kp_point[j]) if q >= 0}
        m0 = np.array([where_j.get(int(q), -1) if q >= 0 else -1 for q in kp_point[i]], np.int64)
        for a in np.nonzero(m0 >= 0)[0]:
            if rs.rand() < wrong_frac:
                # more than 8 px from the right keypoint, and planted where its own point lies more than 8 px from keypoint a
                right, qj = features[j]["keypoints"][m0[a]], kp_point[j]
                other = np.abs(proj[i][np.maximum(qj, 0)] - features[i]["keypoints"][a]).max(axis=1) > 8.0
                far = np.nonzero((np.abs(features[j]["keypoints"] - right).max(axis=1) > 8.0) & ((qj < 0) | other))[0]
                if len(far):
                    m0[a] = far[rs.randint(len(far))]
                    wrong.append((p, int(a)))
        pair_matches.append((i, j, m0))
    return {"points": pts, "box": make_box_corners(), "Ks": Ks, "poses": poses, "features": features, "kp_point": kp_point,
            "pair_matches": pair_matches, "wrong": wrong, "hw": hw}


def make_map_model(seed=0, n_images=40, n_points=600, dim=16, hw=(96, 128)):
    """A synthetic triangulated model for the post-processing stages of the database builder (what COLMAP hands to
    filter_tkl / filter_points / feature_process): two sequences of posed images, points around the 20 cm box (a tenth outside,
    a pair, a triple and a chain closer than 1 mm), tracks of 2..12 observations, per-image features of dimension ``dim``.
    -> dict(poses [V,3,4], seq_ids, xyz [T,3] float64, track_offsets, obs_image, obs_kpt, features, box, max_num_kp3d)."""
    rs = np.random.RandomState(seed)
    poses = make_ring_poses(n_images, rs)
    seq_ids = ["seq-1" if v < n_images // 2 else "seq-2" for v in range(n_images)]
    xyz = rs.uniform(-0.09, 0.09, size=(n_points, 3))
    xyz[rs.rand(n_points) < 0.1, 2] = 0.12
    step = np.array([0.0007, 0.0, 0.0])
    xyz[5] = xyz[2] + 0.3 * step
    xyz[11], xyz[20] = xyz[7] + 0.3 * step, xyz[7] - 0.3 * step
    xyz[14] = np.array([0.01, 0.02, 0.03])
    xyz[17], xyz[25] = xyz[14] + step, xyz[14] + 2 * step
    lengths = rs.randint(2, 13, size=n_points)
    lengths[[2, 5, 7, 11, 20, 14, 17, 25]] = 12
    lengths = np.minimum(lengths, n_images)                 # a track sees an image once: fewer than 12 images shorten it
    obs_image = np.concatenate([np.sort(rs.permutation(n_images)[:m]) for m in lengths]).astype(np.int32)
    per_image = np.bincount(obs_image, minlength=n_images)
    n_kpts = per_image + rs.randint(3, 9, size=n_images)
    slots = [list(rs.permutation(int(n))) for n in n_kpts]
    obs_kpt = np.array([slots[v].pop() for v in obs_image], np.int32)
    h, w = hw
    features = [{"keypoints": rs.uniform(0, [w, h], size=(int(n), 2)).astype(np.float32),
                 "descriptors": rs.standard_normal((dim, int(n))).astype(np.float32), "scores": rs.uniform(0.01, 1.0, int(n)).astype(np.float32)}
                for n in n_kpts]
    return {"poses": poses, "seq_ids": seq_ids, "xyz": xyz, "track_offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32),
            "obs_image": obs_image, "obs_kpt": obs_kpt, "features": features, "box": make_box_corners(), "max_num_kp3d": int(0.6 * n_points)}
