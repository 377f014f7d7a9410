"""numpy restatement of the training-set builder (include/gatsspg_trainset.h), stage by stage, from the header's text: the hash, the
pair rule, the leaf selection, the gather and the two pads.  Integer arithmetic and copies only, so the GPU tests compare bit for
bit.  Also ``check_leaves``, the property checker that the reference's own selections and this oracle's pass alike.
TEST INFRASTRUCTURE ONLY: a plain module the tests import."""
import numpy as np

from oracle.ransac_common import _splitmix64 as sm

M64 = (1 << 64) - 1
DESC_DIM, MAX_REDRAWS = 256, 256
TAG_LEAVES, TAG_PAD2D, TAG_PAD3D = 1, 2, 3


# ---- the hash ----
def stream_key(seed, tag, epoch, image, item):
    h = sm(int(seed) & M64)
    for word in (tag, int(epoch) & 0xFFFFFFFF, int(image) & 0xFFFFFFFF, int(item) & 0xFFFFFFFF):
        h = sm(h ^ word)
    return h


def draw64(key, ctr):
    return sm((key + ctr) & M64)


def draw_index(key, ctr, n):
    return int((draw64(key, ctr) >> 11) % n)


# ---- pairs ----
def assign_pairs(point_offsets, obs_image, obs_kpt, kpt_offsets):
    """-> (pair_offsets [V+1], pair_kpt, pair_point, ignored): the lowest keypoint of a point in an image; the lower point wins a
    keypoint; an observation outside its image is ignored and counted."""
    V = len(kpt_offsets) - 1
    n_kpts = np.diff(kpt_offsets)
    owner = [dict() for _ in range(V)]
    ignored = 0
    for p in range(len(point_offsets) - 1):
        best = {}
        for j in range(point_offsets[p], point_offsets[p + 1]):
            v, q = int(obs_image[j]), int(obs_kpt[j])
            if not (0 <= v < V and 0 <= q < n_kpts[v]):
                ignored += 1
                continue
            best[v] = min(best.get(v, q), q)
        for v, q in best.items():
            owner[v][q] = min(owner[v].get(q, p), p)
    offsets, kpt, point = [0], [], []
    for o in owner:
        for q in sorted(o):
            kpt.append(q)
            point.append(o[q])
        offsets.append(len(kpt))
    return np.array(offsets, np.int32), np.array(kpt, np.int32), np.array(point, np.int32), ignored


# ---- leaves ----
def select_point(key, start, cnt, L):
    """the L slots of one point: rows of collect, or -1"""
    out, ctr = [-1] * L, 0
    if cnt < L:
        used = set()
        for j in range(cnt):
            while True:
                slot = draw_index(key, ctr, L)
                ctr += 1
                if slot not in used:
                    break
            used.add(slot)
            out[slot] = start + j
    else:
        chosen = []
        while len(chosen) < L:
            v = start + draw_index(key, ctr, cnt)
            ctr += 1
            if v not in chosen:
                chosen.append(v)
        out = chosen
    return out


def select_leaves(point_offsets, sample_image, sample_epoch, shape3d, L, seed):
    """-> leaf_src [b, shape3d * L] int32"""
    N = len(point_offsets) - 1
    out = np.full((len(sample_image), shape3d, L), -1, np.int32)
    for s, (v, e) in enumerate(zip(sample_image, sample_epoch)):
        for p in range(min(N, shape3d)):
            start, cnt = int(point_offsets[p]), max(int(point_offsets[p + 1] - point_offsets[p]), 0)
            out[s, p] = select_point(stream_key(seed, TAG_LEAVES, e, v, p), start, cnt, L)
    return out.reshape(len(sample_image), shape3d * L)


def gather_leaves(collect, leaf_src):
    """collect [K, 256] -> [b, 256, M]; the dustbin is all ones"""
    table = np.concatenate([np.asarray(collect, np.float32), np.ones((1, collect.shape[1]), np.float32)])
    src = np.where((leaf_src >= 0) & (leaf_src < len(collect)), leaf_src, len(collect))
    return np.ascontiguousarray(table[src].transpose(0, 2, 1))


def check_leaves(sel, idxs, L, shape3d):
    """``sel`` [shape3d * L]: per slot a row of collect, or a dustbin mark (-1, or anything >= sum(idxs): the reference's dustbin id).
    Per point, the non-dustbin entries are distinct and lie inside the point's range, their number is min(cnt, L); pad points are
    all dustbin."""
    idxs = np.asarray(idxs, np.int64)
    sel = np.asarray(sel, np.int64).reshape(shape3d, L)
    upper = np.cumsum(idxs)
    lower = upper - idxs
    K = int(upper[-1]) if len(idxs) else 0
    for p in range(shape3d):
        real = sel[p][(sel[p] >= 0) & (sel[p] < K)]
        assert ((sel[p] >= -1)).all(), (p, sel[p])
        if p >= len(idxs):
            assert len(real) == 0, (p, sel[p])
            continue
        assert len(real) == min(int(idxs[p]), L), (p, sel[p], idxs[p])
        assert len(set(real.tolist())) == len(real), (p, sel[p])
        assert ((real >= lower[p]) & (real < upper[p])).all(), (p, sel[p], lower[p], upper[p])
    return True


# ---- pads ----
def pad_query(features, image_hw, sample_image, sample_epoch, shape2d, seed):
    """features: per image dict(keypoints [n,2], descriptors [256,n], scores [n]) -> (descriptors2d_query [b,256,shape2d], keypoints2d
    [b,shape2d,2], scores [b,shape2d])"""
    b, V = len(sample_image), len(features)
    dq = np.ones((b, DESC_DIM, shape2d), np.float32)
    kq = np.zeros((b, shape2d, 2), np.float32)
    sq = np.zeros((b, shape2d), np.float32)
    for s, (v, e) in enumerate(zip(sample_image, sample_epoch)):
        inside = 0 <= v < V
        kp = np.asarray(features[v]["keypoints"], np.float32).reshape(-1, 2) if inside else np.zeros((0, 2), np.float32)
        h, w = (max(int(image_hw[v][0]), 1), max(int(image_hw[v][1]), 1)) if inside else (1, 1)
        n = min(len(kp), shape2d)
        if n:
            dq[s, :, :n] = np.asarray(features[v]["descriptors"], np.float32)[:, :n]
            kq[s, :n] = kp[:n]
            sq[s, :n] = np.asarray(features[v]["scores"], np.float32).reshape(-1)[:n]
        own = set(map(tuple, kp.tolist()))
        for j in range(len(kp), shape2d):
            key = stream_key(seed, TAG_PAD2D, e, v, j)
            for attempt in range(MAX_REDRAWS):
                c = (float(draw_index(key, 2 * attempt, h)), float(draw_index(key, 2 * attempt + 1, w)))
                if c not in own:
                    break
            kq[s, j] = c
    return dq, kq, sq


def pad_points(points3d, mean_desc, sample_image, sample_epoch, shape3d, seed):
    """points3d [N,3], mean_desc [256,N] -> (keypoints3d [b,shape3d,3], descriptors3d_db [b,256,shape3d])"""
    b, N = len(sample_image), len(points3d)
    n = min(N, shape3d)
    k3 = np.zeros((b, shape3d, 3), np.float32)
    d3 = np.ones((b, DESC_DIM, shape3d), np.float32)
    k3[:, :n] = np.asarray(points3d, np.float32)[:n]
    d3[:, :, :n] = np.asarray(mean_desc, np.float32)[:, :n]
    for s, (v, e) in enumerate(zip(sample_image, sample_epoch)):
        for j in range(N, shape3d):
            key = stream_key(seed, TAG_PAD3D, e, v, j)
            k3[s, j] = [np.float32(draw64(key, c) >> 40) * np.float32(2.0 ** -24) - np.float32(0.5) for c in range(3)]
    return k3, d3


def build_batch(case, sample_image, sample_epoch, shape2d, shape3d, L, seed):
    """the whole chain on a case of ``make_case`` -> dict of the six outputs"""
    leaf_src = select_leaves(case["point_offsets"], sample_image, sample_epoch, shape3d, L, seed)
    dq, kq, sq = pad_query(case["features"], case["image_hw"], sample_image, sample_epoch, shape2d, seed)
    k3, d3 = pad_points(case["points3d"], case["mean_desc"], sample_image, sample_epoch, shape3d, seed)
    return dict(leaf_src=leaf_src, descriptors2d_db=gather_leaves(case["collect"], leaf_src), descriptors2d_query=dq, keypoints2d=kq,
                scores_query=sq, keypoints3d=k3, descriptors3d_db=d3)


# ---- cases ----
def make_case(N, counts, n_kpts, hw=(24, 32), seed=0, stray=4):
    """A small object: N points whose observation counts cycle through ``counts`` (0 allowed), images with ``n_kpts`` keypoints each
    (integer positions, so that a random pad can coincide with one).  The observations are drawn with replacement: a point may see an
    image through several keypoints (the lowest is its pair) and two points may see one keypoint (the lower point wins); ``stray`` of
    them are moved outside their image (image -1 or V, keypoint -1 or n_v)."""
    rs = np.random.RandomState(seed)
    V = len(n_kpts)
    cnt = [int(counts[p % len(counts)]) for p in range(N)]
    offsets = np.concatenate([[0], np.cumsum(cnt)])
    K = max(int(offsets[-1]), 1)
    seen = [v for v in range(V) if n_kpts[v] > 0]
    obs_image = rs.choice(seen, size=K).astype(np.int32)
    obs_kpt = np.array([rs.randint(n_kpts[v]) for v in obs_image], np.int32)
    for i, j in enumerate(rs.permutation(K)[:stray]):
        if i % 2:
            obs_image[j] = (-1, V)[i // 2 % 2]
        else:
            obs_kpt[j] = (-1, n_kpts[obs_image[j]])[i // 2 % 2]
    h, w = hw
    features = []
    for n in n_kpts:
        pos = rs.permutation(h * w)[:n]
        features.append({"keypoints": np.stack([pos // w, pos % w], axis=1).astype(np.float32).reshape(-1, 2),      # column 0 < h, column 1 < w
                         "descriptors": rs.standard_normal((DESC_DIM, n)).astype(np.float32), "scores": rs.uniform(0.1, 1, n).astype(np.float32)})
    collect = rs.standard_normal((K, DESC_DIM)).astype(np.float32)
    collect[:, 0] = np.arange(K)                                      # a row can be read back from its first channel
    return dict(point_offsets=offsets.astype(np.int32), obs_image=obs_image, obs_kpt=obs_kpt, collect=collect, points3d=rs.uniform(-0.1, 0.1, (N, 3)).astype(np.float32), mean_desc=rs.standard_normal((DESC_DIM, N)).astype(np.float32),
                features=features, image_hw=np.array([hw] * V, np.int32), kpt_offsets=np.concatenate([[0], np.cumsum(n_kpts)]).astype(np.int32))


def tables(case):
    """the case as the flat tables of the C ABI (numpy): name -> array"""
    f = case["features"]
    return dict(point_offsets=case["point_offsets"], obs_image=case["obs_image"], obs_kpt=case["obs_kpt"], collect=case["collect"],
                points3d=case["points3d"], mean_desc=case["mean_desc"], kpt_offsets=case["kpt_offsets"], image_hw=case["image_hw"],
                desc2d=np.concatenate([x["descriptors"].reshape(-1) for x in f] + [np.zeros(0, np.float32)]),
                kpts2d=np.concatenate([x["keypoints"].reshape(-1, 2) for x in f]).astype(np.float32),
                scores2d=np.concatenate([x["scores"].reshape(-1) for x in f]).astype(np.float32))
