"""numpy fp64 restatement of the matcher's training head (include/gatsspg_train.h, "the mathematics") and of the reference's
reshape_assign_matrix (src/utils/data_utils.py:208-230).  TEST INFRASTRUCTURE ONLY: never imported by the product.

Pinned against the reference under autograd by tests/test_train_oracle_golden.py (tests/golden/train_*.npz, made by
tests/golden/make_train_golden.py from the unmodified reference); the GPU tests compare the HIP head with it at the same fp32 inputs."""
import numpy as np

NEGATIVE, POSITIVE, IGNORED = 0, 1, 2


def reshape_assign(pairs, n_orig, m_orig, n, m, pad_val=0):
    """conf_matrix_gt [n, m] int16 of one sample (pad=True branch).  pairs [2, k].  A pair with an index >= the shape is dropped,
    duplicates are one entry, the pad band is written last (also over a positive).  A negative index is ignored (the reference's
    indexing would wrap it around: the one stated difference)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(2, -1)
    out = np.zeros((n, m), dtype=np.int16)
    keep = (pairs[0] >= 0) & (pairs[1] >= 0) & (pairs[0] < n) & (pairs[1] < m)
    out[pairs[0][keep], pairs[1][keep]] = 1
    out[n_orig:] = pad_val
    out[:, m_orig:] = pad_val
    return out


def classes(target):
    """dense integer target -> 0 negative / 1 positive / 2 in neither mean"""
    target = np.asarray(target)
    return np.where(target == 1, POSITIVE, np.where(target == 0, NEGATIVE, IGNORED)).astype(np.int8)


def focal(C, cls, alpha, gamma):
    """(l, dl/dC) per entry, 0 where the entry is in neither mean"""
    l, g = np.zeros_like(C), np.zeros_like(C)
    pos, neg = cls == POSITIVE, cls == NEGATIVE
    with np.errstate(divide="ignore", invalid="ignore"):
        c = C[pos]
        l[pos] = -alpha * (1 - c) ** gamma * np.log(c)
        t = np.where(c == 1.0, 0.0, gamma * (1 - c) ** (gamma - 1) * np.log(c))
        g[pos] = alpha * (t - (1 - c) ** gamma / c)
        c = C[neg]
        l[neg] = -(1 - alpha) * c ** gamma * np.log(1 - c)
        g[neg] = (1 - alpha) * (-gamma * c ** (gamma - 1) * np.log(1 - c) + c ** gamma / (1 - c))
    return l, g


def scores_exp(x, y, scale):
    """E [b,n,m], r [b,n], c [b,m] in fp64 from the given (fp32) descriptors x [b,256,n], y [b,256,m]"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    E = np.exp(np.einsum("bdn,bdm->bnm", x, y) / scale)
    return E, E.sum(2), E.sum(1)


def loss_terms(E, r, c, cls, alpha, gamma, pos_w, neg_w):
    """From E, r, c (any precision, evaluated in fp64): dict(loss, loss_sums [2], counts [3], G, H, rowsum_h, colsum_h, A, B, C)"""
    E, r, c = (np.asarray(v, dtype=np.float64) for v in (E, r, c))
    A, B = E / c[:, None, :], E / r[:, :, None]
    C = A * B
    l, g = focal(C, cls, alpha, gamma)
    pos, neg = cls == POSITIVE, cls == NEGATIVE
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    sums = np.array([l[pos].sum(), l[neg].sum()])
    loss = 0.0
    G = np.zeros_like(C)
    if n_pos:
        loss += pos_w * sums[0] / n_pos
        G[pos] = pos_w / n_pos * g[pos]
    if n_neg:
        loss += neg_w * sums[1] / n_neg
        G[neg] = neg_w / n_neg * g[neg]
    H = G * C
    return dict(loss=loss, loss_sums=sums, counts=np.array([n_pos, n_neg, cls.size - n_pos - n_neg], dtype=np.int64), G=G, H=H,
                rowsum_h=H.sum(2), colsum_h=H.sum(1), A=A, B=B, C=C)


def score_grad(E, r, c, cls, counts, rowsum_h, colsum_h, alpha, gamma, pos_w, neg_w):
    """dS = 2 H - A colsum_j(H) - B rowsum_i(H) from the given stage inputs"""
    E, r, c, rowsum_h, colsum_h = (np.asarray(v, dtype=np.float64) for v in (E, r, c, rowsum_h, colsum_h))
    A, B = E / c[:, None, :], E / r[:, :, None]
    C = A * B
    _, g = focal(C, cls, alpha, gamma)
    w = np.zeros_like(C)
    if counts[0]:
        w[cls == POSITIVE] = pos_w / counts[0]
    if counts[1]:
        w[cls == NEGATIVE] = neg_w / counts[1]
    H = w * g * C
    return 2 * H - A * colsum_h[:, None, :] - B * rowsum_h[:, :, None]


def head(x, y, cls, alpha=0.5, gamma=2.0, pos_w=0.5, neg_w=0.5, scale=0.07):
    """The whole head in fp64: dict(loss, counts, dx, dy, E, r, c, dS, rowsum_h, colsum_h, loss_sums, C)"""
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    E, r, c = scores_exp(x64, y64, scale)
    t = loss_terms(E, r, c, cls, alpha, gamma, pos_w, neg_w)
    dS = 2 * t["H"] - t["A"] * t["colsum_h"][:, None, :] - t["B"] * t["rowsum_h"][:, :, None]
    dx = np.einsum("bdm,bnm->bdn", y64, dS) / scale
    dy = np.einsum("bdn,bnm->bdm", x64, dS) / scale
    return dict(loss=t["loss"], counts=t["counts"], dx=dx, dy=dy, E=E, r=r, c=c, dS=dS, rowsum_h=t["rowsum_h"], colsum_h=t["colsum_h"],
                loss_sums=t["loss_sums"], C=t["C"])


def make_head_case(b, n, m, k, seed, noise=0.8, n_orig=None, m_orig=None, pad_val=0, positives=True, negatives=True, pad_positive=False):
    """The input recipe of the head cases: unit-norm random descriptors, k positives per sample, half of them planted
    (y_j = x_i + noise * N(0, I), renormalised) and half unplanted.  -> x [b,256,n], y [b,256,m] fp32, pairs (list of [2,k] int32),
    target [b,n,m] int16 through reshape_assign.  positives=False: no pair; negatives=False: every non-positive entry gets
    pad_val 2 (in neither mean); pad_positive: one pair is put inside the pad band (which overwrites it)."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((b, 256, n))
    y = rs.standard_normal((b, 256, m))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    n_orig = n if n_orig is None else n_orig
    m_orig = m if m_orig is None else m_orig
    k = min(k, n_orig, m_orig) if positives else 0
    pairs = []
    for bi in range(b):
        i, j = rs.permutation(n_orig)[:k], rs.permutation(m_orig)[:k]
        for t in range(k // 2):
            v = x[bi, :, i[t]] + noise * rs.standard_normal(256)
            y[bi, :, j[t]] = v / np.linalg.norm(v)
        p = np.stack([i, j]).astype(np.int32)
        if pad_positive and (n_orig < n or m_orig < m):
            p = np.concatenate([p, np.array([[n - 1], [m - 1]], dtype=np.int32)], axis=1)
        pairs.append(p)
    x, y = x.astype(np.float32), y.astype(np.float32)
    target = np.stack([reshape_assign(p, n_orig, m_orig, n, m, pad_val) for p in pairs])
    if not negatives:
        target[target == 0] = 2
    return x, y, pairs, target


# ---- the cases of tests/test_training_gpu.py (here so that tests/golden/make_train_golden.py can run the reference on them) ----
DEFAULT = dict(alpha=0.5, gamma=2.0, pos_w=0.5, neg_w=0.5, scale=0.07)
# name -> (make_head_case arguments, focal arguments).  Tiles are 128 x 64: one short of a tile, exactly one, one over in both, a
# second partial tile, several tiles; (1,1,1) and (1,2,2) are the smallest problems.
GPU_CASES = {
    "1x1x1_only_positive": (dict(b=1, n=1, m=1, k=1, seed=1), DEFAULT),                                           # no negative; C == 1
    "1x1x1_neither": (dict(b=1, n=1, m=1, k=0, seed=2, positives=False, negatives=False), DEFAULT),
    "1x2x2": (dict(b=1, n=2, m=2, k=1, seed=3), DEFAULT),
    "1x127x63": (dict(b=1, n=127, m=63, k=12, seed=4, noise=0.8), DEFAULT),
    "3x128x64_ignored_band": (dict(b=3, n=128, m=64, k=10, seed=5, noise=0.7, n_orig=100, m_orig=50, pad_val=-1, pad_positive=True), DEFAULT),
    "2x129x65_pad0_gamma1.5": (dict(b=2, n=129, m=65, k=14, seed=6, noise=0.9, n_orig=120, m_orig=60, pad_val=0), dict(DEFAULT, gamma=1.5)),
    "1x130x70_no_positive_alpha0.25": (dict(b=1, n=130, m=70, k=0, seed=7, positives=False), dict(DEFAULT, alpha=0.25)),
    "1x130x70_no_negative": (dict(b=1, n=130, m=70, k=16, seed=8, noise=0.8, negatives=False), DEFAULT),
    "2x200x333": (dict(b=2, n=200, m=333, k=40, seed=9, noise=0.8), dict(DEFAULT, pos_w=0.7, neg_w=0.3)),
    "2x200x333_alpha0.25_gamma1.5": (dict(b=2, n=200, m=333, k=40, seed=10, noise=0.9, n_orig=190, m_orig=300, pad_val=-1),
                                     dict(DEFAULT, alpha=0.25, gamma=1.5)),
}
# the training-sized case of the hip-against-eager test (the reference's deviation on it is recorded with the others)
BIG_CASE_NAME, BIG_CASE = "2x1000x2000", dict(b=2, n=1000, m=2000, k=300, seed=11, noise=0.8)
