"""numpy oracle of the flow step (include/detector/flow.h): pyramidal Lucas-Kanade in OpenCV's fixed-point arrangement, stated
in the header and restated here expression by expression in the kernel's order.  Everything that touches pixels is int64 (the
sums are exact, so their order does not matter); the per-point algebra is float64, one correctly rounded operation at a time,
which numpy never fuses.  Vectorised over the window, not over points or iterations.

Not OpenCV: cv2.calcOpticalFlowPyrLK keeps points and the 2x2 algebra in fp32 and accumulates in SIMD order (see the header).
"""
import numpy as np

from oracle.ransac_common import lane_tree_sum

KERNEL = np.array([1, 4, 6, 4, 1], np.int64)
W_BITS = 14
ONE = 1 << W_BITS                         # 16384: the bilinear weights sum to it
SCALE = 2.0 ** -20                        # A and b sums -> float64
MIN_DET = 2.0 ** -23
MIN_EIG_THRESHOLD = 1e-4
OSCILLATION = 0.01
EXIT_CONVERGED, EXIT_OSCILLATION, EXIT_ITERATION_CAP, EXIT_LEFT_RANGE, EXIT_REJECTED, EXIT_SKIPPED = range(6)
REPROJ_LANES = 256                        # FLOW_REPROJ_THREADS: the reduction order of flow_reproj_mean


def reflect101(x, n):
    """BORDER_REFLECT_101 (-1 -> 1, n -> n - 2), continued periodically; a 1-pixel axis maps everything to 0."""
    x = np.asarray(x, np.int64)
    if n == 1:
        return np.zeros_like(x)
    p = 2 * (n - 1)
    x = np.mod(x, p)
    return np.where(x >= n, p - x, x)


def pyr_down(img):
    """out(x, y) = (sum_ij k_i k_j I(2x + i - 2, 2y + j - 2) + 128) >> 8 on uint8 [H][W] -> [(H+1)/2][(W+1)/2]."""
    img = np.asarray(img)
    H, W = img.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    src = img.astype(np.int64)
    acc = np.zeros((h, w), np.int64)
    for j in range(5):
        rows = reflect101(2 * np.arange(h) + j - 2, H)
        for i in range(5):
            cols = reflect101(2 * np.arange(w) + i - 2, W)
            acc += KERNEL[i] * KERNEL[j] * src[np.ix_(rows, cols)]
    return ((acc + 128) >> 8).astype(np.uint8)


def pyramid_levels(H, W, win, max_level):
    """Number of levels (effective top level + 1): every level 1..l must be wider than win_w and higher than win_h."""
    n = 1
    while n <= max_level:
        W, H = (W + 1) // 2, (H + 1) // 2
        if not (W > win[0] and H > win[1]):
            break
        n += 1
    return n


def level_sizes(H, W, levels):
    out = [(H, W)]
    for _ in range(levels - 1):
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


class Pyramid:
    """The levels of one image and, on demand, their Scharr planes."""

    def __init__(self, img, levels):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        self.levels = [img]
        for _ in range(levels - 1):
            self.levels.append(pyr_down(self.levels[-1]))
        self._deriv = {}

    def packed(self):
        return np.concatenate([lv.reshape(-1) for lv in self.levels])

    def deriv(self, l):
        """(Ix, Iy) of level l: 3 / 10 / 3 Scharr with reflected neighbours."""
        if l not in self._deriv:
            img = self.levels[l].astype(np.int64)
            H, W = img.shape
            ym, y0, yp = reflect101(np.arange(H) - 1, H), np.arange(H), reflect101(np.arange(H) + 1, H)
            xm, x0, xp = reflect101(np.arange(W) - 1, W), np.arange(W), reflect101(np.arange(W) + 1, W)
            g = lambda r, c: img[np.ix_(r, c)]  # noqa: E731
            ix = 3 * (g(ym, xp) - g(ym, xm)) + 10 * (g(y0, xp) - g(y0, xm)) + 3 * (g(yp, xp) - g(yp, xm))
            iy = 3 * (g(yp, xm) - g(ym, xm)) + 10 * (g(yp, x0) - g(ym, x0)) + 3 * (g(yp, xp) - g(ym, xp))
            self._deriv[l] = (ix, iy)
        return self._deriv[l]


def in_range(ip, size, win):
    """The range test of a window origin against a level of size (H, W)."""
    return bool(ip[0] >= -win[0] and ip[0] < size[1] and ip[1] >= -win[1] and ip[1] < size[0])


def weights(a, b):
    w00 = int(np.rint((1.0 - a) * (1.0 - b) * ONE))
    w01 = int(np.rint(a * (1.0 - b) * ONE))
    w10 = int(np.rint((1.0 - a) * b * ONE))
    return w00, w01, w10, ONE - w00 - w01 - w10


def window_origin(pos, win):
    """c = pos - half, ip = floor(c), (a, b) = c - ip."""
    half = np.array([(win[0] - 1) / 2, (win[1] - 1) / 2])
    c = np.asarray(pos, np.float64) - half
    ip = np.floor(c)
    frac = c - ip
    return ip, frac


def _as_int(ip):
    return int(ip[0]), int(ip[1])


def sample_image(img, ip, w, win):
    """(patch + 256) >> 9 over the window: 5 fractional bits."""
    H, W = img.shape
    x, y = _as_int(ip)
    xs, ys = x + np.arange(win[0] + 1), y + np.arange(win[1] + 1)
    blk = img[np.ix_(reflect101(ys, H), reflect101(xs, W))].astype(np.int64)
    patch = blk[:-1, :-1] * w[0] + blk[:-1, 1:] * w[1] + blk[1:, :-1] * w[2] + blk[1:, 1:] * w[3]
    return (patch + 256) >> 9


def sample_deriv(plane, ip, w, win):
    """(patch + 8192) >> 14 over the window; the derivative is 0 outside the level."""
    H, W = plane.shape
    x, y = _as_int(ip)
    xs, ys = x + np.arange(win[0] + 1), y + np.arange(win[1] + 1)
    inside = np.outer((ys >= 0) & (ys < H), (xs >= 0) & (xs < W))
    blk = np.where(inside, plane[np.ix_(np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1))], 0)
    patch = blk[:-1, :-1] * w[0] + blk[:-1, 1:] * w[1] + blk[1:, :-1] * w[2] + blk[1:, 1:] * w[3]
    return (patch + 8192) >> 14


def patch_sums(pyr, level, pos, win):
    """(A11, A12, A22) as Python ints and the ival / ix / iy patches [win_h][win_w] int64 at one position of one level; None when
    the window origin fails the range test."""
    img = pyr.levels[level]
    ip, frac = window_origin(pos, win)
    if not in_range(ip, img.shape, win):
        return None
    w = weights(frac[0], frac[1])
    dx, dy = pyr.deriv(level)
    ival, ix, iy = sample_image(img, ip, w, win), sample_deriv(dx, ip, w, win), sample_deriv(dy, ip, w, win)
    return (int((ix * ix).sum()), int((ix * iy).sum()), int((iy * iy).sum())), ival, ix, iy


def mismatch_sums(pyr_i, pyr_j, level, prev, nxt, win, patches=None):
    """(B1, B2) for one pair of positions; None when either window origin fails the range test."""
    if patches is None:
        patches = patch_sums(pyr_i, level, prev, win)
        if patches is None:
            return None
    _, ival, ix, iy = patches
    img = pyr_j.levels[level]
    ip, frac = window_origin(nxt, win)
    if not in_range(ip, img.shape, win):
        return None
    diff = sample_image(img, ip, weights(frac[0], frac[1]), win) - ival
    return int((diff * ix).sum()), int((diff * iy).sum())


def _rel(x, t):
    return abs(x - t) / abs(t)


def track(pyr_i, pyr_j, pts, init=None, win=(15, 15), max_iter=10, eps=0.03, min_eig_threshold=MIN_EIG_THRESHOLD):
    """pts [n][2] float32 -> next [n][2] float32, status [n] int32, matches0 [n] int64, trace [n][levels][2] int32
    ({iterations run, exit code}), margins: how close any decision came to its threshold (the exactness conditions)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n, levels = len(pts), len(pyr_i.levels)
    assert len(pyr_j.levels) == levels
    L = levels - 1
    out = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.int32)
    trace = np.zeros((n, levels, 2), np.int32)
    margins = {"min_eig": np.inf, "det": np.inf, "eps": np.inf, "oscillation": np.inf}
    area2 = float(2 * win[0] * win[1])
    eps2 = eps * eps
    for i in range(n):
        p = pts[i].astype(np.float64)
        nxt = None
        for l in range(L, -1, -1):
            size = pyr_i.levels[l].shape
            prev = p * 2.0 ** -l
            if l == L:
                nxt = (p if init is None else np.asarray(init, np.float32)[i].astype(np.float64)) * 2.0 ** -L
            else:
                nxt = 2.0 * nxt
            patches = patch_sums(pyr_i, l, prev, win)
            if patches is None:
                if l == 0:
                    status[i] = 0
                trace[i, l] = (0, EXIT_SKIPPED)
                continue
            (A11, A12, A22), ival, ix, iy = patches
            a11, a12, a22 = A11 * SCALE, A12 * SCALE, A22 * SCALE
            D = a11 * a22 - a12 * a12
            min_eig = (a22 + a11 - np.sqrt((a11 - a22) * (a11 - a22) + 4.0 * a12 * a12)) / area2
            margins["min_eig"] = min(margins["min_eig"], _rel(min_eig, min_eig_threshold))
            margins["det"] = min(margins["det"], _rel(D, MIN_DET))
            if min_eig < min_eig_threshold or D < MIN_DET:
                if l == 0:
                    status[i] = 0
                trace[i, l] = (0, EXIT_REJECTED)
                continue
            pd = np.zeros(2)
            code, ran = EXIT_ITERATION_CAP, 0
            for j in range(max_iter):
                b = mismatch_sums(pyr_i, pyr_j, l, prev, nxt, win, patches)
                if b is None:
                    if l == 0:
                        status[i] = 0
                    code = EXIT_LEFT_RANGE
                    break
                ran = j + 1
                b1, b2 = b[0] * SCALE, b[1] * SCALE
                d = np.array([(a12 * b2 - a22 * b1) / D, (a12 * b1 - a11 * b2) / D])
                nxt = nxt + d
                d2 = d[0] * d[0] + d[1] * d[1]
                if eps2 > 0:
                    margins["eps"] = min(margins["eps"], _rel(d2, eps2))
                if d2 <= eps2:
                    code = EXIT_CONVERGED
                    break
                if j > 0:
                    s = np.abs(d + pd)
                    margins["oscillation"] = min(margins["oscillation"], float(np.abs(s - OSCILLATION).min()))
                    if s[0] < OSCILLATION and s[1] < OSCILLATION:
                        nxt = nxt - 0.5 * d
                        code = EXIT_OSCILLATION
                        break
                pd = d
            trace[i, l] = (ran, code)
        if status[i]:
            ip, _ = window_origin(nxt, win)
            if not in_range(ip, pyr_i.levels[0].shape, win):
                status[i] = 0
        out[i] = nxt.astype(np.float32)
    matches0 = np.where(status == 1, np.arange(n), -1).astype(np.int64)
    return out, status, matches0, trace, margins


def reproj_mean(pose, K, pts3d, pts2d, status, dtype=np.float64):
    """(mean ||project(X, K, pose) - x|| over status == 1, count) in the kernel's order: thread t adds points t, t + 256, ..
    in turn, then the fixed tree.  project = tracking_utils.project: (R X + t), then K, then the division."""
    P, Km = np.asarray(pose, dtype), np.asarray(K, dtype).reshape(3, 3)
    X, x = np.asarray(pts3d, np.float32).astype(dtype), np.asarray(pts2d, np.float32).astype(dtype)
    lanes = np.zeros(REPROJ_LANES, dtype)
    count = 0
    for i in range(len(X)):
        if status[i] != 1:
            continue
        c = [((P[r, 0] * X[i, 0] + P[r, 1] * X[i, 1]) + P[r, 2] * X[i, 2]) + P[r, 3] for r in range(3)]
        h = [(Km[r, 0] * c[0] + Km[r, 1] * c[1]) + Km[r, 2] * c[2] for r in range(3)]
        ex, ey = h[0] / h[2] - x[i, 0], h[1] / h[2] - x[i, 1]
        lanes[i % REPROJ_LANES] = lanes[i % REPROJ_LANES] + np.sqrt(ex * ex + ey * ey)
        count += 1
    total = lane_tree_sum(lanes, REPROJ_LANES)   # one value a lane: wg::tree_sum alone
    with np.errstate(invalid="ignore", divide="ignore"):
        return total / dtype(count), count
