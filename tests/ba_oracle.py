"""numpy fp64 restatement of include/mapping/bundle_adjust.h: residual and Jacobian (a vectorised forward-mode dual through the
reference's expression graph), the normal-equation blocks, the Schur path, an independent dense path and the LM loop with the
same schedule.  Sums run in observation order (np.add.at is sequential), so a permuted observation list gives the fp64 noise
of a problem."""
import numpy as np

MU0, MU_MAX, MIN_RHO, DIAG_MIN, DIAG_MAX = 1e4, 1e16, 1e-3, 1e-6, 1e32
STATUS_OK, STATUS_NONFINITE_START = 0, 1


class Dual:
    """value [M] and derivative [M, 3] with respect to the three angle-axis entries"""

    __array_ufunc__ = None      # ndarray (op) Dual defers to the reflected operator below

    def __init__(self, v, d=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.d = np.zeros(self.v.shape + (3,)) if d is None else d

    @staticmethod
    def lift(x):
        return x if isinstance(x, Dual) else Dual(x)

    def __add__(self, o):
        o = Dual.lift(o)
        return Dual(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __sub__(self, o):
        o = Dual.lift(o)
        return Dual(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return Dual.lift(o) - self

    def __mul__(self, o):
        o = Dual.lift(o)
        return Dual(self.v * o.v, self.d * o.v[:, None] + self.v[:, None] * o.d)

    __rmul__ = __mul__

    def sqrt(self):
        s = np.sqrt(self.v)
        return Dual(s, self.d * (0.5 / s)[:, None])

    def recip(self):
        i = 1.0 / self.v
        return Dual(i, self.d * (-(i * i))[:, None])

    def sin(self):
        return Dual(np.sin(self.v), self.d * np.cos(self.v)[:, None])

    def cos(self):
        return Dual(np.cos(self.v), -(self.d * np.sin(self.v)[:, None]))


def _rotate(a, p):
    """tracking_utils.py:91-139 on duals a[3] and plain p [M,3]; both branches are evaluated and selected per row (the
    reference multiplies by a 0/1 mask; selecting is the same function and never mixes in a non-finite dead branch)."""
    theta2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    pos = theta2.v > 0
    safe = Dual(np.where(pos, theta2.v, 1.0), theta2.d)
    theta = safe.sqrt()
    s, c = theta.sin(), theta.cos()
    ti = theta.recip()
    w = [a[k] * ti for k in range(3)]
    x = [w[1] * p[:, 2] - w[2] * p[:, 1], w[2] * p[:, 0] - w[0] * p[:, 2], w[0] * p[:, 1] - w[1] * p[:, 0]]
    tmp = ((w[0] * p[:, 0] + w[1] * p[:, 1]) + w[2] * p[:, 2]) * (1.0 - c)
    full = [(c * p[:, k] + x[k] * s) + w[k] * tmp for k in range(3)]
    y = [a[1] * p[:, 2] - a[2] * p[:, 1], a[2] * p[:, 0] - a[0] * p[:, 2], a[0] * p[:, 1] - a[1] * p[:, 0]]
    first = [p[:, k] + y[k] for k in range(3)]
    out = [Dual(np.where(pos, full[k].v, first[k].v), np.where(pos[:, None], full[k].d, first[k].d)) for k in range(3)]
    # d / d p: the rotation matrix of the same branch
    cv, sv = np.where(pos, c.v, 1.0), np.where(pos, s.v, 1.0)
    wv = [np.where(pos, w[k].v, a[k].v) for k in range(3)]
    k1 = 1.0 - cv
    R = np.empty(p.shape[:1] + (3, 3))
    R[:, 0, 0] = cv + wv[0] * wv[0] * k1
    R[:, 0, 1] = wv[0] * wv[1] * k1 - wv[2] * sv
    R[:, 0, 2] = wv[0] * wv[2] * k1 + wv[1] * sv
    R[:, 1, 0] = wv[1] * wv[0] * k1 + wv[2] * sv
    R[:, 1, 1] = cv + wv[1] * wv[1] * k1
    R[:, 1, 2] = wv[1] * wv[2] * k1 - wv[0] * sv
    R[:, 2, 0] = wv[2] * wv[0] * k1 - wv[1] * sv
    R[:, 2, 1] = wv[2] * wv[1] * k1 + wv[0] * sv
    R[:, 2, 2] = cv + wv[2] * wv[2] * k1
    return out, R


def linearize(cams, intr, points, obs_cam, obs_pt, obs_xy):
    """r [M,2], Jc [M,2,6], Jp [M,2,3] and the predicted pixels [M,2]; every index must be in range."""
    cam, K, p = cams[obs_cam], intr[obs_cam], points[obs_pt]
    M = len(obs_cam)
    eye = np.eye(3)
    a = [Dual(cam[:, k], np.broadcast_to(eye[k], (M, 3)).copy()) for k in range(3)]
    q, R = _rotate(a, p)
    X, Y, Z = q[0].v + cam[:, 3], q[1].v + cam[:, 4], q[2].v + cam[:, 5]
    with np.errstate(all="ignore"):
        pred = np.stack([K[:, 0] * (X / Z) + K[:, 2], K[:, 1] * (Y / Z) + K[:, 3]], axis=1)
        r = pred - obs_xy
        iz = 1.0 / Z
        A = np.zeros((M, 2, 3))
        A[:, 0, 0] = K[:, 0] * iz
        A[:, 0, 2] = -(K[:, 0] * X * iz * iz)
        A[:, 1, 1] = K[:, 1] * iz
        A[:, 1, 2] = -(K[:, 1] * Y * iz * iz)
        dq = np.stack([q[0].d, q[1].d, q[2].d], axis=1)            # [M, 3 (component), 3 (angle-axis entry)]
        Jc = np.empty((M, 2, 6))
        Jp = np.empty((M, 2, 3))
        for row in range(2):
            for k in range(3):
                Jc[:, row, k] = (A[:, row, 0] * dq[:, 0, k] + A[:, row, 1] * dq[:, 1, k]) + A[:, row, 2] * dq[:, 2, k]
                Jc[:, row, 3 + k] = A[:, row, k]
                Jp[:, row, k] = (A[:, row, 0] * R[:, 0, k] + A[:, row, 1] * R[:, 1, k]) + A[:, row, 2] * R[:, 2, k]
    return r, Jc, Jp, pred


def in_range(obs_cam, obs_pt, C, P):
    return (obs_cam >= 0) & (obs_cam < C) & (obs_pt >= 0) & (obs_pt < P)


def masks(obs_cam, obs_pt, C, P, cam_fixed=None, pt_fixed=None):
    """(camera active [C], point active [P]): not fixed and observed"""
    cam_act = np.bincount(obs_cam, minlength=C) > 0
    pt_act = np.bincount(obs_pt, minlength=P) > 0
    if cam_fixed is not None:
        cam_act &= np.asarray(cam_fixed) == 0
    if pt_fixed is not None:
        pt_act &= np.asarray(pt_fixed) == 0
    return cam_act, pt_act


def normal_blocks(r, Jc, Jp, obs_cam, obs_pt, C, P, cam_fixed=None, pt_fixed=None):
    """U [C,6,6], V [P,3,3], g_c [C,6], g_p [P,3] (zeros for a fixed variable), cost; sums in observation order"""
    U, V = np.zeros((C, 6, 6)), np.zeros((P, 3, 3))
    g_c, g_p = np.zeros((C, 6)), np.zeros((P, 3))
    np.add.at(U, obs_cam, np.einsum("mka,mkb->mab", Jc, Jc))
    np.add.at(V, obs_pt, np.einsum("mka,mkb->mab", Jp, Jp))
    np.add.at(g_c, obs_cam, np.einsum("mka,mk->ma", Jc, r))
    np.add.at(g_p, obs_pt, np.einsum("mka,mk->ma", Jp, r))
    if cam_fixed is not None:
        U[np.asarray(cam_fixed) != 0] = 0
        g_c[np.asarray(cam_fixed) != 0] = 0
    if pt_fixed is not None:
        V[np.asarray(pt_fixed) != 0] = 0
        g_p[np.asarray(pt_fixed) != 0] = 0
    cost = 0.5 * float(np.sum(r * r))
    return U, V, g_c, g_p, cost


def cross_blocks(Jc, Jp, obs_cam, obs_pt, C, P):
    W = np.zeros((C, P, 6, 3))
    np.add.at(W, (obs_cam, obs_pt), np.einsum("mka,mkb->mab", Jc, Jp))
    return W


def clamp_diag(d):
    return np.minimum(np.maximum(d, DIAG_MIN), DIAG_MAX)


def dense_system(U, V, g_c, g_p, W, mu, cam_act, pt_act):
    """The full damped matrix A [(6C+3P)^2] and gradient g: (H + D^2 / mu) delta = -g, with the rows and columns of an
    inactive variable those of the identity and its gradient 0."""
    C, P = U.shape[0], V.shape[0]
    n = 6 * C + 3 * P
    A, g = np.zeros((n, n)), np.zeros(n)
    for c in range(C):
        A[6 * c:6 * c + 6, 6 * c:6 * c + 6] = U[c]
    for j in range(P):
        o = 6 * C + 3 * j
        A[o:o + 3, o:o + 3] = V[j]
        for c in range(C):
            A[6 * c:6 * c + 6, o:o + 3] = W[c, j]
            A[o:o + 3, 6 * c:6 * c + 6] = W[c, j].T
    g[:6 * C], g[6 * C:] = g_c.reshape(-1), g_p.reshape(-1)
    A[np.diag_indices(n)] += clamp_diag(np.diag(A)) / mu
    act = np.concatenate([np.repeat(cam_act, 6), np.repeat(pt_act, 3)])
    A[~act, :] = 0
    A[:, ~act] = 0
    A[~act, ~act] = 1
    g[~act] = 0
    return A, g


def step_dense(U, V, g_c, g_p, W, mu, cam_act, pt_act):
    A, g = dense_system(U, V, g_c, g_p, W, mu, cam_act, pt_act)
    d = np.linalg.solve(A, -g)
    C = U.shape[0]
    return d[:6 * C].reshape(C, 6), d[6 * C:].reshape(-1, 3)


def inverse_3x3(V):
    """closed form (adjugate / determinant) of symmetric 3x3 blocks [P,3,3], as the kernels invert them"""
    a, b, c, d, e, f = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2], V[:, 1, 1], V[:, 1, 2], V[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    det = (a * c00 + b * c01) + c * c02
    inv = np.empty_like(V)
    inv[:, 0, 0] = c00
    inv[:, 0, 1] = inv[:, 1, 0] = c01
    inv[:, 0, 2] = inv[:, 2, 0] = c02
    inv[:, 1, 1] = a * f - c * c
    inv[:, 1, 2] = inv[:, 2, 1] = b * c - a * e
    inv[:, 2, 2] = a * d - b * b
    return inv / det[:, None, None]


def step_schur(U, V, g_c, g_p, W, mu, cam_act, pt_act):
    """delta_c, delta_p through the Schur complement on the cameras, the header's path"""
    C, P = U.shape[0], V.shape[0]
    Vd = V.copy()
    idx = np.arange(3)
    Vd[:, idx, idx] += clamp_diag(V[:, idx, idx]) / mu
    Vd[~pt_act] = np.eye(3)
    Vinv = inverse_3x3(Vd)
    Wa = W * (cam_act[:, None, None, None] & pt_act[None, :, None, None])
    S = np.zeros((6 * C, 6 * C))
    for c in range(C):
        S[6 * c:6 * c + 6, 6 * c:6 * c + 6] = U[c]
    S[np.diag_indices(6 * C)] += clamp_diag(np.diag(S)) / mu
    WV = np.einsum("cjam,jmk->cjak", Wa, Vinv)
    S -= np.einsum("cjak,djbk->cadb", WV, Wa).reshape(6 * C, 6 * C)
    rhs = -g_c.reshape(-1) + np.einsum("cjak,jk->ca", WV, g_p).reshape(-1)
    act = np.repeat(cam_act, 6)
    S[~act, :] = 0
    S[:, ~act] = 0
    S[~act, ~act] = 1
    rhs[~act] = 0
    L = np.linalg.cholesky(S)
    dc = np.linalg.solve(L.T, np.linalg.solve(L, rhs)).reshape(C, 6)
    dp = -np.einsum("jmk,jk->jm", Vinv, g_p + np.einsum("cjam,ca->jm", Wa, dc))
    dp[~pt_act] = 0
    return dc, dp


def backward_error(A, g, delta):
    """eta = ||A delta + g||inf / (||A||inf ||delta||inf + ||g||inf)"""
    return float(np.abs(A @ delta + g).max() / (np.abs(A).sum(axis=1).max() * np.abs(delta).max() + np.abs(g).max()))


def model_decrease(r, Jc, Jp, obs_cam, obs_pt, dc, dp):
    u = np.einsum("mka,ma->mk", Jc, dc[obs_cam]) + np.einsum("mka,ma->mk", Jp, dp[obs_pt])
    return -float(np.sum(np.sum(r * u, axis=1) + 0.5 * np.sum(u * u, axis=1)))


def lm(cams, intr, points, obs_cam, obs_pt, obs_xy, cam_fixed=None, pt_fixed=None, num_iterations=5, num_success_iterations=5,
       dense=False):
    """The LM loop of the header.  Returns (cams, points, trace [num_iterations,6], summary [6])."""
    cams, points = np.array(cams, dtype=np.float64), np.array(points, dtype=np.float64)
    C, P, M = len(cams), len(points), len(obs_cam)
    ok = in_range(obs_cam, obs_pt, C, P)
    obs_cam, obs_pt, obs_xy = obs_cam[ok], obs_pt[ok], obs_xy[ok]
    cam_act, pt_act = masks(obs_cam, obs_pt, C, P, cam_fixed, pt_fixed)
    trace = np.zeros((num_iterations, 6))
    trace[:, 5] = -1
    mu, nu, n_acc, n_att, status = MU0, 2.0, 0, 0, STATUS_OK
    initial = final = None
    for it in range(num_iterations):
        r, Jc, Jp, _ = linearize(cams, intr, points, obs_cam, obs_pt, obs_xy)
        U, V, g_c, g_p, cost = normal_blocks(r, Jc, Jp, obs_cam, obs_pt, C, P, cam_fixed, pt_fixed)
        if it == 0:
            initial = final = cost
            if not np.isfinite(cost):
                status = STATUS_NONFINITE_START
                trace[0, 0] = cost
                break
        W = cross_blocks(Jc, Jp, obs_cam, obs_pt, C, P)
        dc, dp = (step_dense if dense else step_schur)(U, V, g_c, g_p, W, mu, cam_act, pt_act)
        md = model_decrease(r, Jc, Jp, obs_cam, obs_pt, dc, dp)
        rc, _, _, _ = linearize(cams + dc, intr, points + dp, obs_cam, obs_pt, obs_xy)
        cand = 0.5 * float(np.sum(rc * rc))
        with np.errstate(all="ignore"):
            rho = (cost - cand) / md
        accepted = bool(np.isfinite(cand) and md > 0 and rho > MIN_RHO)
        trace[it] = [cost, cand, md, rho, mu, float(accepted)]
        n_att += 1
        if accepted:
            u = 2.0 * rho - 1.0
            mu = min(mu / max(1.0 / 3.0, 1.0 - u * u * u), MU_MAX)
            nu = 2.0
            n_acc += 1
            final = cand
            cams[cam_act] += dc[cam_act]
            points[pt_act] += dp[pt_act]
            if n_acc >= num_success_iterations:
                break
        else:
            mu, nu = mu / nu, 2.0 * nu
    summary = np.array([initial, final, n_acc, n_att, M - int(ok.sum()), status], dtype=np.float64)
    return cams, points, trace, summary


def reproject(cams, intr, points, obs_cam, obs_pt):
    return linearize(cams, intr, points, obs_cam, obs_pt, np.zeros((len(obs_cam), 2)))[3]
