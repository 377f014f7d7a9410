"""Case builders of the bundle-adjustment tests.  Every builder asserts its own preconditions from the oracle on the CPU, so a
case that stops meaning what it says fails loudly, and computes the oracle's answers once (functools.lru_cache): the tests
share them and leave them unchanged."""
import functools

import numpy as np

import ba_oracle as bo

CAMERA_CHUNK = 256            # BA_CAMERA_CHUNK: observations one pass of the per-camera kernels covers
F, CX, CY = 600.0, 320.0, 240.0

# Norm-wise gap ||J_oracle - J_reference|| / ||J_reference|| per observation, the largest over the golden's observations,
# measured when the oracle was written (tests/test_ba_oracle_golden.py prints it).  The bound used by every Jacobian
# comparison is 16 times it, floored at 2^-40: the margin allows for sin / cos differing by an ulp between libraries.
JACOBIAN_GAP_MEASURED = 2.93e-16
JACOBIAN_BOUND = max(16 * JACOBIAN_GAP_MEASURED, 2.0 ** -40)
RESIDUAL_ULPS = 64            # of the predicted pixel coordinate

GOLDEN_ANGLES = (0.0, 1e-8, 1e-3, 1.0, np.pi - 1e-3)
GOLDEN_PER_ANGLE = 60


def golden_inputs():
    """One camera and one point per observation: cams [M,6], points [M,3], features [M,5] = (x, y, f, cx, cy) as the
    reference's residual function takes them.  Rotation angles exactly 0, 1e-8, 1e-3, about 1 and pi - 1e-3."""
    rng = np.random.default_rng(20240917)
    cams, points, feats = [], [], []
    for angle in GOLDEN_ANGLES:
        for k in range(GOLDEN_PER_ANGLE):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            a = angle * (1.0 + (0.2 * rng.uniform(-1, 1) if angle == 1.0 else 0.0))
            t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)])
            cams.append(np.concatenate([axis * a, t]))
            points.append(rng.uniform(-0.15, 0.15, 3))
            feats.append([rng.uniform(0, 640), rng.uniform(0, 480), rng.uniform(400, 900), rng.uniform(300, 340), rng.uniform(220, 260)])
    cams, points, feats = np.array(cams), np.array(points), np.array(feats)
    assert np.all(cams[:GOLDEN_PER_ANGLE, :3] == 0.0)
    return cams, points, feats


def golden_problem(feats):
    """The golden's inputs as the C ABI takes them: intr [M,4], obs_cam = obs_pt = 0 .. M-1, obs_xy [M,2]"""
    M = len(feats)
    intr = np.stack([feats[:, 2], feats[:, 2], feats[:, 3], feats[:, 4]], axis=1)
    idx = np.arange(M, dtype=np.int32)
    return np.ascontiguousarray(intr), idx, idx.copy(), np.ascontiguousarray(feats[:, :2])


def jacobian_gap(Jc, Jp, Jc_ref, Jp_ref):
    """largest over the observations of ||J - J_ref||_F / ||J_ref||_F, J = [Jc | Jp]"""
    J = np.concatenate([Jc, Jp], axis=2).reshape(len(Jc), -1)
    Jr = np.concatenate([Jc_ref, Jp_ref], axis=2).reshape(len(Jc), -1)
    return float(np.max(np.linalg.norm(J - Jr, axis=1) / np.linalg.norm(Jr, axis=1)))


def residual_ulps(r, r_ref, pred):
    """largest |r - r_ref| in ulps of the predicted pixel coordinate"""
    return float(np.max(np.abs(r - r_ref) / np.spacing(np.abs(pred))))


def _scene(C, P, seed, rot=0.3):
    rng = np.random.default_rng(seed)
    points = rng.uniform(-0.1, 0.1, (P, 3))
    cams = np.concatenate([rng.uniform(-rot, rot, (C, 3)), rng.uniform(-0.05, 0.05, (C, 2)), rng.uniform(0.5, 0.7, (C, 1))], axis=1)
    intr = np.tile([F, F, CX, CY], (C, 1))
    return rng, cams, intr, points


def _project(cams, intr, points, obs_cam, obs_pt):
    return bo.reproject(cams, intr, points, obs_cam, obs_pt)


class Problem:
    def __init__(self, cams, intr, points, obs_cam, obs_pt, obs_xy, cam_fixed=None, pt_fixed=None):
        self.cams, self.intr, self.points = cams, intr, points
        self.obs_cam, self.obs_pt, self.obs_xy = obs_cam.astype(np.int32), obs_pt.astype(np.int32), np.ascontiguousarray(obs_xy)
        self.cam_fixed = None if cam_fixed is None else np.asarray(cam_fixed, dtype=np.int32)
        self.pt_fixed = None if pt_fixed is None else np.asarray(pt_fixed, dtype=np.int32)
        self.C, self.P, self.M = len(cams), len(points), len(obs_cam)

    def permuted(self, seed=7):
        perm = np.random.default_rng(seed).permutation(self.M)
        return Problem(self.cams, self.intr, self.points, self.obs_cam[perm], self.obs_pt[perm], self.obs_xy[perm], self.cam_fixed,
                       self.pt_fixed), perm

    def args(self):
        return self.cams, self.intr, self.points, self.obs_cam, self.obs_pt, self.obs_xy

    def linearized(self):
        r, Jc, Jp, _ = bo.linearize(*self.args())
        return r, Jc, Jp

    def blocks(self):
        r, Jc, Jp = self.linearized()
        return bo.normal_blocks(r, Jc, Jp, self.obs_cam, self.obs_pt, self.C, self.P, self.cam_fixed, self.pt_fixed)

    def active(self):
        return bo.masks(self.obs_cam, self.obs_pt, self.C, self.P, self.cam_fixed, self.pt_fixed)

    def system(self, mu):
        """(A, g, U, V, g_c, g_p, W) of the damped system at mu"""
        r, Jc, Jp = self.linearized()
        U, V, g_c, g_p, _ = self.blocks()
        W = bo.cross_blocks(Jc, Jp, self.obs_cam, self.obs_pt, self.C, self.P)
        A, g = bo.dense_system(U, V, g_c, g_p, W, mu, *self.active())
        return A, g, U, V, g_c, g_p, W

    def lm(self, **kw):
        return bo.lm(*self.args(), cam_fixed=self.cam_fixed, pt_fixed=self.pt_fixed, **kw)


@functools.lru_cache(maxsize=None)
def blocks_case(cam0_count=149):
    """C = 3, P = 65: point 0 has no observation, point 1 one, point 2 two, point 3 thirty-three (all by camera 0: duplicates
    from one camera are legal); camera 1 has one observation, camera 2 none, camera 0 exactly ``cam0_count``."""
    C, P = 3, 65
    rng, cams, intr, points = _scene(C, P, 11)
    obs_cam = [0, 0, 1] + [0] * 33
    obs_pt = [1, 2, 2] + [3] * 33
    k = 0
    while obs_cam.count(0) < cam0_count:
        obs_cam.append(0)
        obs_pt.append(4 + k % (P - 4))
        k += 1
    obs_cam, obs_pt = np.array(obs_cam), np.array(obs_pt)
    xy = _project(cams, intr, points, obs_cam, obs_pt) + rng.normal(scale=0.7, size=(len(obs_cam), 2))
    pb = Problem(cams, intr, points, obs_cam, obs_pt, xy)
    n_cam, n_pt = np.bincount(pb.obs_cam, minlength=C), np.bincount(pb.obs_pt, minlength=P)
    assert list(n_cam) == [cam0_count, 1, 0] and list(n_pt[:4]) == [0, 1, 2, 33] and n_pt[4:].min() >= 1
    assert np.isfinite(pb.blocks()[4])
    return pb


@functools.lru_cache(maxsize=None)
def tiny_case():
    """C = 2, P = 1, M = 2"""
    rng, cams, intr, points = _scene(2, 1, 12)
    obs_cam, obs_pt = np.array([0, 1]), np.array([0, 0])
    xy = _project(cams, intr, points, obs_cam, obs_pt) + rng.normal(scale=0.7, size=(2, 2))
    return Problem(cams, intr, points, obs_cam, obs_pt, xy)


def _visibility(rng, C, P, single=0):
    """every point seen by 2 .. C cameras (the first ``single`` points by one), every camera used"""
    obs_cam, obs_pt = [], []
    for j in range(P):
        k = 1 if j < single else int(rng.integers(2, C + 1))
        for c in sorted(rng.choice(C, size=k, replace=False)):
            obs_cam.append(c)
            obs_pt.append(j)
    obs_cam, obs_pt = np.array(obs_cam), np.array(obs_pt)
    order = rng.permutation(len(obs_cam))
    return obs_cam[order], obs_pt[order]


@functools.lru_cache(maxsize=None)
def planted_case(C):
    """No noise, two cameras fixed (the gauge), a perturbed start, 30 iterations: the truth is the answer.  Returns
    (problem at the start, true cams, true points, mask of the points with >= 2 observations, the oracle's lm result)."""
    P = 60
    rng, cams, intr, points = _scene(C, P, 20 + C)
    obs_cam, obs_pt = _visibility(rng, C, P, single=3)
    xy = _project(cams, intr, points, obs_cam, obs_pt)
    fixed = np.zeros(C, dtype=np.int32)
    fixed[:2] = 1
    start_cams = cams + (fixed[:, None] == 0) * np.concatenate([rng.normal(scale=0.01, size=(C, 3)), rng.normal(scale=0.005, size=(C, 3))], axis=1)
    start_points = points + rng.normal(scale=0.003, size=(P, 3))
    pb = Problem(start_cams, intr, start_points, obs_cam, obs_pt, xy, cam_fixed=fixed)
    seen2 = np.bincount(obs_pt, minlength=P) >= 2
    assert seen2.sum() == P - 3
    out = pb.lm(num_iterations=30, num_success_iterations=30)
    assert np.abs(out[0] - cams).max() <= 1e-10 and np.abs(out[1][seen2] - points[seen2]).max() <= 1e-10, "the oracle misses the truth"
    return pb, cams, points, seen2, out


def relative_spread(a, b, floor):
    """|a - b| relative to |a|, elementwise, floored: the fp64 noise of a problem between two summation orders"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.maximum(np.abs(a - b) / np.maximum(np.abs(a), np.finfo(np.float64).tiny), floor)


@functools.lru_cache(maxsize=None)
def reference_case(kind):
    """The solve as the reference calls it: nothing fixed, 0.5 px noise, 5 / 5 iterations.  kind: "plain"; "rejecting" (a
    start bad enough that the oracle rejects at least one step); "zero_rotation" (camera 0 at exactly zero rotation).
    Returns (problem, oracle result, oracle result on the permuted observation list, the permutation)."""
    C, P = 5, 60
    rng, cams, intr, points = _scene(C, P, {"plain": 31, "rejecting": 44, "zero_rotation": 33}[kind])
    if kind == "zero_rotation":
        cams[0, :3] = 0.0
    obs_cam, obs_pt = _visibility(rng, C, P)
    xy = _project(cams, intr, points, obs_cam, obs_pt) + rng.normal(scale=0.5, size=(len(obs_cam), 2))
    scale = 25.0 if kind == "rejecting" else 1.0        # 25 x: the Gauss-Newton-sized first steps overshoot and two are rejected
    start_cams = cams + scale * np.concatenate([rng.normal(scale=0.01, size=(C, 3)), rng.normal(scale=0.005, size=(C, 3))], axis=1)
    if kind == "zero_rotation":
        start_cams[0, :3] = 0.0
    start_points = points + scale * rng.normal(scale=0.003, size=(P, 3))
    pb = Problem(start_cams, intr, start_points, obs_cam, obs_pt, xy)
    out = pb.lm(num_iterations=5, num_success_iterations=5)
    trace = out[2]
    attempted = trace[:, 5] >= 0
    assert attempted.all() and np.isfinite(trace[:, :3]).all()
    assert np.abs(trace[:, 3] - bo.MIN_RHO).min() >= 1e-2, "a rho too close to the threshold: a flip would be legitimate"
    if kind == "rejecting":
        assert (trace[:, 5] == 0).any() and (trace[:, 5] == 1).any(), "the oracle rejects no step"
    else:
        assert (trace[:, 5] == 1).all()
    if kind == "zero_rotation":
        assert np.all(pb.cams[0, :3] == 0.0)
    pp, perm = pb.permuted()
    out_perm = pp.lm(num_iterations=5, num_success_iterations=5)
    assert np.array_equal(out_perm[2][:, 5], trace[:, 5])
    return pb, out, out_perm, perm


def spread_rule(x, ref, ref_perm, floor, factor=32.0):
    """The comparison rule of the solve tests, in the max norm relative to ||ref||: (distance of x from ref, the bound
    max(factor * distance of the oracle's two orderings, floor))."""
    x, ref, ref_perm = (np.asarray(a, dtype=np.float64) for a in (x, ref, ref_perm))
    scale = max(float(np.abs(ref).max()), np.finfo(np.float64).tiny)
    return float(np.abs(x - ref).max()) / scale, max(factor * float(np.abs(ref - ref_perm).max()) / scale, floor)


def block_rule(x, ref, ref_perm, factor=32.0, floor=2.0 ** -40):
    """The comparison rule of the normal blocks, block by block (leading axis) in the Frobenius norm: (distances of x from
    ref [n], bounds max(factor * spread of the oracle's two orderings, floor * ||ref block||) [n])."""
    flat = lambda a: np.asarray(a, dtype=np.float64).reshape(len(a), -1)  # noqa: E731
    x, ref, ref_perm = flat(x), flat(ref), flat(ref_perm)
    return np.linalg.norm(x - ref, axis=1), np.maximum(factor * np.linalg.norm(ref - ref_perm, axis=1), floor * np.linalg.norm(ref, axis=1))


def step_eta_bound(pb, mu):
    """(A, g, the bound 16 * max(eta of the oracle's own Schur path, n 2^-53), the oracle's eta) of the damped system at mu"""
    A, g, U, V, g_c, g_p, W = pb.system(mu)
    dc, dp = bo.step_schur(U, V, g_c, g_p, W, mu, *pb.active())
    eta = bo.backward_error(A, g, np.concatenate([dc.reshape(-1), dp.reshape(-1)]))
    return A, g, 16.0 * max(eta, len(g) * 2.0 ** -53), eta


@functools.lru_cache(maxsize=None)
def wide_case(C, P, used_points, seed):
    """A gauge-fixed noisy problem whose observed points are ``used_points`` of the P (the rest unobserved): for the camera
    limit (C = 32) and for point indices past 4095 (a third radix pass).  Returns (problem, the oracle's 3-iteration result)."""
    rng, cams, intr, points = _scene(C, P, seed)
    used = np.asarray(used_points)
    obs_cam, obs_pt = [], []
    for j in used:
        for c in sorted(rng.choice(C, size=3, replace=False)):
            obs_cam.append(c)
            obs_pt.append(j)
    for c in range(C):                      # every camera sees at least four points
        for j in used[(c + np.arange(4)) % len(used)]:
            obs_cam.append(c)
            obs_pt.append(j)
    obs_cam, obs_pt = np.array(obs_cam), np.array(obs_pt)
    order = rng.permutation(len(obs_cam))
    obs_cam, obs_pt = obs_cam[order], obs_pt[order]
    xy = _project(cams, intr, points, obs_cam, obs_pt) + rng.normal(scale=0.5, size=(len(obs_cam), 2))
    fixed = np.zeros(C, dtype=np.int32)
    fixed[:2] = 1
    start = cams + (fixed[:, None] == 0) * np.concatenate([rng.normal(scale=0.005, size=(C, 3)), rng.normal(scale=0.002, size=(C, 3))], axis=1)
    pb = Problem(start, intr, points + rng.normal(scale=0.002, size=(P, 3)), obs_cam, obs_pt, xy, cam_fixed=fixed)
    out = pb.lm(num_iterations=3, num_success_iterations=3)
    assert (out[2][:, 5] == 1).all() and np.isfinite(out[2]).all()
    return pb, out
