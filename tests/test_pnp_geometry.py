"""The EPnP core (epnp_solve in onepose_amd/csrc/pnp_kernels.hip, both instantiations) across object and view geometry, against the
numpy oracle and against bounds that come from the number formats (tests/pnp_geometry_cases.py; its conditions are asserted on the CPU
by tests/test_pnp_geometry_cases.py), and the rule for flat point sets: a pose that explains the points, or no pose.  Every output
buffer is poisoned before every call.  `pytest -s` prints the measured worst values over their bounds."""
import numpy as np
import pytest
import torch

import pnp_geometry_cases as gc
from onepose_amd import _native_pnp, pnp
from onepose_amd._binding import k_array

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
THR = 5.0
IDENTITY = np.eye(4)[:3]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def epnp(c, scale=gc.SCALE):
    """pnp_epnp over all correspondences of the case -> [3, 4] numpy, t in metres."""
    pose = torch.full((3, 4), 7.0, device=DEV, dtype=torch.float64)
    _native_pnp.call("pnp_epnp", DEV, gpu(c["pts_3d"]), gpu(c["pts_2d"]), k_array(c["K"]), float(scale), len(c["pts_3d"]), pose, None, 0)
    return pose.cpu().numpy()


def hypotheses(c, iterations, seed, scale=gc.SCALE):
    hyp = torch.full((iterations, 12), 7.0, device=DEV, dtype=torch.float64)
    _native_pnp.call("pnp_hypotheses", DEV, gpu(c["pts_3d"]), gpu(c["pts_2d"]), k_array(c["K"]), float(scale), len(c["pts_3d"]), iterations, seed, hyp)
    return hyp


def solve(c, iterations=64, seed=3, scale=gc.SCALE):
    """pnp_ransac_epnp from poisoned outputs -> (pose, mask, info) numpy."""
    n = len(c["pts_3d"])
    lib = _native_pnp.load()
    ws = torch.full((lib.pnp_workspace_bytes(n, iterations),), 0xA5, device=DEV, dtype=torch.uint8)
    pose = torch.full((3, 4), 7.0, device=DEV, dtype=torch.float64)
    mask = torch.full((n,), 7, device=DEV, dtype=torch.int32)
    info = torch.full((4,), -9, device=DEV, dtype=torch.int32)
    _native_pnp.call("pnp_ransac_epnp", DEV, gpu(c["pts_3d"]), gpu(c["pts_2d"]), k_array(c["K"]), float(scale), n, THR, iterations, seed, pose, mask,
                     info, ws, ws.numel())
    return pose.cpu().numpy(), mask.cpu().numpy(), info.cpu().numpy()


def solve_matches(c, iterations=64, seed=3, scale=gc.SCALE):
    """The _matches form: the correspondences among n + 3 query keypoints and n + 2 database points, in reversed database order."""
    n = len(c["pts_3d"])
    n1 = n + 3
    kp2 = np.full((n1, 2), 100.0, np.float32)
    q = np.arange(n) + (np.arange(n) >= n // 2) * 3                   # three unmatched keypoints in the middle
    kp2[q] = c["pts_2d"]
    kp3 = np.concatenate([np.full((2, 3), 0.5, np.float32), c["pts_3d"][::-1]])
    matches = -np.ones(n1, np.int64)
    matches[q] = n + 1 - np.arange(n)
    lib = _native_pnp.load()
    ws = torch.full((lib.pnp_workspace_bytes(n1, iterations),), 0xA5, device=DEV, dtype=torch.uint8)
    pose = torch.full((3, 4), 7.0, device=DEV, dtype=torch.float64)
    mask = torch.full((n1,), 7, device=DEV, dtype=torch.int32)
    info = torch.full((4,), -9, device=DEV, dtype=torch.int32)
    _native_pnp.call("pnp_ransac_epnp_matches", DEV, gpu(kp2), gpu(kp3), gpu(matches), n1, k_array(c["K"]), float(scale), THR, iterations, seed,
                     pose, mask, info, ws, ws.numel())
    return pose.cpu().numpy(), mask.cpu().numpy(), info.cpu().numpy(), q


def assert_rotation(pose, what):
    r = pose[:, :3]
    np.testing.assert_allclose(r @ r.T, np.eye(3), rtol=0, atol=1e-12, err_msg=what)
    assert abs(np.linalg.det(r) - 1.0) <= 1e-11, what


def assert_no_model(pose, mask, info, what, count=0):
    assert np.array_equal(pose, IDENTITY) and not mask.any() and info.tolist() == [0, 0, -1, count], f"{what}: {info.tolist()}"


class Worst:
    """The largest measured value over its bound, printed with pytest -s."""

    def __init__(self):
        self.v = {}

    def add(self, key, value, bound, what):
        ratio = value / bound
        if ratio > self.v.get(key, (-1.0,))[0]:
            self.v[key] = (ratio, value, bound, what)

    def show(self, title):
        for key, (ratio, value, bound, what) in self.v.items():
            print(f"{title}: worst {key} = {value:.3e} over its bound {bound:.3e} = {ratio:.4f} at {what}")


# ---- EPnP core, wave path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", list(gc.VIEWS))
def test_epnp_wave_path_over_objects_and_views(view):
    """pnp_epnp (NPTS = 0: the 64 lanes share the point loops) over every object at n in {6, 40, 65}, scale 1000: a rotation, the
    case's own points within E_MAX, and the oracle's pose within max(floor, 64 x spread) except where the case is reprojection-only."""
    worst = Worst()
    for obj, n, c in gc.benign_cases(view):
        what = f"{obj} / {view} / n = {n}"
        pose = epnp(c)
        assert np.isfinite(pose).all() and not np.array_equal(pose, IDENTITY), what
        assert_rotation(pose, what)
        e = gc.worst_reprojection(pose, c)
        worst.add("reprojection (px)", e, c["e_max"], what)
        if c["pose_to_pose"]:
            worst.add("|dR|", np.abs(pose[:, :3] - c["oracle"][:, :3]).max(), c["tol"][0], what)
            worst.add("|dt| (m)", np.abs(pose[:, 3] - c["oracle"][:, 3]).max(), c["tol"][1], what)
        assert e <= c["e_max"], f"{what}: {e:.3e} px"
        if c["pose_to_pose"]:
            np.testing.assert_allclose(pose[:, :3], c["oracle"][:, :3], rtol=0, atol=c["tol"][0], err_msg=what)
            np.testing.assert_allclose(pose[:, 3], c["oracle"][:, 3], rtol=0, atol=c["tol"][1], err_msg=what)
    worst.show(f"wave path, {view}")


# ---- EPnP core, thread path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", list(gc.VIEWS))
def test_epnp_thread_path_over_objects_and_views(view):
    """pnp_hypotheses (NPTS = 5: one thread per hypothesis) on FIVE correspondences, 64 hypotheses: each is a hash-ordered permutation
    of the same five points, so every row is finite, a rotation, and reprojects all five within E_MAX; pnp_epnp on the five too.  The
    poses are not compared: a 5-point null space is two-dimensional (tests/test_pnp_stages.py)."""
    worst = Worst()
    for obj, n, c in gc.benign_cases(view, (gc.N_THREAD,)):
        what = f"{obj} / {view} / n = 5"
        rows = hypotheses(c, 64, 3).cpu().numpy().reshape(64, 3, 4)
        assert np.isfinite(rows).all(), what
        rows[:, :, 3] /= gc.SCALE
        for h, row in enumerate(rows):
            assert_rotation(row, f"{what}, hypothesis {h}")
            worst.add("hypothesis reprojection (px)", gc.worst_reprojection(row, c), c["e_max"], f"{what}, hypothesis {h}")
        pose = epnp(c)
        assert np.isfinite(pose).all() and not np.array_equal(pose, IDENTITY), what
        assert_rotation(pose, what)
        worst.add("pnp_epnp reprojection (px)", gc.worst_reprojection(pose, c), c["e_max"], what)
    worst.show(f"thread path, {view}")
    for key, (ratio, value, bound, what) in worst.v.items():
        assert ratio <= 1.0, f"{key}: {value:.3e} px > {bound:.3e} px at {what}"


# ---- scale ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", list(gc.VIEWS))
def test_epnp_is_homogeneous_in_the_scale(view):
    """Scale 1 against scale 1000 (t in metres in both): within the case's pose bound, or both within E_MAX where the case is
    reprojection-only.  Scale 1024 against scale 1: BIT FOR BIT -- multiplying fp32 points by 2^10 is exact, every step of epnp_solve
    is homogeneous in the points (degree 0: alphas, M^T M, its null vectors, L, the rotation; degree 1: control points, betas, t;
    degree 2: covariance, rho) and every threshold in it is relative, the flatness guard included."""
    worst = Worst()
    for obj, n, c in gc.benign_cases(view):
        what = f"{obj} / {view} / n = {n}"
        p1000, p1, p1024 = epnp(c), epnp(c, 1.0), epnp(c, 1024.0)
        assert np.array_equal(p1024.view(np.int64), p1.view(np.int64)), f"{what}: scale 1024 and scale 1 differ by {np.abs(p1024 - p1).max():.3e}"
        assert_rotation(p1, what)
        e = gc.worst_reprojection(p1, c)
        worst.add("scale-1 reprojection (px)", e, c["e_max"], what)
        assert e <= c["e_max"], f"{what}: {e:.3e} px"
        if c["pose_to_pose"]:
            worst.add("|dR|", np.abs(p1[:, :3] - p1000[:, :3]).max(), c["tol"][0], what)
            worst.add("|dt| (m)", np.abs(p1[:, 3] - p1000[:, 3]).max(), c["tol"][1], what)
            np.testing.assert_allclose(p1[:, :3], p1000[:, :3], rtol=0, atol=c["tol"][0], err_msg=what)
            np.testing.assert_allclose(p1[:, 3], p1000[:, 3], rtol=0, atol=c["tol"][1], err_msg=what)
    worst.show(f"scale, {view}")


# ---- a pose or nothing ----------------------------------------------------------------------------------------------------------------
def assert_pose_or_nothing(pose, c, what, must_refuse, refused):
    if must_refuse:
        assert refused, f"{what}: a flat set got a pose"
    if not refused:
        assert np.isfinite(pose).all(), what
        assert_rotation(pose, what)
        e = gc.worst_reprojection(pose, c)
        assert e <= c["e_max"], f"{what}: a pose that misses its own points by {e:.3e} px"
    return refused


def test_pose_or_nothing_from_pnp_epnp():
    """Flat sets and the whole thin band: an exact identity, or a pose within E_MAX.  The flat sets must be refused."""
    refused = 0
    cases = gc.no_pose_or_good_cases()
    for label, c, must_refuse in cases:
        pose = epnp(c)
        refused += assert_pose_or_nothing(pose, c, label, must_refuse, np.array_equal(pose, IDENTITY))
    print(f"pnp_epnp: {refused} of {len(cases)} flat or thin sets refused")


def test_pose_or_nothing_from_pnp_hypotheses():
    """The n = 5 sets: every one of 64 rows is twelve NaNs or a pose of all five points within E_MAX."""
    refused = rows_seen = 0
    for label, c, must_refuse in gc.no_pose_or_good_cases():
        if len(c["pts_3d"]) != gc.N_THREAD:
            continue
        rows = hypotheses(c, 64, 3).cpu().numpy().reshape(64, 3, 4)
        nan = np.isnan(rows).reshape(64, 12)
        assert np.array_equal(nan.any(axis=1), nan.all(axis=1)), label
        rows[:, :, 3] /= gc.SCALE
        for h, row in enumerate(rows):
            refused += assert_pose_or_nothing(row, c, f"{label}, hypothesis {h}", must_refuse, bool(nan[h].all()))
            rows_seen += 1
    print(f"pnp_hypotheses: {refused} of {rows_seen} rows refused")


def test_pose_or_nothing_from_the_solves():
    """pnp_ransac_epnp and the _matches form: info[0] = info[1] = 0 with an identity pose (and, as pnp.h has it, a zero mask and
    info[2] = -1), or ok = 1 with a pose of ALL given points within E_MAX -- a refit of flat inliers never comes back ok."""
    refused = 0
    cases = gc.no_pose_or_good_cases()
    for label, c, must_refuse in cases:
        n = len(c["pts_3d"])
        pose, mask, info = solve(c)
        if info[0] == 0:
            assert info[1] == 0 and info[2] == -1 and np.array_equal(pose, IDENTITY) and not mask.any(), f"{label}: {info.tolist()}"
        else:
            assert info[0] == 1 and 5 <= info[1] == mask.sum() and set(np.unique(mask)) <= {0, 1}, f"{label}: {info.tolist()}"
        refused += assert_pose_or_nothing(pose, c, label, must_refuse, info[0] == 0)
        pose_m, mask_m, info_m, q = solve_matches(c)
        assert np.array_equal(pose_m.view(np.int64), pose.view(np.int64)) and np.array_equal(info_m, info), f"{label}: the _matches form differs"
        full = np.zeros(n + 3, np.int32)
        full[q] = mask                                                 # the database order is reversed, the query order is not
        assert np.array_equal(mask_m, full), label
    print(f"solves: {refused} of {len(cases)} flat or thin sets refused")


def test_pose_or_nothing_from_one_batch_of_32_mixed_frames():
    """One pnp_ransac_epnp_batch call: flat sets, thin-band slabs and benign objects side by side, cap 40 (the line holds 20).  Every
    frame is a pose or nothing, the flat ones nothing, the benign ones a pose; every frame is bitwise its own single-frame solve."""
    flat = [(label, c, True) for label, c, must in gc.no_pose_or_good_cases() if must and len(c["pts_3d"]) in (20, 40)][:10]
    band = [(label, c, False) for label, c, must in gc.no_pose_or_good_cases() if not must and len(c["pts_3d"]) == 40][::2][:18]
    good = [(f"{obj}/generic/n=40", gc.benign_case(obj, "generic", 40), None) for obj in ("box", "slab1e-05", "tilt1e-03", "rod")]
    frames = (flat + band + good)
    order = np.random.RandomState(5).permutation(len(frames))
    frames = [frames[i] for i in order]
    assert len(frames) == 32 and len(flat) == 10 and len(band) == 18
    p3 = np.full((32, 40, 3), np.nan, np.float32)
    p2 = np.full((32, 40, 2), np.nan, np.float32)
    counts = np.array([len(c["pts_3d"]) for _, c, _ in frames])
    for i, (_, c, _) in enumerate(frames):
        p3[i, :counts[i]], p2[i, :counts[i]] = c["pts_3d"], c["pts_2d"]
    pose, mask, info = pnp.ransac_pnp_batch(gc.K, gpu(p2), gpu(p3), counts=counts, scale=gc.SCALE, iterations=64, seeds=3)
    pose, mask, info = pose.cpu().numpy(), mask.cpu().numpy(), info.cpu().numpy()
    for i, (label, c, must_refuse) in enumerate(frames):
        what = f"frame {i}: {label}"
        if info[i, 0] == 0:
            assert_no_model(pose[i], mask[i], info[i], what, count=info[i, 3])
        assert_pose_or_nothing(pose[i], c, what, bool(must_refuse), info[i, 0] == 0)
        if must_refuse is None:
            assert info[i].tolist() == [1, 40, info[i, 2], 40], what
        alone = solve(c)
        assert np.array_equal(pose[i].view(np.int64), alone[0].view(np.int64)) and np.array_equal(info[i], alone[2]), what
        assert np.array_equal(mask[i, :counts[i]], alone[1]) and not mask[i, counts[i]:].any(), what


# ---- refusals end to end --------------------------------------------------------------------------------------------------------------
def test_a_planar_object_is_refused_end_to_end():
    """40 points on z = 0: every minimal sample is flat, so every hypothesis is NaN and counts nothing -> info = {0, 0, -1, 0}, the
    identity and a zero mask from pnp_ransac_epnp, from the _matches form, as one frame of a batch whose neighbours (box, slab, a
    4-point frame) are bitwise what they are alone (pnp_batch.h), and the identity with inliers == [] from ransac_PnP."""
    plane = gc.degenerate_case("plane0", "generic", 40)
    pose, mask, info = solve(plane, iterations=256)
    assert_no_model(pose, mask, info, "pnp_ransac_epnp")
    pose, mask, info, _ = solve_matches(plane, iterations=256)
    assert_no_model(pose, mask, info, "pnp_ransac_epnp_matches")
    box, slab = gc.benign_case("box", "generic", 40), gc.benign_case("slab1e-03", "corner", 40)
    four = dict(box, pts_3d=box["pts_3d"][:4], pts_2d=box["pts_2d"][:4])
    frames = [box, plane, slab, four]
    p3, p2 = np.full((4, 40, 3), np.nan, np.float32), np.full((4, 40, 2), np.nan, np.float32)
    counts = [40, 40, 40, 4]
    for i, c in enumerate(frames):
        p3[i, :counts[i]], p2[i, :counts[i]] = c["pts_3d"], c["pts_2d"]
    bp, bm, bi = (x.cpu().numpy() for x in pnp.ransac_pnp_batch(gc.K, gpu(p2), gpu(p3), counts=counts, scale=gc.SCALE, iterations=256, seeds=[3, 3, 4, 5]))
    assert_no_model(bp[1], bm[1], bi[1], "the planar frame of the batch")
    assert_no_model(bp[3], bm[3], bi[3], "the 4-point frame of the batch")
    for i, seed in ((0, 3), (2, 4)):
        pose, mask, info = solve(frames[i], iterations=256, seed=seed)
        assert info[0] == 1 and info[1] == 40
        assert np.array_equal(bp[i].view(np.int64), pose.view(np.int64)) and np.array_equal(bm[i], mask) and np.array_equal(bi[i], info), f"frame {i}"
    pose, homo, inliers = pnp.ransac_PnP(plane["K"], plane["pts_2d"], plane["pts_3d"], scale=1000, iterations=256)
    assert np.array_equal(pose, IDENTITY) and np.array_equal(homo, np.eye(4)) and inliers == []


# ---- the object on two faces ----------------------------------------------------------------------------------------------------------
def test_an_object_on_two_faces_loses_exactly_its_flat_samples():
    """20 points on z = 0 and 20 on x = 0: the samples po.sample_indices puts wholly in one face (about 6 %) are flat, and exactly
    those rows are NaN and count 0; every other row counts all 40; the solve is ok with the oracle's pose."""
    c = gc.two_faces_case()
    it = gc.TWO_FACES_ITERATIONS
    assert c["flat"].any() and (~c["flat"]).any()
    hyp = hypotheses(c, it, c["seed"])
    counts = torch.full((it,), -9, device=DEV, dtype=torch.int32)
    _native_pnp.call("pnp_score_hypotheses", DEV, gpu(c["pts_3d"]), gpu(c["pts_2d"]), k_array(c["K"]), gc.SCALE, 40, THR, hyp, it, counts)
    rows, counts = hyp.cpu().numpy(), counts.cpu().numpy()
    nan = np.isnan(rows)
    assert np.array_equal(nan.any(axis=1), nan.all(axis=1))
    np.testing.assert_array_equal(nan.all(axis=1), c["flat"])
    np.testing.assert_array_equal(counts, np.where(c["flat"], 0, 40))
    pose, mask, info = solve(c, iterations=it, seed=c["seed"])
    assert info.tolist() == [1, 40, int(np.argmin(c["flat"])), 40] and mask.all()
    print(f"two faces: {c['flat'].sum()} of {it} samples flat; |dR| = {np.abs(pose[:, :3] - c['oracle'][:, :3]).max():.3e} (bound {c['tol'][0]:.1e}), "
          f"|dt| = {np.abs(pose[:, 3] - c['oracle'][:, 3]).max():.3e} m (bound {c['tol'][1]:.1e})")
    np.testing.assert_allclose(pose[:, :3], c["oracle"][:, :3], rtol=0, atol=c["tol"][0])
    np.testing.assert_allclose(pose[:, 3], c["oracle"][:, 3], rtol=0, atol=c["tol"][1])


# ---- the refit refuses what the selection found ---------------------------------------------------------------------------------------
def select_and_refit(c, hyp, counts):
    n = len(c["pts_3d"])
    p3, p2, k = gpu(c["pts_3d"]), gpu(c["pts_2d"]), k_array(c["K"])
    mask = torch.full((n,), 7, device=DEV, dtype=torch.int32)
    idx = torch.full((n,), -1, device=DEV, dtype=torch.int32)
    info = torch.full((4,), -9, device=DEV, dtype=torch.int32)
    pose = torch.full((3, 4), 7.0, device=DEV, dtype=torch.float64)
    _native_pnp.call("pnp_select_best", DEV, p3, p2, k, gc.SCALE, n, THR, gpu(hyp), gpu(counts), len(counts), mask, idx, info)
    selected = (mask.cpu().numpy(), idx.cpu().numpy(), info.cpu().numpy())
    _native_pnp.call("pnp_refit", DEV, p3, p2, k, gc.SCALE, n, idx, mask, info, pose)
    return selected, (pose.cpu().numpy(), mask.cpu().numpy(), info.cpu().numpy())


def test_a_refit_that_refuses_leaves_the_no_model_state():
    """include/pnp.h: NO MODEL is one state whichever stage says so.  Crafted pnp_select_best input whose best hypothesis (the planted
    pose, crafted count 20) has exactly the 20 coplanar correspondences as inliers: the selection succeeds ({1, 20, 3, 20}, their
    mask), pnp_refit refuses them and leaves the identity, a ZERO mask and info = {0, 0, -1, 20} -- info[3] >= 5 is how a caller
    tells a refused refit from hypotheses that found nothing."""
    c = gc.refit_refusal_case()
    (mask_s, idx_s, info_s), (pose, mask, info) = select_and_refit(c, c["hyp"], c["counts"])
    want = np.zeros(40, np.int32)
    want[c["inliers"]] = 1
    assert info_s.tolist() == [1, 20, c["best"], 20] and np.array_equal(mask_s, want) and np.array_equal(idx_s[:20], c["inliers"])
    assert_no_model(pose, mask, info, "pnp_refit of coplanar inliers", count=20)


def test_a_refit_that_succeeds_changes_neither_mask_nor_info():
    """The other side of the same entry point: the box, every correspondence an inlier of the planted row -> pnp_refit writes the
    pose pnp_epnp gives for the listed correspondences, bitwise, and leaves mask and info as pnp_select_best wrote them."""
    c = gc.benign_case("box", "generic", 40)
    planted = np.array(c["pose_gt"])
    planted[:, 3] *= gc.SCALE
    hyp = np.tile(planted.reshape(12), (4, 1))
    counts = np.array([1, 40, 3, 40], np.int32)
    (mask_s, idx_s, info_s), (pose, mask, info) = select_and_refit(c, hyp, counts)
    assert info_s.tolist() == [1, 40, 1, 40] and mask_s.all() and np.array_equal(idx_s, np.arange(40))
    assert np.array_equal(info, info_s) and np.array_equal(mask, mask_s)
    assert np.array_equal(pose.view(np.int64), epnp(c).view(np.int64))
