"""The pose solver's kernels stage by stage through the stage entry points of include/pnp.h (pnp_hypotheses, pnp_score_hypotheses,
pnp_select_best) against the numpy restatement in tests/pnp_cases.py.  Everything downstream of the hypotheses is discrete and is
compared exactly; every case meets the conditions of pnp_cases (asserted on the CPU by tests/test_pnp_cases.py)."""
import functools

import numpy as np
import pytest
import torch

import pnp_cases as pc
from onepose_amd import _native_pnp, pnp
from onepose_amd._binding import k_array

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def hypotheses(c, iterations, seed):
    hyp = torch.full((iterations, 12), 7.0, device=DEV, dtype=torch.float64)
    _native_pnp.call("pnp_hypotheses", DEV, gpu(c["pts_3d"]), gpu(c["pts_2d"]), k_array(c["K"]), pc.SCALE, len(c["pts_3d"]), iterations, seed, hyp)
    return hyp


def score(c, hyp):
    hyp = hyp if isinstance(hyp, torch.Tensor) else gpu(hyp)
    counts = torch.full((hyp.shape[0],), -9, device=DEV, dtype=torch.int32)
    _native_pnp.call("pnp_score_hypotheses", DEV, gpu(c["pts_3d"]), gpu(c["pts_2d"]), k_array(c["K"]), pc.SCALE, len(c["pts_3d"]), pc.THR, hyp,
                     hyp.shape[0], counts)
    return counts


def select(c, hyp, counts):
    """-> (mask [n], inlier_idx [n], info [4]) as numpy; the outputs start out dirty."""
    hyp = hyp if isinstance(hyp, torch.Tensor) else gpu(hyp)
    counts = counts if isinstance(counts, torch.Tensor) else gpu(counts)
    n = len(c["pts_3d"])
    mask = torch.full((n,), 7, device=DEV, dtype=torch.int32)
    idx = torch.full((n,), -1, device=DEV, dtype=torch.int32)
    info = torch.full((4,), -9, device=DEV, dtype=torch.int32)
    _native_pnp.call("pnp_select_best", DEV, gpu(c["pts_3d"]), gpu(c["pts_2d"]), k_array(c["K"]), pc.SCALE, n, pc.THR, hyp, counts, hyp.shape[0],
                     mask, idx, info)
    return mask.cpu().numpy(), idx.cpu().numpy(), info.cpu().numpy()


# ---- score_kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.SCORE_N)
def test_score_kernel_counts_equal_the_restated_inlier_test(n):
    """counts[h] for EVERY h, over hypotheses from the planted pose to far off it, at the edges of the 64-lane pass (n) and of the
    four hypotheses per workgroup (iterations).  Planted rows: twelve NaNs count 0; [I | -p_k scale] puts correspondence k at Z == 0
    and does not count it; the NEGATED planted pose puts every point behind the camera on the same pixels and counts exactly what the
    planted pose counts -- the restated cv2 inlier test has no depth test (cv2.projectPoints has none either), and this pins that."""
    for iterations in pc.SCORE_ITERATIONS:
        c = pc.score_case(n, iterations)
        counts = score(c, c["hyp"]).cpu().numpy()
        np.testing.assert_array_equal(counts, c["counts"], err_msg=f"n = {n}, iterations = {iterations}")
        rows = c["rows"]
        if "nan" in rows:
            assert counts[rows["nan"]] == 0
        if "negated" in rows:
            assert counts[rows["negated"]] == c["planted_count"]
        if "z0" in rows:
            assert not c["masks"][rows["z0"], c["k"]] and counts[rows["z0"]] == c["masks"][rows["z0"]].sum()


# ---- best_kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", pc.BEST_ITERATIONS)
@pytest.mark.parametrize("n", pc.BEST_N)
def test_best_kernel_takes_the_first_maximum_and_lists_its_inliers(n, iterations):
    """Crafted counts: the first maximum wins wherever it sits in the per-thread strided scan and the 1024-wide tree (tied maxima
    hold poses with different inlier sets, so info[2] and the mask each show which was taken), and the mask and the ORDERED inlier
    list are those of that pose, across the 1024-thread passes of the compaction."""
    prob = pc.best_problem(n)
    for name in pc.best_placements(iterations):
        c = pc.best_case(n, iterations, name)
        mask, idx, info = select(prob, c["hyp"], c["counts"])
        first = int(np.argmax(c["counts"]))                              # numpy: the first maximum
        want = pc.inlier_masks(c["hyp"][first], prob["pts_3d"], prob["pts_2d"], prob["K"])[0]
        what = f"n = {n}, iterations = {iterations}, maxima {name}"
        np.testing.assert_array_equal(info, [1, want.sum(), first, c["counts"][first]], err_msg=what)
        np.testing.assert_array_equal(mask, want.astype(np.int32), err_msg=what)
        np.testing.assert_array_equal(idx[:info[1]], np.nonzero(want)[0], err_msg=what)
        assert first == c["argmax"] and np.array_equal(want, c["mask"])


@pytest.mark.parametrize("iterations", pc.BEST_ITERATIONS)
@pytest.mark.parametrize("kind", ["below5", "zeros"])
def test_best_kernel_refuses_counts_below_the_model_size(kind, iterations):
    prob = pc.best_problem(1025)
    counts = pc.failing_counts(iterations, kind)
    hyp = np.tile(prob["poses"]["A"], (iterations, 1))                    # a pose WITH inliers: they must not be reported
    mask, _, info = select(prob, hyp, counts)
    np.testing.assert_array_equal(info, [0, 0, -1, counts.max()])
    assert not mask.any()


# ---- hyp_kernel -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hyp_rows(n, seed):
    """The rows of the longest pnp_hypotheses call of a case, checked for determinism on the way -> numpy [256, 12]."""
    c = pc.hyp_case(n, seed)
    full = max(pc.HYP_ITERATIONS)
    hyp = hypotheses(c, full, seed)
    assert torch.equal(hyp.view(torch.int64), hypotheses(c, full, seed).view(torch.int64))            # deterministic, bit for bit
    for iterations in pc.HYP_ITERATIONS[:-1]:                                                          # a row depends on (seed, h) alone
        assert torch.equal(hypotheses(c, iterations, seed).view(torch.int64), hyp[:iterations].view(torch.int64)), iterations
    return hyp.cpu().numpy()


@pytest.mark.parametrize("seed", pc.HYP_SEEDS)
@pytest.mark.parametrize("n", pc.HYP_N)
def test_hyp_kernel_draws_the_oracles_samples_and_fits_them(n, seed):
    """Noise-free data: the pose of hypothesis h explains exactly the planted inliers if and only if the ORACLE's minimal set
    (oracle/ransac_common.py, the same integers as sampling::distinct) lies wholly in them -- a wrong draw for some h breaks one
    side or the other.  The per-hypothesis poses are NOT compared with the oracle's: a 5-point sample leaves M^T M a two-dimensional
    null space whose basis is the implementation's (Jacobi here, LAPACK there), the betas depend on it, and no honest tolerance
    exists for a sample with an outlier in it.  Every row is twelve NaNs or all finite with det R > 0; two calls, and a shorter
    call against the first rows of the longest, are bitwise equal."""
    c = pc.hyp_case(n, seed)
    rows = hyp_rows(n, seed)
    nan = np.isnan(rows)
    assert np.array_equal(nan.any(axis=1), nan.all(axis=1)) and np.isfinite(rows[~nan.any(axis=1)]).all()
    R = rows[~nan.any(axis=1)].reshape(-1, 3, 4)[:, :, :3]
    assert (np.linalg.det(R) > 0).all()
    masks = pc.inlier_masks(rows, c["pts_3d"], c["pts_2d"], c["K"])
    n_in = int(c["planted"].sum())
    np.testing.assert_array_equal(masks.sum(axis=1) == n_in, c["clean"])
    np.testing.assert_array_equal(masks[c["clean"]], np.broadcast_to(c["planted"], masks[c["clean"]].shape))


@pytest.mark.parametrize("seed", pc.HYP_SEEDS)
@pytest.mark.parametrize("n", pc.HYP_N)
def test_hyp_kernel_rotations_are_orthonormal(n, seed):
    """R R^T = I to 1e-12 for EVERY finite row (the bound of test_hip_epnp_vs_oracle_and_drop_in_signature), the rows of samples
    with an outlier in them included: such a sample makes the absolute-orientation matrix M ill-conditioned, and U = M V / sigma
    taken column by column is then orthogonal only to about eps (sigma_0 / sigma_k)^2.  Before procrustes_rotation rebuilt such a
    frame the rows of contaminated samples were off by 6e-11 .. 2.4e-7 for n >= 7 (clean samples: 2e-14); with it, 1e-13 at most."""
    rows = hyp_rows(n, seed)
    R = rows[~np.isnan(rows).any(axis=1)].reshape(-1, 3, 4)[:, :, :3]
    print(f"n = {n}, seed = {seed}: {len(R)} finite rows, max |R R^T - I| = {np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max():.3e}")
    np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.broadcast_to(np.eye(3), R.shape), rtol=0, atol=1e-12)


# ---- the whole solve --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.CHAIN_CASES))
def test_the_solve_is_its_stages(name):
    """pnp_ransac_epnp against pnp_hypotheses -> pnp_score_hypotheses -> pnp_select_best at the default 10000 iterations: mask and
    info bitwise, and the solve's pose against pnp_epnp over the listed correspondences (gathered with torch indexing) bitwise --
    refit_kernel's index-list path against its plain path: each lane sees the same points in the same order."""
    c = pc.chain_case(name)
    p2, p3 = gpu(c["pts_2d"]), gpu(c["pts_3d"])
    pose, mask, info = pnp.ransac_pnp_device(c["K"], p2, p3, scale=pc.SCALE, reproj_error=pc.THR, iterations=pc.CHAIN_ITERATIONS, seed=pc.CHAIN_SEED)
    hyp = hypotheses(c, pc.CHAIN_ITERATIONS, pc.CHAIN_SEED)
    counts = score(c, hyp)
    mask_s, idx_s, info_s = select(c, hyp, counts)
    info = info.cpu().numpy()
    counts = counts.cpu().numpy()
    assert info[0] == 1 and info[1] >= 5
    np.testing.assert_array_equal(info_s, info)
    np.testing.assert_array_equal(mask_s, mask.cpu().numpy())
    assert info_s[2] == int(np.argmax(counts)) and info_s[3] == counts.max()                          # numpy: the first maximum of 10000
    listed = idx_s[:info_s[1]]
    np.testing.assert_array_equal(listed, np.nonzero(mask_s)[0])
    sel = gpu(listed.astype(np.int64))
    refit = pnp.epnp(c["K"], p2[sel], p3[sel], scale=pc.SCALE)
    assert torch.equal(refit.view(torch.int64), pose.view(torch.int64))
