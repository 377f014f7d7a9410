"""The numpy oracle of the bundle adjustment against the reference's own residual function (tests/golden/ba_residual_golden.npz:
SnavelyReprojectionErrorV2 and its autograd Jacobians, run on the CPU by tests/golden/make_ba_golden.py), its Schur path against
its independent dense path, and its LM loop on the planted problems."""
import os

import numpy as np
import pytest

import ba_cases as bc
import ba_oracle as bo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_residual_golden.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    cams, points, feats = bc.golden_inputs()
    assert np.array_equal(cams, g["cams"]) and np.array_equal(points, g["points"]) and np.array_equal(feats, g["features"])
    return g


def test_golden_covers_the_rotation_angles(golden):
    theta = np.linalg.norm(golden["cams"][:, :3], axis=1)
    n = bc.GOLDEN_PER_ANGLE
    assert len(theta) == n * len(bc.GOLDEN_ANGLES) >= 200
    assert np.all(theta[:n] == 0.0)
    assert np.allclose(theta[n:2 * n], 1e-8, rtol=1e-12) and np.allclose(theta[2 * n:3 * n], 1e-3, rtol=1e-12)
    assert np.all(np.abs(theta[3 * n:4 * n] - 1.0) <= 0.2) and np.allclose(theta[4 * n:], np.pi - 1e-3, rtol=1e-12)
    assert np.isfinite(golden["residual"]).all() and np.isfinite(golden["Jc"]).all() and np.isfinite(golden["Jp"]).all()


def test_residual_and_jacobian_match_the_reference(golden):
    intr, obs_cam, obs_pt, xy = bc.golden_problem(golden["features"])
    r, Jc, Jp, pred = bo.linearize(golden["cams"], intr, golden["points"], obs_cam, obs_pt, xy)
    ulps = bc.residual_ulps(r, golden["residual"], pred)
    gap = bc.jacobian_gap(Jc, Jp, golden["Jc"], golden["Jp"])
    print(f"residual: {ulps:.2f} ulp of the predicted pixel; Jacobian gap {gap:.3e} (recorded {bc.JACOBIAN_GAP_MEASURED:.3e}, bound {bc.JACOBIAN_BOUND:.3e})")
    assert ulps <= bc.RESIDUAL_ULPS
    assert gap <= bc.JACOBIAN_BOUND
    assert bc.JACOBIAN_BOUND == max(16 * bc.JACOBIAN_GAP_MEASURED, 2.0 ** -40)


def test_first_order_branch_is_the_function_at_zero_rotation():
    cams = np.array([[0.0, 0.0, 0.0, 0.01, -0.02, 0.8]])
    pts = np.array([[0.03, -0.05, 0.07]])
    r, Jc, Jp, _ = bo.linearize(cams, np.array([[500.0, 500.0, 320.0, 240.0]]), pts, np.array([0]), np.array([0]), np.zeros((1, 2)))
    X, Y, Z = pts[0] + cams[0, 3:]
    A = np.array([[500.0 / Z, 0, -500.0 * X / Z ** 2], [0, 500.0 / Z, -500.0 * Y / Z ** 2]])
    px, py, pz = pts[0]
    minus_skew = np.array([[0, pz, -py], [-pz, 0, px], [py, -px, 0]])       # d (w x p) / d w
    assert np.allclose(Jc[0, :, :3], A @ minus_skew, rtol=1e-14, atol=0) and np.allclose(Jp[0], A, rtol=1e-14, atol=0)


@pytest.mark.parametrize("mu", [1e4, 1.0, 1e-2])
@pytest.mark.parametrize("case", ["blocks", "tiny"])
def test_schur_path_agrees_with_the_dense_path(case, mu):
    pb = bc.blocks_case() if case == "blocks" else bc.tiny_case()
    A, g, U, V, g_c, g_p, W = pb.system(mu)
    act = pb.active()
    etas = {}
    for name, step in (("schur", bo.step_schur), ("dense", bo.step_dense)):
        dc, dp = step(U, V, g_c, g_p, W, mu, *act)
        etas[name] = bo.backward_error(A, g, np.concatenate([dc.reshape(-1), dp.reshape(-1)]))
        assert np.all(dc[~act[0]] == 0) and np.all(dp[~act[1]] == 0)
    print(f"{case} mu={mu:g}: eta schur {etas['schur']:.3e}, dense {etas['dense']:.3e}")
    assert etas["schur"] <= 16 * max(etas["dense"], len(g) * 2.0 ** -53)


@pytest.mark.parametrize("C", [3, 6])
def test_oracle_lm_recovers_the_planted_problem(C):
    pb, cams, points, seen2, (cams_o, points_o, trace, summary) = bc.planted_case(C)
    assert np.abs(cams_o - cams).max() <= 1e-10 and np.abs(points_o[seen2] - points[seen2]).max() <= 1e-10
    assert summary[1] <= 1e-20 and summary[5] == bo.STATUS_OK
    assert np.array_equal(cams_o[:2], pb.cams[:2])


def test_oracle_dense_lm_follows_the_schur_lm():
    pb, out, out_perm, _ = bc.reference_case("plain")
    dense = pb.lm(dense=True)
    assert np.array_equal(dense[2][:, 5], out[2][:, 5])
    assert np.allclose(dense[2][:, :2], out[2][:, :2], rtol=1e-9, atol=0)
