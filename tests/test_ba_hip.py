"""The HIP bundle adjustment stage by stage and as a whole against tests/ba_oracle.py, on the smallest shapes at which each kernel
can still go wrong (tests/ba_cases.py).  Tolerances come from the reference-run golden, from the fp64 noise of each problem (the
spread between the oracle's two summation orders) and from the backward error of the oracle's own solve -- never from the HIP
result.  Measured figures are printed (pytest -s) and recorded in DESIGN section 17."""
import os

import numpy as np
import pytest
import torch

import ba_cases as bc
import ba_oracle as bo

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_residual_golden.npz")


@pytest.fixture(scope="module")
def ba():
    from onepose_amd import BundleAdjuster
    return BundleAdjuster()


def gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def problem_gpu(pb):
    return [gpu(a) for a in pb.args()]


def solve(ba, pb, **kw):
    return host(*ba.solve(*problem_gpu(pb), cam_fixed=gpu(pb.cam_fixed), pt_fixed=gpu(pb.pt_fixed), **kw))


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- linearise ---------------------------------------------------------------------------------------------------------------

def test_linearize_matches_the_reference_golden(ba):
    g = np.load(GOLDEN)
    intr, obs_cam, obs_pt, xy = bc.golden_problem(g["features"])
    parts = []
    for k in range(0, len(obs_cam), 30):        # one camera per observation: BA_MAX_CAMERAS allows 32 at a time
        s = slice(k, k + 30)
        parts.append(host(*ba.linearize(gpu(g["cams"][s]), gpu(intr[s]), gpu(g["points"][s]), gpu(obs_cam[s] - k), gpu(obs_pt[s] - k), gpu(xy[s]))))
    r, Jc, Jp = (np.concatenate(x) for x in zip(*parts))
    pred = g["residual"] + xy
    ulps, gap = bc.residual_ulps(r, g["residual"], pred), bc.jacobian_gap(Jc, Jp, g["Jc"], g["Jp"])
    print(f"ba_linearize vs the reference: {ulps:.2f} ulp of the predicted pixel, Jacobian gap {gap:.3e} (bound {bc.JACOBIAN_BOUND:.3e})")
    assert ulps <= bc.RESIDUAL_ULPS and gap <= bc.JACOBIAN_BOUND


def test_linearize_zeroes_an_observation_out_of_range(ba):
    pb = bc.tiny_case()
    obs_cam, obs_pt = np.array([0, 2, 1, -1], dtype=np.int32), np.array([0, 0, 1, 0], dtype=np.int32)
    xy = np.concatenate([pb.obs_xy, pb.obs_xy])
    r, Jc, Jp = host(*ba.linearize(gpu(pb.cams), gpu(pb.intr), gpu(pb.points), gpu(obs_cam), gpu(obs_pt), gpu(xy)))
    ro, Jco, Jpo, _ = bo.linearize(pb.cams, pb.intr, pb.points, obs_cam[:1], obs_pt[:1], xy[:1])
    assert np.all(r[1:] == 0) and np.all(Jc[1:] == 0) and np.all(Jp[1:] == 0)
    assert np.allclose(r[0], ro[0], rtol=1e-12) and bc.jacobian_gap(Jc[:1], Jp[:1], Jco, Jpo) <= bc.JACOBIAN_BOUND


# ---- normal blocks -----------------------------------------------------------------------------------------------------------

def hip_blocks(ba, pb):
    r, Jc, Jp = pb.linearized()
    out = ba.normal_blocks(gpu(r), gpu(Jc), gpu(Jp), gpu(pb.obs_cam), gpu(pb.obs_pt), pb.C, pb.P, gpu(pb.cam_fixed), gpu(pb.pt_fixed))
    return host(*out)


@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("cam0_count", [149, bc.CAMERA_CHUNK - 1, bc.CAMERA_CHUNK, bc.CAMERA_CHUNK + 1])
def test_normal_blocks(ba, cam0_count, permute):
    base = bc.blocks_case(cam0_count)
    other, _ = base.permuted()
    pb, pb_perm = (other, base) if permute else (base, other)
    ref, ref_perm = pb.blocks(), pb_perm.blocks()
    U, V, g_c, g_p, cost_cam = hip_blocks(ba, pb)
    worst = 0.0
    for name, x, a, b in (("U", U, ref[0], ref_perm[0]), ("V", V, ref[1], ref_perm[1]), ("g_c", g_c, ref[2], ref_perm[2]),
                          ("g_p", g_p, ref[3], ref_perm[3]), ("cost", [cost_cam.sum()], [ref[4]], [ref_perm[4]])):
        dist, bound = bc.block_rule(x, a, b)
        ratio = float(np.max(np.where(bound > 0, dist / np.where(bound > 0, bound, 1.0), 0.0)))
        worst = max(worst, ratio)
        assert np.all(dist <= bound), (name, ratio)
    print(f"normal blocks, camera 0 with {cam0_count} observations, permuted={permute}: worst distance / bound {worst:.3f}")
    assert np.all(U[2] == 0) and np.all(g_c[2] == 0) and np.all(V[0] == 0) and np.all(g_p[0] == 0) and cost_cam[2] == 0
    assert np.array_equal(U, np.swapaxes(U, 1, 2)) and np.array_equal(V, np.swapaxes(V, 1, 2))


def test_normal_blocks_zero_a_fixed_variable(ba):
    base = bc.blocks_case()
    cam_fixed, pt_fixed = np.array([0, 1, 0], dtype=np.int32), np.zeros(base.P, dtype=np.int32)
    pt_fixed[3] = 1
    pb = bc.Problem(*base.args(), cam_fixed=cam_fixed, pt_fixed=pt_fixed)
    U, V, g_c, g_p, cost_cam = hip_blocks(ba, pb)
    U0, V0, g_c0, g_p0, cost0 = hip_blocks(ba, base)
    assert np.all(U[1] == 0) and np.all(g_c[1] == 0) and np.all(V[3] == 0) and np.all(g_p[3] == 0)
    assert np.array_equal(U[0], U0[0]) and np.array_equal(np.delete(V, 3, axis=0), np.delete(V0, 3, axis=0)) and np.array_equal(cost_cam, cost0)


# ---- step --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mu", [1e4, 1.0, 1e-2])
@pytest.mark.parametrize("case", ["blocks", "tiny"])
def test_step_backward_error(ba, case, mu):
    pb = bc.blocks_case() if case == "blocks" else bc.tiny_case()
    A, g, bound, eta_oracle = bc.step_eta_bound(pb, mu)
    r, Jc, Jp = pb.linearized()
    U, V, g_c, g_p, _ = pb.blocks()
    dc, dp, md = host(*ba.step(gpu(U), gpu(V), gpu(g_c), gpu(g_p), gpu(r), gpu(Jc), gpu(Jp), gpu(pb.obs_cam), gpu(pb.obs_pt), mu))
    eta = bo.backward_error(A, g, np.concatenate([dc.reshape(-1), dp.reshape(-1)]))
    print(f"ba_step {case} mu={mu:g}: eta {eta:.3e} (oracle's Schur path {eta_oracle:.3e}, bound {bound:.3e})")
    assert eta <= bound
    cam_act, pt_act = pb.active()
    assert np.all(dc[~cam_act] == 0) and np.all(dp[~pt_act] == 0)
    # the same delta summed in two orders: M <= 150 terms of one sign up to a factor of about 3, so M * 3 * 2^-53 = 5e-14 << 1e-12
    md_oracle = bo.model_decrease(r, Jc, Jp, pb.obs_cam, pb.obs_pt, dc, dp)
    assert md[0] > 0 and abs(md[0] - md_oracle) <= 1e-12 * abs(md_oracle)


def test_step_leaves_fixed_variables_at_zero(ba):
    base = bc.blocks_case()
    cam_fixed, pt_fixed = np.array([0, 1, 0], dtype=np.int32), np.zeros(base.P, dtype=np.int32)
    pt_fixed[[3, 10]] = 1
    pb = bc.Problem(*base.args(), cam_fixed=cam_fixed, pt_fixed=pt_fixed)
    A, g, bound, _ = bc.step_eta_bound(pb, 1.0)
    r, Jc, Jp = pb.linearized()
    U, V, g_c, g_p, _ = pb.blocks()
    dc, dp, _ = host(*ba.step(gpu(U), gpu(V), gpu(g_c), gpu(g_p), gpu(r), gpu(Jc), gpu(Jp), gpu(pb.obs_cam), gpu(pb.obs_pt), 1.0,
                              gpu(cam_fixed), gpu(pt_fixed)))
    assert np.all(dc[1:] == 0) and np.all(dp[[0, 3, 10]] == 0) and np.any(dc[0] != 0)
    assert bo.backward_error(A, g, np.concatenate([dc.reshape(-1), dp.reshape(-1)])) <= bound


# ---- the whole solve ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [3, 6])
def test_solve_recovers_the_planted_problem(ba, C):
    pb, cams, points, seen2, oracle = bc.planted_case(C)
    cams_h, points_h, trace, summary = solve(ba, pb, num_iterations=30, num_success_iterations=30)
    err_c, err_p = np.abs(cams_h - cams).max(), np.abs(points_h[seen2] - points[seen2]).max()
    print(f"planted C={C}: cameras within {err_c:.2e}, points within {err_p:.2e}, final cost {summary[1]:.2e} after {int(summary[2])} accepted steps")
    assert err_c <= 1e-9 and err_p <= 1e-9
    assert summary[5] == 0 and summary[4] == 0 and summary[0] == trace[0, 0]
    assert np.array_equal(bits(cams_h[:2]), bits(pb.cams[:2]))


@pytest.mark.parametrize("kind", ["plain", "rejecting", "zero_rotation"])
def test_solve_as_the_reference_calls_it(ba, kind):
    pb, oracle, oracle_perm, _ = bc.reference_case(kind)
    cams_h, points_h, trace, summary = solve(ba, pb)
    assert np.array_equal(trace[:, 5], oracle[2][:, 5]), (trace[:, 5], oracle[2][:, 5])
    worst = 0.0
    for it in range(5):
        for col in (0, 1):
            dist, bound = bc.spread_rule(trace[it, col], oracle[2][it, col], oracle_perm[2][it, col], 1e-12)
            worst = max(worst, dist / bound)
            assert dist <= bound, (it, col, dist, bound)
    px = [bo.reproject(c, pb.intr, p, pb.obs_cam, pb.obs_pt) for c, p in ((cams_h, points_h), oracle[:2], oracle_perm[:2])]
    dist, bound = bc.spread_rule(*px, 1e-12)
    print(f"{kind}: costs at most {worst:.3f} of their bound, final pixels {dist:.2e} (bound {bound:.2e})")
    assert dist <= bound
    assert summary[2] == oracle[3][2] and summary[3] == 5 and summary[5] == 0
    dist, bound = bc.spread_rule(summary[1], oracle[3][1], oracle_perm[3][1], 1e-12)
    assert dist <= bound and summary[0] == trace[0, 0]


# ---- contract ----------------------------------------------------------------------------------------------------------------

def test_two_runs_are_bitwise_equal(ba):
    pb = bc.reference_case("rejecting")[0]
    a, b = solve(ba, pb), solve(ba, pb)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))


def test_fixed_and_unobserved_variables_come_back_bitwise(ba):
    base = bc.planted_case(3)[0]
    cams = np.concatenate([base.cams, [[0.1, -0.2, 0.3, 0.0, 0.0, 0.6]]])             # camera 3: no observation
    intr = np.concatenate([base.intr, base.intr[:1]])
    points = np.concatenate([base.points, [[-0.0, 1e-300, 7.0]]])                      # point 60: no observation
    cam_fixed, pt_fixed = np.array([1, 1, 0, 0], dtype=np.int32), np.zeros(61, dtype=np.int32)
    pt_fixed[[5, 17]] = 1
    pb = bc.Problem(cams, intr, points, base.obs_cam, base.obs_pt, base.obs_xy, cam_fixed, pt_fixed)
    cams_h, points_h, trace, summary = solve(ba, pb, num_iterations=6, num_success_iterations=6)
    assert summary[2] >= 3 and summary[1] < 0.1 * summary[0]       # the two fixed points stay 3 mm off: the cost cannot vanish
    assert np.array_equal(bits(cams_h[[0, 1, 3]]), bits(cams[[0, 1, 3]])) and np.array_equal(bits(points_h[[5, 17, 60]]), bits(points[[5, 17, 60]]))
    assert np.all(cams_h[2] != cams[2]) and np.all(points_h[6] != points[6])


@pytest.mark.parametrize("shape", ["32 cameras", "points past 4095"])
def test_limits_and_the_third_radix_pass(ba, shape):
    if shape == "32 cameras":
        pb, oracle = bc.wide_case(32, 48, tuple(range(48)), 51)
    else:
        pb, oracle = bc.wide_case(3, 4100, tuple(range(0, 4100, 100)) + (4095, 4096, 4099), 52)
    cams_h, points_h, trace, summary = solve(ba, pb, num_iterations=3, num_success_iterations=3)
    assert np.array_equal(trace[:, 5], oracle[2][:, 5])
    # gauge fixed: the iterates are determined, and 1e-9 is the bound of the planted problems (fp64 noise times a condition of 1e6)
    assert np.allclose(trace[:, :2], oracle[2][:, :2], rtol=1e-9, atol=0)
    assert np.allclose(cams_h, oracle[0], rtol=0, atol=1e-9) and np.allclose(points_h, oracle[1], rtol=0, atol=1e-9)
    unobserved = np.bincount(pb.obs_pt, minlength=pb.P) == 0
    assert np.array_equal(bits(points_h[unobserved]), bits(pb.points[unobserved]))


def test_out_of_range_observations_are_counted_and_ignored(ba):
    pb = bc.reference_case("plain")[0]
    bad_cam = np.array([-1, pb.C, 0, 2, 1 << 30, -(1 << 31)], dtype=np.int32)
    bad_pt = np.array([0, 3, pb.P, -5, 1, 2], dtype=np.int32)
    where = np.array([0, 7, 7, 100, pb.M, pb.M])
    dirty = bc.Problem(pb.cams, pb.intr, pb.points, np.insert(pb.obs_cam, where, bad_cam), np.insert(pb.obs_pt, where, bad_pt),
                       np.insert(pb.obs_xy, where, 1e9, axis=0))
    clean_out, dirty_out = solve(ba, pb), solve(ba, dirty)
    assert dirty_out[3][4] == 6 and clean_out[3][4] == 0
    for x, y in zip(clean_out[:3], dirty_out[:3]):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(np.delete(clean_out[3], 4), np.delete(dirty_out[3], 4))


def test_success_count_stops_the_solve(ba):
    pb = bc.planted_case(3)[0]
    cams_a, points_a, trace_a, summary_a = solve(ba, pb, num_iterations=6, num_success_iterations=2)
    cams_b, points_b, trace_b, summary_b = solve(ba, pb, num_iterations=2, num_success_iterations=2)
    assert summary_a[2] == 2 and summary_a[3] == 2 and np.all(trace_a[:2, 5] == 1)
    assert np.all(trace_a[2:, 5] == -1) and np.all(trace_a[2:, :5] == 0)
    assert np.array_equal(bits(cams_a), bits(cams_b)) and np.array_equal(bits(points_a), bits(points_b))
    assert np.array_equal(bits(trace_a[:2]), bits(trace_b)) and np.array_equal(bits(summary_a), bits(summary_b))


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_non_finite_start_returns_its_inputs(ba, poison):
    base = bc.planted_case(3)[0]
    points = base.points.copy()
    points[7, 1] = poison
    pb = bc.Problem(base.cams, base.intr, points, base.obs_cam, base.obs_pt, base.obs_xy, base.cam_fixed)
    cams_h, points_h, trace, summary = solve(ba, pb)
    assert summary[5] == bo.STATUS_NONFINITE_START and summary[2] == 0 and summary[3] == 0 and not np.isfinite(summary[0])
    assert np.array_equal(bits(cams_h), bits(pb.cams)) and np.array_equal(bits(points_h), bits(points))
    assert np.all(trace[:, 5] == -1)
