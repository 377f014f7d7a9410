"""The numpy oracle of the flow step (tests/flow_oracle.py) on its own: the pyramid against a direct double loop, planted shifts
recovered to the termination step, the status and exit-code rules, and the exactness conditions the GPU comparison
(tests/test_flow_hip.py) rests on -- no decision of any case sits on its threshold.  No GPU."""
import numpy as np
import pytest

import flow_cases as fc
import flow_oracle as fo
from onepose_amd._native_det import FLOW_EXIT, FLOW_REPROJ_THREADS


def test_the_oracle_speaks_the_bindings_exit_codes():
    assert FLOW_EXIT == {"converged": fo.EXIT_CONVERGED, "oscillation": fo.EXIT_OSCILLATION, "iteration_cap": fo.EXIT_ITERATION_CAP,
                         "left_range": fo.EXIT_LEFT_RANGE, "rejected": fo.EXIT_REJECTED, "skipped": fo.EXIT_SKIPPED}
    assert FLOW_REPROJ_THREADS == fo.REPROJ_LANES


def pyr_down_loops(img):
    """The definition, pixel by pixel."""
    H, W = img.shape
    k = [1, 4, 6, 4, 1]
    ref = lambda v, n: 0 if n == 1 else (lambda m: 2 * (n - 1) - m if m >= n else m)(v % (2 * (n - 1)))  # noqa: E731
    out = np.zeros(((H + 1) // 2, (W + 1) // 2), np.uint8)
    for y in range(out.shape[0]):
        for x in range(out.shape[1]):
            acc = 0
            for j in range(5):
                for i in range(5):
                    acc += k[i] * k[j] * int(img[ref(2 * y + j - 2, H), ref(2 * x + i - 2, W)])
            out[y, x] = (acc + 128) >> 8
    return out


@pytest.mark.parametrize("H,W", [(16, 20), (17, 20), (16, 21), (9, 7), (2, 2), (3, 2), (1, 5)])
def test_pyr_down_is_the_definition(H, W):
    img = np.random.RandomState(H * 100 + W).randint(0, 256, (H, W)).astype(np.uint8)
    got = fo.pyr_down(img)
    assert got.dtype == np.uint8 and got.shape == ((H + 1) // 2, (W + 1) // 2)
    assert np.array_equal(got, pyr_down_loops(img))
    if W > 3:
        assert fo.reflect101(np.array([-1, -2, W, W + 1]), W).tolist() == [1, 2, W - 2, W - 3]


@pytest.mark.parametrize("case", fc.planted_cases(), ids=lambda c: c.name)
def test_planted_integer_shifts_are_recovered_to_the_termination_step(case):
    nxt, status, matches0, trace, _ = case.result
    assert case.levels == 3 and len(case.pts) == 40
    H, W = case.first.shape
    assert (case.pts.min(axis=0) >= 20).all() and (case.pts[:, 0] <= W - 21).all() and (case.pts[:, 1] <= H - 21).all()
    assert (status == 1).all() and np.array_equal(matches0, np.arange(40))
    err = np.linalg.norm(nxt.astype(np.float64) - (case.pts.astype(np.float64) + np.array(case.planted)), axis=1)
    print(f"{case.name}: worst error {err.max():.4f} px, level-0 iterations <= {trace[:, 0, 0].max()}")
    assert err.max() <= 0.03


def test_a_constant_image_is_rejected_before_iterating():
    _, status, matches0, trace, _ = fc.constant_case().result
    assert (status == 0).all() and (matches0 == -1).all()
    assert (trace[:, :, 0] == 0).all() and (trace[:, :, 1] == fo.EXIT_REJECTED).all()


def test_levels_stop_where_a_level_is_not_larger_than_the_window():
    case = fc.short_pyramid_case()
    assert case.max_level == 3 and case.levels == 2 == fo.pyramid_levels(48, 64, (15, 15), 3)      # level 2 would be 12 x 16
    assert fo.pyramid_levels(512, 512, (15, 15), 2) == 3 and fo.pyramid_levels(512, 512, (15, 15), 5) == 6
    assert fo.pyramid_levels(64, 64, (15, 15), 5) == 3 and fo.pyramid_levels(64, 64, (15, 7), 0) == 1
    nxt, status, _, trace, _ = case.result
    assert trace.shape == (12, 2, 2) and (status == 1).all()
    assert np.abs(nxt - (case.pts + np.array(case.planted, np.float32))).max() <= 0.03


def test_border_points_track_and_a_far_point_is_skipped():
    case = fc.border_case()
    nxt, status, matches0, trace, _ = case.result
    assert status.tolist() == [1, 1, 1, 0] and matches0.tolist() == [0, 1, 2, -1]
    assert trace[3, 0].tolist() == [0, fo.EXIT_SKIPPED]
    assert np.abs(nxt[:3, 0] - (case.pts[:3, 0] + 1)).max() < 0.5       # the 1-px shift is followed along x


def test_the_noisy_case_exercises_every_path_the_gpu_comparison_needs():
    case = fc.noisy_case()
    nxt, status, _, trace, _ = case.result
    H, W = case.first.shape
    drawn = case.pts[:200]
    assert len(case.pts) == 202 and drawn[:, 0].min() >= -5 and drawn[:, 0].max() <= W + 5 and drawn[:, 1].min() >= -5 and drawn[:, 1].max() <= H + 5
    it0, code0 = trace[:, 0, 0], trace[:, 0, 1]
    hist = {int(k): int((it0 == k).sum()) for k in np.unique(it0)}
    print(f"noisy: {int(status.sum())} of {len(status)} tracked, level-0 iterations {hist}, codes {sorted(set(code0.tolist()))}")
    for k in (1, 2, 3, case.max_iter):
        assert hist.get(k, 0) > 0, k
    assert any(5 <= k < case.max_iter for k in hist)
    assert {fo.EXIT_CONVERGED, fo.EXIT_ITERATION_CAP, fo.EXIT_LEFT_RANGE, fo.EXIT_SKIPPED} <= set(code0.tolist())
    assert 150 <= int(status.sum()) < 200


def test_the_oscillation_exit_occurs_in_the_case_set():
    codes = set()
    for case in fc.all_cases():
        codes |= set(case.result[3][:, :, 1].ravel().tolist())
    assert codes == {fo.EXIT_CONVERGED, fo.EXIT_OSCILLATION, fo.EXIT_ITERATION_CAP, fo.EXIT_LEFT_RANGE, fo.EXIT_REJECTED, fo.EXIT_SKIPPED}


@pytest.mark.parametrize("case", fc.all_cases(), ids=lambda c: c.name)
def test_no_decision_of_any_case_sits_on_its_threshold(case):
    """Conditions on the inputs: with them, the last bit of an fp64 operation cannot turn a comparison."""
    margins = case.result[4]
    assert margins["min_eig"] > 1e-9 and margins["det"] > 1e-9 and margins["eps"] > 1e-9 and margins["oscillation"] > 1e-12, margins


def test_an_initial_guess_is_used_at_the_top_level():
    case = fc.guess_case()
    nxt, status, _, _, _ = case.result
    assert (status == 1).all() and np.abs(nxt - (case.pts + np.array(case.planted, np.float32))).max() <= 0.03
    far = fo.track(*case.pyramids, case.pts[:4], init=case.pts[:4] + np.float32(40.0))[0]     # a useless guess is not ignored
    assert not np.allclose(far, nxt[:4], atol=0.5)


def test_stage_functions_agree_with_the_tracker_and_refuse_out_of_range_windows():
    case = fc.planted_cases()[0]
    pi, pj = case.pyramids
    p = case.pts[0].astype(np.float64)
    (A11, A12, A22), ival, ix, iy = fo.patch_sums(pi, 0, p, case.win)
    assert ival.shape == (15, 15) and A11 == int((ix * ix).sum()) and A11 > 0 and A22 > 0 and A12 * A12 < A11 * A22
    assert 0 <= ival.min() and ival.max() <= 255 * 32 and np.abs(ix).max() <= 16 * 255
    assert fo.mismatch_sums(pi, pi, 0, p, p, case.win) == (0, 0)
    b = fo.mismatch_sums(pi, pj, 0, p, p + np.array(case.planted), case.win)
    assert abs(b[0]) * fo.SCALE < 1e-2 * A11 * fo.SCALE                  # at the planted position the mismatch is small
    assert fo.patch_sums(pi, 0, np.array([-9.0, 5.0]), case.win) is None and fo.patch_sums(pi, 0, np.array([-8.0, 5.0]), case.win) is not None
    assert fo.weights(0.0, 0.0) == (16384, 0, 0, 0) and fo.weights(0.5, 0.5) == (4096, 4096, 4096, 4096)
    assert sum(fo.weights(1 - 2.0 ** -20, 0.5)) == 16384


def test_reproj_mean_is_the_mean_distance_over_the_tracked_points():
    rs = np.random.RandomState(5)
    X = rs.uniform(-0.1, 0.1, (300, 3)).astype(np.float32)
    pose = np.concatenate([np.eye(3), [[0.01], [-0.02], [0.6]]], axis=1)
    K = np.array([[500.0, 0, 64], [0, 500.0, 64], [0, 0, 1]])
    c = X.astype(np.float64) @ pose[:, :3].T + pose[:, 3]
    h = c @ K.T
    x = (h[:, :2] / h[:, 2:] + rs.normal(0, 1.0, (300, 2))).astype(np.float32)
    status = (rs.uniform(size=300) < 0.8).astype(np.int32)
    mean, count = fo.reproj_mean(pose, K, X, x, status)
    direct = np.linalg.norm(h[:, :2] / h[:, 2:] - x, axis=1)[status == 1]
    assert count == int(status.sum()) and abs(mean - direct.mean()) < 1e-12
    assert np.isnan(fo.reproj_mean(pose, K, X, x, np.zeros(300, np.int32))[0])
