"""Every generated case of the EPnP geometry tests (tests/test_pnp_geometry.py) meets the conditions of tests/pnp_geometry_cases.py, and
the oracle's flatness guard does what include/pnp.h says of the kernel's.  No GPU needed."""
import math

import numpy as np
import pytest

import pnp_geometry_cases as gc
from oracle import pnp_oracle as po


def test_e_max_is_two_to_the_minus_ten_inside_the_image():
    assert gc.e_max(np.array([[3.0, 511.9]], np.float32)) == 2.0 ** -10 == gc.e_max(np.array([[-400.0, 20.0]], np.float32))
    assert gc.e_max(np.array([[1023.0, 20.0]], np.float32)) == 2.0 ** -10 and gc.e_max(np.array([[0.0, -1025.0]], np.float32)) == 2.0 ** -9


@pytest.mark.parametrize("view", list(gc.VIEWS))
def test_benign_cases_meet_the_conditions(view):
    """(a) ratio, (b) the oracle's reprojection, (c) spread, (d) clearance from the guard, for the cases of both EPnP paths."""
    cases = gc.benign_cases(view) + gc.benign_cases(view, (gc.N_THREAD,))
    assert {obj for obj, _, _ in cases} == set(gc.BENIGN_OBJECTS) and {n for _, n, _ in cases} == {5, 6, 8, 14, 40, 65}
    assert {obj for obj, n, _ in cases if n == 5} == {obj for obj in gc.BENIGN_OBJECTS if not gc.not_at_five(obj, view)}
    assert [obj for obj in gc.BENIGN_OBJECTS if gc.not_at_five(obj, view)] == (["dup", "rod_tilt"] if view == "far20m" else ["dup"])
    for obj, n, c in cases:
        what = f"{obj} / {view} / n = {n}"
        assert len(c["pts_3d"]) == n and c["pts_3d"].dtype == c["pts_2d"].dtype == np.float32, what
        assert c["ratio"] >= gc.RATIO_MIN and c["ratio"] >= gc.GUARD_CLEARANCE * po.FLATNESS_TAU, what               # (a), (d)
        assert c["oracle_err"] <= c["e_max"] / 4, what                                                             # (b)
        assert gc.worst_reprojection(c["pose_gt"], c) <= math.sqrt(2) * c["e_max"] / 32, what      # the planted pose: half an ulp per coordinate
        if n == gc.N_THREAD:
            continue
        if c["pose_to_pose"]:
            assert 64 * c["spread"][0] <= gc.R_FLOOR and 64 * c["spread"][1] <= gc.T_FLOOR, what                   # (c)
            assert (c["tie_spread"] != (0.0, 0.0)) == (obj in ("cube", "prism")), what                              # tied eigenvalues
            assert c["tol"] == (max(gc.R_FLOOR, 64 * c["tie_spread"][0]), max(gc.T_FLOOR, 64 * c["tie_spread"][1])), what
        else:
            assert gc.REPROJECTION_ONLY_ALLOWED(obj, view), what
    if view in ("near", "corner"):
        assert any(np.abs(c["pts_2d"]).max() > 512 or c["pts_2d"].min() < 0 for _, _, c in cases)      # pixels outside the image
    if view == "far20m":
        assert all(abs(c["pose_gt"][2, 3] + c["pose_gt"][2, :3] @ gc.OBJECTS[obj][1] - 20.0) < 1e-9 for obj, _, c in cases)


def test_only_rods_and_the_far_view_are_compared_by_reprojection_alone():
    loose = [(obj, view, n) for view in gc.VIEWS for obj, n, c in gc.benign_cases(view) if not c["pose_to_pose"]]
    assert loose and all(gc.REPROJECTION_ONLY_ALLOWED(obj, view) for obj, view, _ in loose)
    tight = [(obj, view) for view in gc.VIEWS for obj, n, c in gc.benign_cases(view) if c["pose_to_pose"]]
    assert {obj for obj, _ in tight} >= set(gc.BENIGN_OBJECTS) - set(gc.RODS) and {view for _, view in tight} >= set(gc.VIEWS) - {"far20m"}


def test_the_guard_changes_no_bit_of_the_oracle_where_it_does_not_fire(monkeypatch):
    guarded = [(c, gc.oracle_pose(c)) for view in ("generic", "identity", "far20m") for _, _, c in gc.benign_cases(view)]
    monkeypatch.setattr(po, "FLATNESS_TAU", -math.inf)
    for c, pose in guarded:
        assert np.array_equal(gc.oracle_pose(c), pose) and np.array_equal(pose, c["oracle"])


def test_flat_sets_get_no_pose_from_the_oracle_and_never_an_exception():
    for name, view, n, c in gc.degenerate_cases():
        what = f"{name} / {view} / n = {n}"
        assert len(c["pts_3d"]) == n and c["ratio"] <= po.FLATNESS_TAU / gc.GUARD_CLEARANCE, what
        r, t = po.epnp(c["pts_3d"].astype(np.float64) * gc.SCALE, c["pts_2d"].astype(np.float64), c["K"])
        assert np.isnan(r).all() and np.isnan(t).all(), what
        ok, r, t, inl = po.solve_pnp_ransac(c["pts_3d"].astype(np.float64) * gc.SCALE, c["pts_2d"], c["K"], 5.0, 32, 3)
        assert not ok and np.array_equal(r, np.eye(3)) and not t.any() and len(inl) == 0, what
    assert {(name, n) for name, _, n, _ in gc.degenerate_cases()} == {(name, n) for name, (_, full) in gc.DEGENERATE.items() for n in (full, 5)}
    pose, homo, inl = po.ransac_pnp(c["K"], c["pts_2d"], c["pts_3d"], scale=1000, iterations=16)
    assert np.array_equal(pose, np.eye(4)[:3]) and inl == []


def test_thin_band_cases_are_clear_of_the_guard_and_the_oracle_keeps_a_pose_or_nothing():
    cases = gc.band_cases()
    assert {obj for obj, _, _, _ in cases} == set(gc.BAND_OBJECTS) and len(gc.BAND_OBJECTS) == 14
    for obj, view, n, c in cases:
        what = f"{obj} / {view} / n = {n}"
        assert gc.clear_of_guard(c["ratio"]), what                                                                 # (d)
        pose = gc.oracle_pose(c)
        assert np.isnan(pose).all() or (np.isfinite(pose).all() and gc.worst_reprojection(pose, c) <= c["e_max"]), what
        assert np.isnan(pose).all() == (c["ratio"] <= po.FLATNESS_TAU), what


def test_the_two_face_object_has_both_kinds_of_sample():
    c = gc.two_faces_case()
    assert c["flat"].any() and (~c["flat"]).any() and 0.02 < c["flat"].mean() < 0.12            # about 6 % lie wholly in one face
    assert (c["face"] == 0).sum() == (c["face"] == 1).sum() == 20
    assert (c["pts_3d"][c["face"] == 0, 2] == 0).all() and (c["pts_3d"][c["face"] == 1, 0] == 0).all()
    assert c["ratio"] > 1e-2 and c["worst_sample_err2"] < 1.0 and c["tol"] == (gc.R_FLOOR, gc.T_FLOOR)
    ok, r, t, inl = po.solve_pnp_ransac(c["pts_3d"].astype(np.float64) * gc.SCALE, c["pts_2d"], c["K"], 5.0, gc.TWO_FACES_ITERATIONS, c["seed"])
    assert ok and len(inl) == 40 and np.array_equal(np.concatenate([r, (t / gc.SCALE)[:, None]], axis=1), c["oracle"])


def test_the_refit_refusal_case_lists_coplanar_inliers():
    c = gc.refit_refusal_case()
    assert np.array_equal(c["inliers"], np.arange(0, 40, 2)) and (c["pts_3d"][c["inliers"], 2] == 0).all()
    assert c["e2"][0::2].max() < 1e-6 and c["e2"][1::2].min() > 100.0                        # px^2: nothing near the 25 px^2 threshold
    assert int(np.argmax(c["counts"])) == c["best"] and c["counts"].max() == 20
    assert gc.eigen_ratio(c["pts_3d"]) > 1e-2 and gc.eigen_ratio(c["pts_3d"][c["inliers"]]) == 0.0
