"""The numpy oracle of the map update step against what the reference's own functions give (tests/golden/track_golden.npz:
BATracker._triangulatePy, BATracker.cm_degree_5_metric and tracking_utils.project, run on the CPU) and on small hand cases.

Bounds come from the golden alone: the triangulated points are held within 16 x the distance between the reference's two
own answers (eigenvector of A^T A by scipy's SVD, and the right singular vector of A), floored at 2^-40; `project` within 4 ulp;
the metric within 1e-12.  Every discrete outcome of `update` is recomputed from the reference's points and numpy.median, and
the cases are checked to keep every decision clear of its threshold by 1e-9 relative, so the comparison is exact."""
import os

import numpy as np
import pytest

import track_cases as tc
import track_oracle as orc

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_golden.npz"))
FLOOR = 2.0 ** -40
CLEAR = 1e-9


def parts(c):
    i = np.where(c["matches0"] >= 0)[0]
    j = c["matches0"][i]
    ids = c["kf_pt_ids"][i]
    return i, j, ids, ids == -1, ids >= 0


@pytest.mark.parametrize("name", sorted(tc.GOLDEN))
def test_triangulation_against_the_reference(name):
    c = tc.golden_cases()[name]
    i, j, ids, cand, _ = parts(c)
    ref, svd = GOLDEN[name + "/X"], GOLDEN[name + "/X_svd"]
    X = orc.triangulate_pairs(orc.projection_matrix(c["K_kf"], c["pose_kf"]), orc.projection_matrix(c["K_q"], c["pose_q"]),
                              c["kf_xy"][i[cand]], c["q_xy"][j[cand]])
    rel = lambda a, b: np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)  # noqa: E731
    spread = rel(svd, ref)
    gap = rel(X, ref)
    bound = np.maximum(16 * spread.max(), FLOOR)
    print(f"{name}: {len(X)} points, reference spread max {spread.max():.3e}, oracle gap max {gap.max():.3e}, bound {bound:.3e}")
    assert X.shape == ref.shape and len(X) >= 100
    assert gap.max() <= bound


@pytest.mark.parametrize("name", sorted(tc.GOLDEN))
def test_project_within_4_ulp(name):
    c = tc.golden_cases()[name]
    _, _, ids, _, known = parts(c)
    for X, K, pose, key in ((GOLDEN[name + "/X"], c["K_q"], c["pose_q"], "/rep_q"), (GOLDEN[name + "/X"], c["K_kf"], c["pose_kf"], "/rep_kf"),
                            (c["points"][ids[known]], c["K_q"], c["pose_q"], "/known_rep_q")):
        got, ref = orc.project(X, K, pose), GOLDEN[name + key]
        ulp = np.abs(got - ref) / np.spacing(np.abs(ref))
        assert got.shape == ref.shape and ulp.max() <= 4, (key, ulp.max())


def test_metric_equals_the_reference():
    from onepose_amd.tracker import cm_degree_5_metric
    got = np.array([cm_degree_5_metric(p, t) for p, t in tc.METRIC_POSES])
    assert np.abs(got - GOLDEN["metric"]).max() <= 1e-12
    assert got[0, 0] == 0 and got[0, 1] == 0 and got[1, 0] > 1 and got[2, 1] > 10


def clear_of(value, threshold):
    return np.abs(value - threshold) > CLEAR * np.abs(threshold)


@pytest.mark.parametrize("name", sorted(tc.GOLDEN))
def test_discrete_outcomes_equal_the_reference_recomputation(name):
    c = tc.golden_cases()[name]
    i, j, ids, cand, known = parts(c)
    m = len(i)
    # from the reference's numbers alone
    d = np.linalg.norm(GOLDEN[name + "/known_rep_q"] - c["q_xy"][j[known]], axis=1)
    med = np.median(d) * tc.GATE
    X = GOLDEN[name + "/X"]
    rep_q = np.linalg.norm(GOLDEN[name + "/rep_q"] - c["q_xy"][j[cand]], axis=1)
    rep_kf = np.linalg.norm(GOLDEN[name + "/rep_kf"] - c["kf_xy"][i[cand]], axis=1)
    # the exactness condition, on the reference alone
    assert clear_of(d, med).all() and clear_of(rep_q, tc.MAX_REPROJ).all() and clear_of(rep_kf, tc.MAX_REPROJ).all()
    assert clear_of(X[:, 2], tc.MAX_Z).all() and np.isfinite(X).all()
    keep_known = d < med
    keep_cand = ~((rep_q > tc.MAX_REPROJ) | (rep_kf > tc.MAX_REPROJ) | (X[:, 2] > tc.MAX_Z))
    want = np.full(m, -1)
    want[np.where(known)[0][keep_known]] = ids[known][keep_known]
    want[np.where(cand)[0][keep_cand]] = len(c["points"]) + np.arange(keep_cand.sum())

    u = orc.update(**c)
    assert np.array_equal(u.pair_kf[:m], i) and np.array_equal(u.pair_q[:m], j) and (u.pair_kf[m:] == -1).all()
    assert np.array_equal(u.q_pt_ids[:m], want) and (u.q_pt_ids[m:] == -1).all()
    n_unmatched = c["q_xy"].shape[0] - len(set(j.tolist()))
    assert u.summary.tolist() == [m, known.sum(), keep_known.sum(), cand.sum(), keep_cand.sum(), 0, 0, n_unmatched]
    # a distance moves by at most the 4 ulp `project` may differ by on each pixel coordinate (below 512), times sqrt(2)
    assert abs(u.median[0] - med) <= tc.GATE * 8 * np.spacing(512.0)
    assert 0 < keep_known.sum() < known.sum()
    if tc.GOLDEN[name]["outliers"] > 0:
        assert keep_cand.sum() < cand.sum()
    rel = np.linalg.norm(u.new_points - X[keep_cand], axis=1) / np.linalg.norm(X[keep_cand], axis=1)
    spread = np.linalg.norm(GOLDEN[name + "/X_svd"] - X, axis=1) / np.linalg.norm(X, axis=1)
    assert rel.max() <= max(16 * spread.max(), FLOOR)


def test_median_is_numpys():
    rs = np.random.RandomState(3)
    for n in (1, 2, 3, 4, 64, 65, 1000, 1001):
        d = rs.uniform(0, 30, n)
        assert orc.median(d) == np.median(d)
        med, keep = orc.gate_median(d, 1.2)
        assert med == np.median(d) * 1.2 and np.array_equal(keep, d < med)
    d = np.full(10, 2.5)
    assert orc.median(d) == 2.5 and orc.gate_median(d, 1.2)[1].all()
    d[3] = np.nan
    med, keep = orc.gate_median(d, 1.2)
    assert np.isnan(med) and not keep.any() and np.isnan(orc.median(np.zeros(0)))


# ---- hand cases ------------------------------------------------------------------------------------------------------------------

def hand(name):
    return orc.update(**tc.hand_cases()[name])


def test_no_pair():
    u = hand("no_pair")
    assert u.summary.tolist() == [0, 0, 0, 0, 0, 0, 0, 4] and np.isnan(u.median[0]) and u.new_points.shape == (0, 3)
    assert (u.pair_kf == -1).all() and (u.q_pt_ids == -1).all() and np.isnan(u.pair_dist).all() and u.unmatched_q.tolist() == [0, 1, 2, 3]


def test_one_known_pair():
    u = hand("one_known")
    d = u.pair_dist[0, 0]
    assert u.summary.tolist() == [1, 1, 1, 0, 0, 0, 0, 2] and u.median[0] == 1.2 * d and d < 1e-3 and np.isnan(u.pair_dist[0, 1])
    assert u.q_pt_ids.tolist() == [0, -1, -1] and u.unmatched_q.tolist() == [1, 2, -1]


def test_two_known_pairs_take_the_even_median():
    u = hand("two_known")
    d = u.pair_dist[:2, 0]
    assert d[1] > 1.9 and d[0] < 1e-3            # pair 0 -> query 1 (exact), pair 1 -> query 0 (moved by 2 px)
    assert u.median[0] == 1.2 * ((d[0] + d[1]) / 2.0) == 1.2 * np.median(d)
    assert u.q_pt_ids.tolist() == [0, -1, -1] and u.summary.tolist() == [2, 2, 1, 0, 0, 0, 0, 1]


def test_tied_distances_are_all_kept():
    u = hand("tied_distances")
    d = u.pair_dist[:, 0]
    assert (d == d[0]).all() and d[0] > 1 and u.median[0] == 1.2 * d[0]
    assert u.q_pt_ids.tolist() == [0, 0, 0, 0] and u.summary.tolist() == [4, 4, 4, 0, 0, 0, 0, 0]


def test_a_nan_point_makes_the_median_nan_and_keeps_nothing():
    u = hand("nan_point")
    assert np.isnan(u.median[0]) and np.isnan(u.pair_dist[1, 0]) and np.isfinite(u.pair_dist[[0, 2], 0]).all()
    assert u.q_pt_ids[:3].tolist() == [-1, -1, -1] and u.summary[:3].tolist() == [4, 3, 0]
    assert u.summary[3:6].tolist() == [1, 1, 0] and u.q_pt_ids[3] == 4         # the candidate is not touched by the gate
    assert u.pair_dist.view(np.uint64)[1, 0] == 0x7ff8000000000000


def test_identical_cameras_remove_the_pair_and_count_it():
    c = tc.hand_cases()["identical_cameras"]
    u = orc.update(**c)
    P = orc.projection_matrix(c["K_kf"], c["pose_kf"])
    X = orc.triangulate_raw(P, P, c["kf_xy"][:2], c["q_xy"][:2])
    rep = orc.reproj_dist(X, c["K_q"], c["pose_q"], c["q_xy"][:2])
    assert not (np.isfinite(X).all(axis=1) & np.isfinite(rep)).any()      # the point at infinity (v[3] = 0) or the centre (0 / 0)
    assert u.summary.tolist() == [3, 1, 1, 2, 0, 2, 0, 0] and u.q_pt_ids.tolist() == [-1, -1, 0] and u.new_points.shape == (0, 3)


def test_out_of_range_matches_and_ids_are_ignored_and_counted():
    u = hand("out_of_range")
    # matches0 = [0, 5, -2, 3, 4, 1] over 5 query points: 5 and -2 make no pair; ids [0, -1, 1, 9, -3, -1]: 9 and -3 are ignored
    assert u.pair_kf.tolist() == [0, 3, 4, 5, -1, -1] and u.pair_q.tolist() == [0, 3, 4, 1, -1, -1]
    assert u.summary[[0, 1, 3, 6, 7]].tolist() == [4, 1, 1, 4, 1] and u.unmatched_q.tolist() == [2, -1, -1, -1, -1]
    assert u.q_pt_ids[1] == -1 and u.q_pt_ids[2] == -1 and np.isnan(u.pair_dist[1:3]).all()


def test_two_pairs_on_one_query_point_both_stand():
    u = hand("two_pairs_one_query")
    assert u.pair_kf[:3].tolist() == [0, 1, 2] and u.pair_q[:3].tolist() == [1, 1, 0]
    assert u.summary[[0, 7]].tolist() == [3, 2] and u.unmatched_q.tolist() == [2, 3, -1, -1]


def test_an_empty_map_makes_every_pair_a_candidate():
    u = hand("no_points")
    assert u.summary.tolist() == [3, 0, 0, 3, 3, 0, 0, 0] and u.q_pt_ids.tolist() == [0, 1, 2] and np.isnan(u.median[0])
    assert np.abs(u.new_points - tc.HAND_X[:3]).max() < 1e-5          # exact projections rounded to fp32


def test_constants():
    from onepose_amd import _native_trk
    assert orc.MAX_KEYPOINTS == _native_trk.MAX_KEYPOINTS and orc.SUMMARY_ENTRIES == _native_trk.SUMMARY_ENTRIES
