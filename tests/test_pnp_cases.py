"""Every generated case of the pose solver's stage tests (tests/test_pnp_stages.py) meets the conditions of tests/pnp_cases.py: the
cap that keeps those exact comparisons honest.  No GPU needed."""
import numpy as np
import pytest

import pnp_cases as pc
from oracle import pnp_oracle as po


def test_the_restated_inlier_test_is_the_oracles():
    """residuals2 / inlier_masks against oracle/pnp_oracle.py's reproj_err2 on the same fp64 points, and the non-finite side."""
    c = pc.score_case(129, 257)
    pw, uv = c["pts_3d"].astype(np.float64) * pc.SCALE, c["pts_2d"].astype(np.float64)
    for h in (0, 1, 100, 256):
        P = c["hyp"][h].reshape(3, 4)
        np.testing.assert_allclose(pc.residuals2(c["hyp"][h], c["pts_3d"], c["pts_2d"], c["K"])[0], po.reproj_err2(P[:, :3], P[:, 3], pw, uv, c["K"]),
                                   rtol=1e-9)
    nan = np.full(12, np.nan)
    assert not pc.inlier_masks(nan, c["pts_3d"], c["pts_2d"], c["K"]).any()
    assert pc.clear_of_threshold(nan, c["pts_3d"], c["pts_2d"], c["K"]) == (True, float("inf"))
    on_it = np.concatenate([np.eye(3), [[0.0], [0.0], [1.0]]], axis=1).reshape(12)       # a residual of exactly 25: an inlier, and refused
    p3, p2, K = np.zeros((1, 3), np.float32), np.array([[3.0, 4.0]], np.float32), np.eye(3)
    assert pc.inlier_masks(on_it, p3, p2, K, 1.0).all() and pc.clear_of_threshold(on_it, p3, p2, K, 1.0) == (False, 0.0)


@pytest.mark.parametrize("n", pc.SCORE_N)
def test_scoring_cases_meet_the_conditions(n):
    for iterations in pc.SCORE_ITERATIONS:
        c = pc.score_case(n, iterations)
        assert all(c["conditions"]) and c["gap"] > pc.MARGIN and c["hyp"].shape == (iterations, 12)
        rows, counts = c["rows"], c["counts"]
        assert len(rows) == min(iterations, 4) and (iterations < 5 or set(rows) == set(pc.SPECIAL_ROWS))
        if "nan" in rows:
            assert np.isnan(c["hyp"][rows["nan"]]).all() and counts[rows["nan"]] == 0
        if "negated" in rows:                                                   # no depth test: the planted pose's count
            assert counts[rows["negated"]] == c["planted_count"] > 0
        if "planted" in rows:
            assert counts[rows["planted"]] == c["planted_count"]
        if "z0" in rows:
            e = pc.residuals2(c["hyp"][rows["z0"]], c["pts_3d"], c["pts_2d"], c["K"])[0]
            assert np.isnan(e[c["k"]]) and not c["masks"][rows["z0"], c["k"]]
        if iterations >= 255 and n >= 63:                                       # from nothing to (nearly) everything the planted pose has
            assert counts.min() == 0 and counts.max() >= c["planted_count"] and len(np.unique(counts)) > min(n, 40) // 4


def test_single_hypothesis_scoring_cases_cover_every_planted_row():
    assert {name for n in pc.SCORE_N for name in pc.score_case(n, 1)["rows"]} == set(pc.SPECIAL_ROWS)


@pytest.mark.parametrize("n", pc.BEST_N)
def test_selection_cases_meet_the_conditions(n):
    prob = pc.best_problem(n)
    assert all(prob["conditions"]) and prob["gap"] > pc.MARGIN
    a, b = prob["masks"]["A"], prob["masks"]["B"]
    assert a.any() and b.any() and (a != b).any()
    for edge in range(1024, n, 1024):
        assert a[:edge].any() and a[edge:].any() and a[edge - 1024:edge].any() and a[edge:edge + 1024].any()
    for iterations in pc.BEST_ITERATIONS:
        places = pc.best_placements(iterations)
        assert {"first", "last", "all_equal"} <= set(places)
        for name, idx in places.items():
            c = pc.best_case(n, iterations, name)
            counts = c["counts"]
            assert counts.dtype == np.int32 and counts.max() == pc.BEST_MAX >= po.MODEL_POINTS
            assert tuple(np.nonzero(counts == counts.max())[0]) == idx and int(np.argmax(counts)) == idx[0] == c["argmax"]
            assert np.array_equal(c["hyp"][idx[0]], prob["poses"]["A"]) and all(np.array_equal(c["hyp"][j], prob["poses"]["B"]) for j in idx[1:3])
        for kind in ("below5", "zeros"):
            f = pc.failing_counts(iterations, kind)
            assert f.dtype == np.int32 and f.min() >= 0 and f.max() == (4 if kind == "below5" else 0) < po.MODEL_POINTS
    full = pc.best_placements(10000)
    assert full["lower_in_higher_thread"] == (1000, 1024) and 1000 % 1024 > 1024 % 1024        # thread of the lower index is the higher one
    assert full["same_thread"][0] % 1024 == full["same_thread"][1] % 1024


@pytest.mark.parametrize("n", pc.HYP_N)
def test_hypothesis_cases_meet_the_conditions(n):
    for seed in pc.HYP_SEEDS:
        c = pc.hyp_case(n, seed)
        assert all(c["conditions"])
        n_in = int(c["planted"].sum())
        assert (n_in == n) == (n == 5) and c["clean"].any()
        assert np.array_equal(c["oracle_counts"] == n_in, c["clean"])
        assert c["samples"].shape == (256, 5) and all(len(set(s)) == 5 for s in c["samples"].tolist()) and c["samples"].max() < n


def test_wrapping_seeds_draw_other_samples():
    """seed << 40 wraps for the two large seeds: they must still differ from each other and from the small ones."""
    s = [tuple(map(tuple, pc.hyp_case(300, seed)["samples"].tolist())) for seed in pc.HYP_SEEDS]
    assert len(set(s)) == len(s)
    assert (2 ** 24 + 3) << 40 >= 2 ** 64 and (2 ** 63 + 1) << 40 >= 2 ** 64


def test_chain_cases_are_solvable_problems():
    for name, (n, outl, noise, _) in pc.CHAIN_CASES.items():
        p = pc.chain_case(name)
        assert len(p["pts_3d"]) == n and 0.5 * n < p["inlier_mask"].sum() < n
