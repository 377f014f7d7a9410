"""Every generated case of the object database builder's GPU tests (tests/test_map_hip.py, tests/test_map_module.py) meets the
exactness conditions of tests/map_cases.py: the cap that keeps those exact comparisons honest.  No GPU needed."""
import numpy as np
import pytest

import map_cases as mc
import mapping_oracle as mo


@pytest.mark.parametrize("P", mc.VERIFY_PAIRS)
def test_verification_cases_meet_the_conditions(P):
    b = mc.verify_batch(P)
    assert len(b["pairs"]) == P and all(all(c["conditions"]) for c in b["pairs"])
    assert P < 65 or set(mc.VERIFY_MATCHES) <= {c["n"] for c in b["pairs"]}
    assert b["match_offsets"][-1] == len(b["matches0"]) and b["kpt_offsets"][-1] == len(b["kpts"])


def test_single_pair_cases_cover_the_reporting_and_chunk_edges():
    cases = [mc.verify_pair_case(n, 3) for n in mc.VERIFY_MATCHES]
    assert all(all(c["conditions"]) for c in cases)
    assert [int(((c["matches0"] > -1) & (c["matches0"] < len(c["kpj"]))).sum()) for c in cases] == mc.VERIFY_MATCHES
    counts = [len(c["survivors"]) for c in cases]
    assert counts[:4] == [0, 14, 15, 16] and all(0 < k < n for k, n in zip(counts[4:], mc.VERIFY_MATCHES[4:]))   # of the large ones some fail
    assert [c["count"] for c in cases] == [0, 0, 15, 16] + counts[4:]                                 # fewer than 15 survivors report 0


@pytest.mark.parametrize("m", mc.TRACK_LENGTHS)
def test_track_cases_meet_the_conditions(m):
    for kind in mc.TRACK_KINDS:
        c = mc.track_case(m, kind, 1)
        assert all(c["conditions"]), (m, kind, c["conditions"])
        assert c["result"]["ok"] == (kind != "narrow"), (m, kind)
    a, b = mo.hypotheses(m)
    assert len(a) == min(m * (m - 1) // 2, mo.MAX_HYPOTHESES) and np.all(a != b)
    assert (m <= 16) == bool(np.all(a < b) and len(set(zip(a.tolist(), b.tolist()))) == len(a) == m * (m - 1) // 2)


@pytest.mark.parametrize("T", mc.TRACK_BATCHES)
def test_batched_track_cases_meet_the_conditions(T):
    cases = mc.batch_cases(T)
    assert len(cases) == T and all(all(c["conditions"]) for c in cases)


def test_budget_cases_meet_the_conditions():
    c = mc.track_case(8, "outliers", 2)
    for budget in (28, 27, 1):
        assert all(mc.track_conditions(mo.triangulate_track(c["cams"], c["xy"], max_hypotheses=budget)))
    for c in (mc.track_case(8, "clean", 0), mc.track_case(65, "clean", 0)):
        assert all(c["conditions"])
    assert all(mc.track_conditions(mo.triangulate_track(mc.track_case(8, "clean", 0)["cams"][1:], mc.track_case(8, "clean", 0)["xy"][1:])))


@pytest.mark.parametrize("n", mc.POINT_COUNTS)
def test_point_cases_meet_the_conditions(n):
    c = mc.points_case(n)
    assert all(c["conditions"])
    if n >= 31:
        thr = mo.track_length_threshold(c["lengths"], c["max_num_kp3d"])
        present = np.unique(c["lengths"][c["lengths"] > 0])
        assert present[0] < thr < present[-1]                          # the rule lands on a middle bin
        ids, xyz = mo.filter_points(c["xyz"], c["lengths"], thr, c["box"])
        assert 0 < len(ids) < (c["lengths"] > 0).sum()                 # the box and the length both reject something
        _, members = mo.merge_points(xyz)
        assert max(len(m) for m in members) >= 2


def test_the_module_scenes_meet_the_conditions():
    import test_map_module as tm
    for name in tm.SCENES:
        scene, ref = tm.scene_and_reference(name)
        assert all(tm.scene_conditions(scene, ref)), name
