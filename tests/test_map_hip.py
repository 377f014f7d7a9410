"""The object database builder's HIP library (include/mapping/mapping.h) stage by stage through its C ABI (one call per
onepose_amd.mapping.MapTail method) against the numpy oracle (tests/mapping_oracle.py).  The oracle restates every expression in
the kernels' order, so survivors, counts, hypothesis indices, inlier masks, kept ids, merged members and gathered descriptors are
compared exactly; the triangulated point is held to the bound of DESIGN section 13.  Every case meets the exactness conditions
of tests/map_cases.py (asserted for all of them in tests/test_map_cases.py, and again here)."""
import numpy as np
import pytest
import torch

import map_cases as mc
import mapping_oracle as mo
from onepose_amd.mapping import MapTail

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tail():
    return MapTail("cuda:0")


def host(t):
    return t.cpu().numpy()


# ---- verification ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", mc.VERIFY_PAIRS)
def test_verify_survivors_and_counts_are_identical(tail, P):
    b = mc.verify_batch(P)
    out, counts = tail.verify(b["kpts"], b["kpt_offsets"], b["cams"], b["pair_images"], b["match_offsets"], b["matches0"])
    out, counts = host(out), host(counts)
    for p, c in enumerate(b["pairs"]):
        assert all(c["conditions"])
        assert counts[p] == c["count"], (p, len(c["matches0"]), counts[p], c["count"])
        base = b["match_offsets"][p]
        assert np.array_equal(out[base:base + c["count"]], c["survivors"][:c["count"]]), p
    if P == 65:
        assert set(mc.VERIFY_MATCHES) <= {c["n"] for c in b["pairs"]}                      # every size of the list in one launch


@pytest.mark.parametrize("n", mc.VERIFY_MATCHES)
def test_verify_single_pair_sizes(tail, n):
    """The min_pair_inliers edge (14 / 15 / 16 matches of which some fail) and the 1024-thread chunk edge, one pair per launch."""
    c = mc.verify_pair_case(n, 3)
    assert all(c["conditions"])
    out, counts = tail.verify(np.concatenate([c["kpi"], c["kpj"]]), [0, len(c["kpi"]), len(c["kpi"]) + len(c["kpj"])], c["cams"], [[0, 1]],
                              [0, len(c["matches0"])], c["matches0"])
    assert int(counts[0]) == c["count"]
    assert np.array_equal(host(out)[:c["count"]], c["survivors"][:c["count"]])
    # every survivor below the reporting threshold gives 0
    out, counts = tail.verify(np.concatenate([c["kpi"], c["kpj"]]), [0, len(c["kpi"]), len(c["kpi"]) + len(c["kpj"])], c["cams"], [[0, 1]],
                              [0, len(c["matches0"])], c["matches0"], min_pair_inliers=len(c["survivors"]) + 1)
    assert int(counts[0]) == 0


# ---- triangulation ---------------------------------------------------------------------------------------------------
def run_tracks(tail, cases, **kw):
    b = mc.track_batch(cases)
    xyz, mask, info, lengths = tail.triangulate(b["track_offsets"], b["obs_image"], b["obs_xy"], b["cams"], b["max_len"], **kw)
    torch.cuda.synchronize()
    return b, host(xyz), host(mask), host(info), host(lengths)


def xyz_bound(case):
    """4 x the oracle's own fp64 error against its longdouble evaluation of the same inliers, plus 4 ulps of the output scale
    (the rule of the SuperGlue and detector stage tests)."""
    r = case["result"]
    ld = mo.refit(case["cams"], case["xy"], r["inliers"], r["start"], dtype=np.longdouble)
    own = float(np.abs(r["xyz"] - ld).max())
    return 4 * own + 4 * np.finfo(np.float64).eps * float(np.abs(ld).max()), own


def check_tracks(cases, b, xyz, mask, info, lengths):
    worst = (0.0, 0.0)
    for t, c in enumerate(cases):
        r = c["result"]
        assert all(c["conditions"]), (t, c["conditions"])
        s, e = b["track_offsets"][t], b["track_offsets"][t + 1]
        assert info[t].tolist() == list(r["info"]), (t, e - s, c["kind"], info[t].tolist(), r["info"])
        assert np.array_equal(mask[s:e], r["mask"].astype(np.int32)), (t, e - s, c["kind"])
        assert lengths[t] == r["length"]
        if r["ok"]:
            bound, own = xyz_bound(c)
            err = float(np.abs(xyz[t] - r["xyz"]).max())
            if err > worst[0]:
                worst = (err, bound)
            print(f"m={e - s} {c['kind']}: |HIP - oracle| {err:.3e}, oracle's own error {own:.3e}, bound {bound:.3e}")
            assert err <= bound, (t, e - s, c["kind"], err, bound)
        else:
            assert (xyz[t] == 0).all()
    return worst


@pytest.mark.parametrize("m", mc.TRACK_LENGTHS)
def test_track_lengths_of_every_kind(tail, m):
    """Wave edge (63, 64, 65), workgroup path (65, 200), all pairs against sampled pairs (16, 17), every kind of track."""
    cases = [mc.track_case(m, kind, 1) for kind in mc.TRACK_KINDS]
    b, xyz, mask, info, lengths = run_tracks(tail, cases)
    worst = check_tracks(cases, b, xyz, mask, info, lengths)
    print(f"m={m}: worst |HIP - oracle| {worst[0]:.3e} (bound {worst[1]:.3e})")
    kinds = {c["kind"]: c["result"] for c in cases}
    assert not kinds["narrow"]["ok"]
    if m >= 3:
        assert kinds["behind"]["ok"] and not kinds["behind"]["mask"].all()
        assert kinds["outliers"]["ok"] and not kinds["outliers"]["mask"].all()


@pytest.mark.parametrize("T", mc.TRACK_BATCHES)
def test_batched_tracks_match_the_oracle_each_alone_and_twice(tail, T):
    cases = mc.batch_cases(T)
    b, xyz, mask, info, lengths = run_tracks(tail, cases)
    check_tracks(cases, b, xyz, mask, info, lengths)
    _, xyz2, mask2, info2, lengths2 = run_tracks(tail, cases)                              # two runs: bitwise equal
    assert xyz.tobytes() == xyz2.tobytes() and np.array_equal(mask, mask2) and np.array_equal(info, info2) and np.array_equal(lengths, lengths2)
    for t in range(T):                                                                     # every track alone: bitwise equal
        _, x1, m1, i1, l1 = run_tracks(tail, [cases[t]])
        s, e = b["track_offsets"][t], b["track_offsets"][t + 1]
        assert x1[0].tobytes() == xyz[t].tobytes() and np.array_equal(m1, mask[s:e]) and np.array_equal(i1[0], info[t]) and l1[0] == lengths[t], t


def test_hypothesis_budget_on_both_sides(tail):
    """m (m - 1) / 2 = 28 observation pairs: enumerated with a budget of 28, hash-sampled with 27."""
    c = mc.track_case(8, "outliers", 2)
    for budget in (28, 27, 1):
        r = mo.triangulate_track(c["cams"], c["xy"], max_hypotheses=budget)
        case = dict(c, result=r, conditions=mc.track_conditions(r))
        b, xyz, mask, info, lengths = run_tracks(tail, [case], max_hypotheses=budget)
        check_tracks([case], b, xyz, mask, info, lengths)


def test_refused_tracks(tail):
    """A single observation, an image index out of range and a track longer than the bound the caller promised: ok = 0, while
    their neighbours in the batch are triangulated."""
    c8, c65 = mc.track_case(8, "clean", 0), mc.track_case(65, "clean", 0)
    b = mc.track_batch([c8, c8, c8, c65])
    offs = np.array([0, 1, 8, 16, 24, 89], np.int32)
    img = b["obs_image"].copy()
    img[10] = 10 ** 6
    xyz, mask, info, lengths = (host(t) for t in tail.triangulate(offs, img, b["obs_xy"], b["cams"], 64))
    seven = mo.triangulate_track(c8["cams"][1:], c8["xy"][1:])
    assert info.tolist() == [[0, 1, -1, 0], seven["info"], [0, 8, -1, 0], c8["result"]["info"], [0, 65, -1, 0]]
    assert lengths.tolist() == [0, 7, 0, 8, 0] and seven["ok"] and c8["result"]["ok"]
    assert (mask[:1] == 0).all() and (mask[8:16] == 0).all() and (mask[24:] == 0).all() and mask[1:8].all() and mask[16:24].all()
    assert (xyz[[0, 2, 4]] == 0).all() and np.isfinite(xyz).all()


# ---- threshold, filter, merge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mc.POINT_COUNTS)
def test_threshold_filter_and_merge_are_identical(tail, n):
    c = mc.points_case(n)
    assert all(c["conditions"])
    thr = tail.track_length_threshold(c["lengths"], c["max_num_kp3d"])
    ref_thr = mo.track_length_threshold(c["lengths"], c["max_num_kp3d"])
    assert int(thr) == ref_thr
    ids, xyz32 = tail.filter_points(c["xyz"], c["lengths"], thr, c["box"])
    ref_ids, ref_xyz = mo.filter_points(c["xyz"], c["lengths"], ref_thr, c["box"])
    assert np.array_equal(host(ids), ref_ids) and host(xyz32).tobytes() == ref_xyz.tobytes()
    if len(ref_ids) == 0:
        return
    merged, offs, members = tail.merge_points(xyz32)
    ref_merged, ref_members = mo.merge_points(ref_xyz)
    assert host(merged).tobytes() == ref_merged.tobytes()
    assert np.array_equal(host(offs), np.concatenate([[0], np.cumsum([len(m) for m in ref_members])]))
    assert np.array_equal(host(members), np.concatenate(ref_members))
    if n >= 31:
        sizes = sorted(len(m) for m in ref_members)
        where = {int(i): k for k, i in enumerate(ref_ids)}
        groups = [set(ref_ids[m].tolist()) for m in ref_members]
        if all(i in where for i in (2, 5)):
            assert {2, 5} in groups
        if all(i in where for i in (7, 11, 20)):
            assert {7, 11, 20} in groups and sizes[-1] == 3
        if all(i in where for i in (14, 17, 25)):                   # 14 founds {14, 17}; 17 and 25 see a taken member: 25 is dropped
            assert {14, 17} in groups and not any(25 in g for g in groups)


def test_threshold_rule_as_written(tail):
    """filter_tkl.py:42-50: absent lengths are not walked; points of exactly the returned length come back in."""
    for lengths, max_num, want in [([3, 3, 5, 5, 5, 9], 10, 3), ([3, 3, 5, 5, 5, 9], 4, 3), ([3, 3, 5, 5, 5, 9], 3, 5), ([3, 3, 5, 5, 5, 9], 0, 9),
                                   ([0, 0, 0], 5, 0), ([2, 0, 7], 1, 2), ([2000, 4], 0, 1023)]:
        assert mo.track_length_threshold(lengths, max_num) == want
        assert int(tail.track_length_threshold(np.array(lengths, np.int32), max_num)) == want


# ---- gather ----------------------------------------------------------------------------------------------------------
def test_gather_is_bitwise_equal_to_the_oracle(tail):
    c = mc.gather_case()
    cd, cs, idxs, md, ms = (host(t) for t in tail.gather([f["descriptors"] for f in c["features"]], [f["scores"] for f in c["features"]],
                                                         c["point_offsets"], c["obs_image"], c["obs_kpt"]))
    r_cd, r_cs, r_idxs, r_md, r_ms = mo.gather_descriptors(c["features"], c["point_offsets"], c["obs_image"], c["obs_kpt"])
    assert idxs.tolist() == r_idxs.tolist() == mc.GATHER_COUNTS + [3, 3]
    assert cd.tobytes() == r_cd.tobytes() and cs.tobytes() == r_cs.tobytes()
    assert md.tobytes() == r_md.tobytes() and ms.tobytes() == r_ms.tobytes()
