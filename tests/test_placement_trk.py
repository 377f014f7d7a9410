"""Placement tests of the tracker's map update step (include/mapping/track_update.h): trk_update, trk_gate_median and
trk_triangulate_pairs at the shapes 5x7, 63x65, 257x300 and 1025x1000 of track_cases.shape_cases(), every device argument an exact
piece of a guarded arena (tests/arena.py) under the fills 0xFF and 0x00; the workspace is exactly trk_workspace_bytes.  Every case
runs a second time with each call captured and replayed (arena.run_captured).  Bitwise comparisons only; the oracle comparisons stay
in tests/test_track_hip.py."""
import numpy as np
import pytest
import torch

import track_cases as tc
import track_oracle as orc
from arena import captured_twin, run_placement
from onepose_amd import _native_trk

BINDING = _native_trk
ROLES = {
    "trk_update": dict(matches0="in", kf_xy="in", q_xy="in", kf_pt_ids="in", points="in", K_kf="in", K_q="in", pose_kf="in", pose_q="in",
                       pair_kf="out", pair_q="out", q_pt_ids="out", pair_dist="out", new_points="out", unmatched_q="out", median="out",
                       summary="out", workspace="scratch"),
    "trk_triangulate_pairs": dict(P1="in", P2="in", xy1="in", xy2="in", X="out"),
    "trk_gate_median": dict(dist="in", median="out", keep="out", workspace="scratch"),
}
NAMES = ["5x7", "63x65", "257x300", "1025x1000"]
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("name", NAMES)
def test_update(name, run=run_placement):
    c = tc.shape_cases()[name]
    n_kf, n_q, n_points = len(c["matches0"]), len(c["q_xy"]), len(c["points"])
    nbytes = BINDING.load().trk_workspace_bytes(n_kf, n_q)
    assert nbytes > 0 and n_points > 0
    i32, f64 = torch.int32, torch.float64
    outputs = (("pair_kf", (n_kf,), i32), ("pair_q", (n_kf,), i32), ("q_pt_ids", (n_kf,), i32), ("pair_dist", (n_kf, 2), f64),
               ("new_points", (n_kf, 3), f64), ("unmatched_q", (n_q,), i32), ("median", (1,), f64), ("summary", (8,), i32))

    def body(mem):
        ins = [mem.place(tensor(c[k]), "in", k) for k in tc.INPUTS]
        outs = {nm: mem.place(torch.empty(s, dtype=t), "out", nm) for nm, s, t in outputs}
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "trk_update", *ins, n_kf, n_q, n_points, tc.GATE, tc.MAX_REPROJ, tc.MAX_Z, *outs.values(), ws, ws.numel())
        kept = int(outs["summary"][4])
        # the header: new_points "rows past the kept count are not written"
        return outs, {"new_points": outs["new_points"][:kept]}

    got = run(body, DEV, ROLES)
    m, kept = int(got["summary"][0]), int(got["summary"][4])
    assert 0 < m <= n_kf and (n_kf < 60 or 0 < kept < m)
    assert bool((got["new_points"][kept:].view(torch.int64) == -1).all())          # still the first pattern: every byte 0xFF


@pytest.mark.parametrize("name", NAMES)
def test_gate_median(name, run=run_placement):
    """n = the case's keyframe count; the distances of tests/test_track_hip.py (one run of them with ties).  The workspace is that of
    trk_workspace_bytes(n, 1), as the header says."""
    n = len(tc.shape_cases()[name]["matches0"])
    d = np.round(np.random.RandomState(1000 + n).uniform(0, 40, n) ** 2 / 40, 1)
    nbytes = BINDING.load().trk_workspace_bytes(n, 1)

    def body(mem):
        dist = mem.place(tensor(d), "in", "dist")
        median, keep = mem.place(torch.empty(1, dtype=torch.float64), "out", "median"), mem.place(torch.empty(n, dtype=torch.int32), "out", "keep")
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "trk_gate_median", dist, n, 1.2, median, keep, ws, ws.numel())
        return dict(median=median, keep=keep)

    got = run(body, DEV, ROLES)
    assert got["median"].item() == np.median(d) * 1.2 and got["keep"].tolist() == (d < np.median(d) * 1.2).astype(int).tolist()


@pytest.mark.parametrize("name", NAMES)
def test_triangulate_pairs(name, run=run_placement):
    """n = the case's keyframe count: one pair per keyframe keypoint, query keypoints taken in order (cycled)."""
    c = tc.shape_cases()[name]
    n = len(c["kf_xy"])
    xy1, xy2 = c["kf_xy"], np.ascontiguousarray(np.resize(c["q_xy"], (n, 2)))
    P1, P2 = orc.projection_matrix(tc.K, tc.POSE_KF), orc.projection_matrix(tc.K, tc.POSE_Q)

    def body(mem):
        ins = [mem.place(tensor(a), "in", nm) for a, nm in ((P1, "P1"), (P2, "P2"), (xy1, "xy1"), (xy2, "xy2"))]
        X = mem.place(torch.empty(n, 3, dtype=torch.float64), "out", "X")
        mem.call(BINDING, "trk_triangulate_pairs", *ins, n, X)
        return dict(X=X)

    run(body, DEV, ROLES)


# every case again with each library call captured in a graph and replayed (arena.run_captured): the stream contract
test_update_captured = captured_twin(test_update)
test_gate_median_captured = captured_twin(test_gate_median)
test_triangulate_pairs_captured = captured_twin(test_triangulate_pairs)
