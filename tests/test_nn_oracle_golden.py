"""The numpy oracle of the nearest-neighbour matcher (tests/nn_oracle.py) against goldens recorded by RUNNING THE REFERENCE
MODULE (tests/golden/make_nn_golden.py), and the comparison rule on every case the GPU tests use.  No GPU."""
import json
import os

import numpy as np
import pytest

import nn_cases
import nn_oracle as orc
from conftest import GOLDEN_DIR

GOLDENS = ("tiny", "plain", "ratio", "distance", "both", "nomutual", "batch")


def load(name):
    g = np.load(os.path.join(GOLDEN_DIR, f"nn_{name}.npz"))
    return g, json.loads(str(g["conf"]))


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_equals_the_reference_on_decided_rows_and_columns(name):
    g, conf = load(name)
    assert g["matches0"].dtype == np.int64 and g["matches1"].dtype == np.int64
    assert g["matching_scores0"].dtype == np.float32 and g["matching_scores1"].dtype == np.float32
    for i in range(g["descriptors0"].shape[0]):
        ref = orc.forward(g["descriptors0"][i], g["descriptors1"][i], conf)
        orc.compare({k: g[k][i] for k in orc.OUT_KEYS}, ref, f"{name}[{i}]")
        assert 0 < np.count_nonzero(ref["matches0"] > -1)


def test_goldens_cover_the_configurations():
    confs = [load(n)[1] for n in GOLDENS]
    assert any(c.get("do_mutual_check") is False for c in confs)
    assert any(c.get("ratio_threshold") and not c.get("distance_threshold") for c in confs)
    assert any(c.get("distance_threshold") and not c.get("ratio_threshold") for c in confs)
    assert any(c.get("distance_threshold") and c.get("ratio_threshold") for c in confs) and any(not c for c in confs)
    for n in GOLDENS:      # both outcomes of the tests occur
        m = load(n)[0]["matches1"]
        if load(n)[1].get("ratio_threshold") or load(n)[1].get("distance_threshold"):
            assert (m > -1).any() and (m == -1).any(), n


def test_reference_quirks_matches1_is_not_mutual_checked_and_scores0_survive():
    """The reference as written: the mutual check rewrites matches0 only.  Checked on the recorded reference outputs and on the oracle's."""
    dropped = kept1 = 0
    for name, i in [(n, i) for n in GOLDENS if load(n)[1].get("do_mutual_check", True) for i in range(load(n)[0]["matches0"].shape[0])]:
        g, conf = load(name)
        ref = orc.forward(g["descriptors0"][i], g["descriptors1"][i], conf)
        loose = orc.forward(g["descriptors0"][i], g["descriptors1"][i], {**conf, "do_mutual_check": False})
        for m0, m1, s0 in ((g["matches0"][i], g["matches1"][i], g["matching_scores0"][i]),
                           (ref["matches0"], ref["matches1"], ref["matching_scores0"])):
            # a column whose match does not point back keeps its match: matches1 is find_nn's, untouched
            back = m0[np.where(m1 > -1, m1, 0)]
            kept1 += np.count_nonzero((m1 > -1) & (back != np.arange(len(m1))))
            # a row the mutual check dropped keeps its score
            gone = (m0 == -1) & (loose["matches0"] > -1) & ref["decided0"]
            dropped += np.count_nonzero(gone)
            assert (s0[gone] > 0).all()
        assert np.array_equal(ref["matches1"], loose["matches1"]) and np.array_equal(ref["matching_scores0"], loose["matching_scores0"])
    print(f"rows dropped by the mutual check that keep their score: {dropped}; columns that keep a one-way match: {kept1}")
    assert dropped > 0 and kept1 > 0


def test_tie_rule_lowest_index_and_multiset_second():
    for side in ("rows", "cols"):
        d0, d1 = nn_cases.tie_pair(side)
        ref = orc.forward(d0, d1, {"do_mutual_check": False})
        strict = orc.forward(d0, d1, {"ratio_threshold": 0.99, "do_mutual_check": False})
        for r, a, b in nn_cases.TIE_ROWS if side == "rows" else ():
            assert ref["matches0"][r] == min(a, b) and strict["matches0"][r] == -1      # second == best: any ratio < 1 rejects
        for c, a, b in nn_cases.TIE_COLS if side == "cols" else ():
            assert ref["matches1"][c] == min(a, b) and strict["matches1"][c] == -1


def test_every_gpu_case_stays_under_the_cap():
    worst, count = 0.0, 0
    for name, d0, d1, conf in nn_cases.all_cases():
        ref = orc.forward(d0, d1, conf)
        assert ref["left_out"] <= orc.CAP, f"{name}: {ref['left_out']:.4f} of rows + columns undecided"
        worst, count = max(worst, ref["left_out"]), count + 1
    print(f"{count} cases, worst share left out {worst:.4f}")
    assert count > 100


def test_selection_case_is_what_it_says():
    """The planted best / second neighbours are the oracle's, and the tight ratio test hinges on the true second."""
    d0, d1 = nn_cases.selection_pair()
    sim = orc.similarity(d0, d1)
    for r, a, b in nn_cases.SEL_ROWS:
        order = np.argsort(-sim[r])
        assert (order[0], order[1]) == (a, b)
        dist = 2 * (1 - sim[r, order[:3]])
        assert dist[0] > 0.22 ** 2 * dist[1] and dist[0] < 0.22 ** 2 * dist[2] and dist[0] < 0.8 ** 2 * dist[1]
    for c, a, b in nn_cases.SEL_COLS:
        order = np.argsort(-sim[:, c])
        assert (order[0], order[1]) == (a, b)
    d0, d1 = nn_cases.negative_pair()
    assert orc.similarity(d0, d1).max() < -0.4
