"""tests/train_oracle.py (numpy fp64: the mathematics of include/gatsspg_train.h and reshape_assign_matrix) against what the unmodified
reference gives under autograd in fp64 (tests/golden/train_*.npz, tests/golden/make_train_golden.py).  No GPU."""
import json
import os

import numpy as np
import pytest

import train_oracle
from conftest import GOLDEN_DIR, load_golden

with open(os.path.join(GOLDEN_DIR, "train_golden_meta.json")) as f:
    META = json.load(f)
HEAD_CASES = sorted(META["head"])


def head_case(name):
    """(x, y, pairs, target, focal arguments by the oracle's names, golden, meta)"""
    meta = META["head"][name]
    x, y, pairs, target = train_oracle.make_head_case(**meta["inputs"])
    f = meta["focal"]
    focal = dict(alpha=f["alpha"], gamma=f["gamma"], pos_w=f["pos_weights"], neg_w=f["neg_weights"], scale=meta["scale"])
    return x, y, pairs, target, focal, load_golden("train_head_" + name), meta


def test_the_cases_cover_what_they_should():
    assert HEAD_CASES == ["edge", "no_negative", "no_positive", "pad0", "small"]
    for name in HEAD_CASES:
        _, _, _, target, _, g, meta = head_case(name)
        np.testing.assert_array_equal(target, g["target"])                      # the recipe rebuilds the golden's inputs
        if meta["conf_positive_min_max"]:                                       # the recipe's point: positives spread, none saturated
            lo, hi = meta["conf_positive_min_max"]
            assert lo < 1e-3 and 1e-3 < hi < 0.999 and meta["conf_max"] < 0.999
    assert (head_case("no_positive")[3] == 1).sum() == 0 and (head_case("no_negative")[3] == 0).sum() == 0
    edge = head_case("edge")
    assert (edge[3] == -1).sum() > 0 and edge[2][0][0, -1] == 129 and edge[3][0, 129, 69] == -1   # a positive inside the ignored band


@pytest.mark.parametrize("name", HEAD_CASES)
def test_oracle_head_equals_the_reference_under_fp64_autograd(name):
    x, y, _, target, focal, g, _ = head_case(name)
    o = train_oracle.head(x, y, train_oracle.classes(target), **focal)
    assert abs(o["loss"] - float(g["loss"])) <= 1e-12 * abs(float(g["loss"]))
    for key in ("dx", "dy"):
        assert np.abs(o[key] - g[key]).max() <= 1e-11 * np.abs(g[key]).max(), key
    np.testing.assert_array_equal(o["counts"], [(target == 1).sum(), (target == 0).sum(), ((target != 0) & (target != 1)).sum()])


def test_oracle_stages_compose_to_the_head():
    x, y, _, target, focal, _, _ = head_case("edge")
    cls = train_oracle.classes(target)
    o = train_oracle.head(x, y, cls, **focal)
    E, r, c = train_oracle.scores_exp(x, y, focal["scale"])
    kw = {k: focal[k] for k in ("alpha", "gamma", "pos_w", "neg_w")}
    t = train_oracle.loss_terms(E, r, c, cls, **kw)
    dS = train_oracle.score_grad(E, r, c, cls, t["counts"], t["rowsum_h"], t["colsum_h"], **kw)
    assert t["loss"] == o["loss"] and np.abs(dS - o["dS"]).max() <= 1e-15 * np.abs(o["dS"]).max()


def test_neither_positive_nor_negative_gives_zero():
    x, y, _, target = train_oracle.make_head_case(b=1, n=5, m=7, k=0, seed=3, positives=False)
    o = train_oracle.head(x, y, np.full(target.shape, 2, dtype=np.int8))
    assert o["loss"] == 0.0 and not o["dx"].any() and not o["dy"].any() and list(o["counts"]) == [0, 0, 35]


@pytest.mark.parametrize("name", sorted(META["assign"]))
def test_oracle_reshape_assign_equals_the_reference(name):
    g, s = load_golden("train_assign"), META["assign"][name]
    pairs = g[name + ".pairs"]
    assert (pairs[0] >= s["n"]).any() and (pairs[1] >= s["m"]).any() and (pairs[:, 5] == pairs[:, 2]).all()
    out = train_oracle.reshape_assign(pairs, s["n_orig"], s["m_orig"], s["n"], s["m"], s["pad_val"])
    np.testing.assert_array_equal(out, g[name + ".target"])
    assert out.dtype == np.int16
    if name in ("a", "b"):
        assert out[s["n"] - 1, s["m"] - 1] == s["pad_val"]                      # the pair inside the pad band was overwritten
    # a negative index is ignored, not wrapped around
    neg = np.concatenate([pairs, np.array([[-1, 2], [3, -2]], dtype=np.int32)], axis=1)
    np.testing.assert_array_equal(train_oracle.reshape_assign(neg, s["n_orig"], s["m_orig"], s["n"], s["m"], s["pad_val"]), out)
