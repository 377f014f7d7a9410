"""The numpy SuperGlue oracle (tests/superglue_oracle.py) reproduces every reference-run golden (tests/golden/sg_*.npz)."""
import json
import os

import numpy as np
import pytest

from onepose_amd import synthetic
import superglue_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _meta():
    with open(os.path.join(GOLD, "sg_golden_meta.json")) as f:
        return json.load(f)


def case_inputs(spec):
    cfg = spec["cfg"]
    n_layers = len(cfg["GNN_layers"])
    fn = synthetic.make_superglue_passthrough_state_dict if spec["w"]["kind"] == "passthrough" else synthetic.make_superglue_state_dict
    sd = fn(spec["w"]["seed"], n_layers)
    inp = synthetic.make_superglue_inputs(**spec["inp"])
    return sd, inp, cfg


def clear_rows(gold):
    """Rows / columns whose best and second-best Z values are more than 1e-4 apart: the argmax there is not a near-tie."""
    if "Z" in gold:
        stats = so.z_stats(gold["Z"].astype(np.float64))
    else:
        stats = gold
    return stats["row_best"] - stats["row_second"] > 1e-4, stats["col_best"] - stats["col_second"] > 1e-4


def compare(out, Z, gold, ztol=1e-4, stol=1e-5):
    if "Z" in gold:
        np.testing.assert_allclose(Z, gold["Z"], rtol=0, atol=ztol)
    else:
        st = so.z_stats(Z)
        for k in ("row_best", "col_best", "dust_row", "dust_col"):
            np.testing.assert_allclose(st[k], gold[k], rtol=0, atol=ztol, err_msg=k)
    c0, c1 = clear_rows(gold)
    assert (out["matches0"][c0] == gold["matches0"][c0]).all()
    assert (out["matches1"][c1] == gold["matches1"][c1]).all()
    np.testing.assert_allclose(out["matching_scores0"], gold["matching_scores0"], rtol=2e-6, atol=stol)
    np.testing.assert_allclose(out["matching_scores1"], gold["matching_scores1"], rtol=2e-6, atol=stol)


CASES = ["tiny", "iters0", "iters1", "n1", "planted", "outdoor", "headline"]


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_golden(name):
    spec = _meta()["cases"][name]
    sd, inp, cfg = case_inputs(spec)
    gold = dict(np.load(os.path.join(GOLD, f"sg_{name}.npz")))
    out, Z = so.forward(sd, inp, cfg, np.float32)
    compare(out, Z, gold)


def test_planted_passthrough_recovers_every_pair():
    spec = _meta()["cases"]["planted"]
    sd, inp, cfg = case_inputs(spec)
    gold = dict(np.load(os.path.join(GOLD, "sg_planted.npz")))
    m0 = gold["matches0"][0]
    p0, p1 = inp["planted0"][0], inp["planted1"][0]
    assert (m0[p0] == p1).all()
    assert (m0 >= 0).sum() == len(p0)


def test_golden_files_stay_small():
    sizes = [os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD) if f.startswith("sg_") and f.endswith(".npz")]
    assert max(sizes) < 1_000_000 and sum(sizes) < 6_000_000


def test_match_tail_first_index_wins_on_ties():
    Z = np.zeros((1, 4, 5), np.float32)
    Z[0, :3, :4] = -5
    Z[0, 0, 1] = Z[0, 0, 3] = -0.1     # tie in row 0: column 1 wins
    Z[0, 2, 1] = -0.1                  # tie in column 1: row 0 wins
    out = so.match_tail(Z, 0.0)
    assert out["matches0"][0].tolist() == [1, -1, -1]
    assert out["matches1"][0].tolist() == [-1, 0, -1, -1]
