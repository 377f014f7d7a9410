"""CPU checks of tests/gats_stage_reference.py: both dtype forms of every stage restatement against oracle/gatsspg_oracle.py
(itself pinned on the goldens of the reference module), and the properties of the GPU test's cases that can be vouched for
without a GPU -- the kernel-form table against the thresholds in the launchers, the conditioning of the attention shapes, and
the near-tie count of the score cases."""
import os
import re

import numpy as np
import pytest

import gats_stage_reference as R
from conftest import TIE_GAP
from oracle import gatsspg_oracle as orc
from onepose_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK_ATOL = 2e-5      # what test_hip_parity.py::test_f64_yardstick_agrees_with_the_oracle holds the float64 yardstick to
DTYPES = [np.float32, np.float64]
SMALL = [(1, 90, 140), (2, 5, 33), (3, 64, 129)]   # (b, n1, n2)


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


@pytest.fixture(scope="module")
def sd():
    return synthetic.make_state_dict(0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,n1,n2", SMALL)
def test_attention_propagation_agrees_with_the_oracle(sd, b, n1, n2, dtype):
    data = synthetic.make_inputs(b=b, n1=n1, n2=n2, num_leaf=1, seed=11)
    x, y = data["descriptors2d_query"], data["descriptors3d_db"]
    for p, a, s in (("gnn.layers.1", x, x), ("gnn.layers.1", y, y), ("gnn.layers.2", x, y), ("gnn.layers.2", y, x)):
        got = R.attention_propagation(sd, p, a, s, dtype)
        assert got.dtype == dtype
        assert maxdiff(got, orc.attention_propagation(sd, p, a, s)) < YARDSTICK_ATOL
    d2, d3 = R.attention_layer_deltas(sd, "gnn.layers.2", x, y, "cross", dtype)
    assert np.array_equal(d2, R.attention_propagation(sd, "gnn.layers.2", x, y, dtype))
    assert np.array_equal(d3, R.attention_propagation(sd, "gnn.layers.2", y, x, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flags", [1, 0, 3, 5, 7, 4])
@pytest.mark.parametrize("b,n2,num_leaf", [(2, 5, 8), (1, 65, 3), (3, 17, 1)])
def test_graph_attention_layer_agrees_with_the_oracle(sd, b, n2, num_leaf, flags, dtype):
    data = synthetic.make_inputs(b=b, n1=4, n2=n2, num_leaf=num_leaf, seed=5)
    h2 = np.transpose(data["descriptors2d_db"], (0, 2, 1))
    h3 = np.transpose(data["descriptors3d_db"], (0, 2, 1))
    inc, add, wlt = bool(flags & 1), bool(flags & 2), bool(flags & 4)
    for layer in (0, 9):
        W, a = sd[f"gnn.layers.{layer}.W"], sd[f"gnn.layers.{layer}.a"]
        got = R.graph_attention_layer(W, a, h2, h3, inc, add, wlt, dtype)
        assert got.dtype == dtype and got.shape == h3.shape
        assert maxdiff(got, orc.graph_attention_layer(W, a, h2, h3, inc, add, wlt)) < YARDSTICK_ATOL


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,n1,n2", SMALL)
def test_final_proj_and_dual_softmax_agree_with_the_oracle(sd, b, n1, n2, dtype):
    data = synthetic.make_inputs(b=b, n1=n1, n2=n2, num_leaf=1, seed=13, planted=True)
    x, y = data["descriptors2d_query"] * np.float32(3), data["descriptors3d_db"] * np.float32(3)
    m2, m3 = R.final_proj_normalize(sd, x, dtype), R.final_proj_normalize(sd, y, dtype)
    o2 = orc.l2_normalize(orc.conv1x1(sd["final_proj.weight"], sd["final_proj.bias"], x))
    o3 = orc.l2_normalize(orc.conv1x1(sd["final_proj.weight"], sd["final_proj.bias"], y))
    assert m2.dtype == dtype and maxdiff(m2, o2) < YARDSTICK_ATOL and maxdiff(m3, o3) < YARDSTICK_ATOL
    for scale in (0.07, 0.01):
        s = R.scores(m2, m3, scale, dtype)
        so = (np.einsum("bdn,bdm->bnm", o2, o3).astype(np.float32) / np.float32(scale)).astype(np.float32)
        assert s.dtype == dtype and maxdiff(s, so) < YARDSTICK_ATOL / scale
        conf, co = R.dual_softmax(s), orc.dual_softmax(so)
        assert conf.dtype == dtype and co.max() > 0.5 and maxdiff(conf, co) < YARDSTICK_ATOL
        ref = orc.mutual_nn_match(co, 0.0)
        m0, m1 = R.mutual_matches(conf)
        if min(R.top2_rel_gap(co.astype(np.float64), 2).min(), R.top2_rel_gap(co.astype(np.float64), 1).min()) >= 1e-3:
            np.testing.assert_array_equal(m0, ref["matches0"])
            np.testing.assert_array_equal(m1, ref["matches1"])


# ----------------------------------------------------------------------------------------------------------------------
# the GPU test's cases
# ----------------------------------------------------------------------------------------------------------------------
def _constant(text, name):
    m = re.search(r"constexpr\s+int\s+(?:\w+\s*=\s*\d+\s*,\s*)*" + name + r"\s*=\s*(\d+)", text)
    assert m, f"{name} not found"
    return int(m.group(1))


def test_form_table_straddles_every_launcher_threshold():
    """The kernel-form cases are only worth their time while each sits on the side of its threshold that the table names: read
    the thresholds from the launchers, recompute every row's tile count, and require a row on either side of each."""
    gemm = open(os.path.join(ROOT, "onepose_amd", "csrc", "gatsspg_gemm_kernels.hip")).read()
    split = open(os.path.join(ROOT, "onepose_amd", "csrc", "gatsspg_split_kernels.hip")).read()
    diet, small3 = _constant(gemm, "DIET_MIN_TILES"), _constant(gemm, "SMALL_NT3")
    wide_min, wide_max = _constant(split, "SP_MLP0_WIDE_MIN"), _constant(split, "SP_MLP0_WIDE_MAX")
    assert re.search(r"return\s+tiles\s*/\s*2\s*>=\s*wide_min\s*&&\s*tiles\s*/\s*2\s*<=\s*wide_max", split)
    m = re.search(r"\(256\s*/\s*T2::BM\)\s*\*\s*NT\s*>\s*(\d+)", split)
    assert m, "the two-stage ring's threshold of launch_mlp3_sp_t not found"
    ring = int(m.group(1))
    bm2 = re.search(r"using\s+Mlp3SpTile2\s*=\s*SpTile<\s*(\d+)\s*,", split)
    assert bm2, "Mlp3SpTile2's row count not found"
    per_tile = 256 // int(bm2.group(1))      # workgroups of the two-stage ring per 64-column tile: the issue's `2 * NT > 512`
    assert per_tile == 2
    assert re.search(r"active_tiles\(w\.L\)\s*>\s*diet_min_tiles\(\)", gemm) and re.search(r"tiles\s*<=\s*small_nt3", gemm)

    tiles = {}
    for purpose, b, n2, stated, precisions in R.FORM_CASES:
        t = R.launch_tiles(b, R.FORM_N1, n2)
        assert t == stated == b * ((R.FORM_N1 + 127) // 128 * 128 + (n2 + 127) // 128 * 128) // 64, purpose
        for prec in precisions:
            tiles.setdefault(prec, set()).add(t)
            if b > 1:
                tiles.setdefault(prec + " batched", set()).add(t)

    def straddled(prec, large):
        sides = {bool(large(t)) for t in tiles[prec]}
        return sides == {False, True}

    assert straddled("fp32", lambda t: t > diet), "qkv_kv / mlp0 fp32: two-half fragment loop and register-diet form"
    assert straddled("fp32", lambda t: not t <= small3), "mlp3 fp32: Mlp3TileS and Mlp3TileTallW8"
    assert straddled("fp32 batched", lambda t: t > diet) and straddled("fp32 batched", lambda t: not t <= small3)
    for prec in ("fp16x4", "fp16x3"):
        assert straddled(prec, lambda t: wide_min <= t // 2 <= wide_max), f"{prec} mlp0: narrow and wide tile"
        assert straddled(prec, lambda t: per_tile * t > ring), f"{prec} mlp3: three- and two-stage ring"
    # fp16x4 additionally sits on both edges of the wide window, from inside and from outside
    t4 = tiles["fp16x4"]
    assert {2 * wide_min - 2, 2 * wide_min, 2 * wide_max, 2 * wide_max + 2} <= t4
    assert {ring // per_tile, ring // per_tile + 2} <= t4
    # the small attention shapes all stay on the small side of every threshold
    for n1, n2 in R.ATTN_EDGE_SHAPES:
        for b in R.ATTN_B:
            t = R.launch_tiles(b, n1, n2)
            assert t <= min(diet, small3) and t // 2 < wide_min


@pytest.mark.parametrize("n1,n2", R.ATTN_EDGE_SHAPES)
def test_attention_edge_shapes_are_well_conditioned(sd, n1, n2):
    """InstanceNorm over a handful of points can amplify rounding by orders of magnitude; a shape where the fp32 restatement
    itself is off by more than 1e-3 of the largest delta entry proves nothing about a kernel."""
    for b in R.ATTN_B:
        x, y = R.attention_inputs(b, n1, n2)
        for kind, p in (("self", "gnn.layers.1"), ("cross", "gnn.layers.2")):
            d64 = R.attention_layer_deltas(sd, p, x, y, kind, np.float64)
            d32 = R.attention_layer_deltas(sd, p, x, y, kind, np.float32)
            for side in (0, 1):
                e32, dmax = maxdiff(d32[side], d64[side]), float(np.abs(d64[side]).max())
                assert e32 <= 1e-3 * dmax, (b, kind, side, e32, dmax)


@pytest.mark.parametrize("n1,n2", R.SCORE_SHAPES)
def test_score_cases_reach_conf_of_order_one_with_few_near_ties(sd, n1, n2):
    """The planted score cases: conf reaches O(1); at most 1 % of the rows and of the columns of the float64 conf have a top-2
    relative gap below TIE_GAP['fp32'] (they are exempt from the match comparison); a row above the gap points at a column above
    it and the other way round (so that its match does not hinge on an exempt arg-max); and the float32 restatement gives the
    float64 matches on all of them."""
    tie = TIE_GAP["fp32"]
    for b in R.SCORE_B:
        x, y = R.score_inputs(b, n1, n2)
        for scale in R.SCORE_SCALES:
            _, _, c64 = R.score_reference(sd, x, y, scale, np.float64)
            _, _, c32 = R.score_reference(sd, x, y, scale, np.float32)
            assert c64.max() > 0.9
            rows_ok, cols_ok = R.top2_rel_gap(c64, 2) >= tie, R.top2_rel_gap(c64, 1) >= tie
            assert (~rows_ok).mean() <= 0.01 and (~cols_ok).mean() <= 0.01
            idx0, idx1 = c64.argmax(axis=2), c64.argmax(axis=1)
            assert np.take_along_axis(cols_ok, idx0, axis=1)[rows_ok].all()
            assert np.take_along_axis(rows_ok, idx1, axis=1)[cols_ok].all()
            (a0, a1), (r0, r1) = R.mutual_matches(c32), R.mutual_matches(c64)
            assert np.array_equal(a0[rows_ok], r0[rows_ok]) and np.array_equal(a1[cols_ok], r1[cols_ok])
            assert (r0 >= 0).any()
