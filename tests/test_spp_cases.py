"""Every generated case of the extractor head's edge tests (tests/test_spp_detect_edges.py) meets the conditions of tests/spp_cases.py:
what keeps those exact comparisons aimed at the paths they are meant for.  No GPU needed."""
import numpy as np
import pytest

import spp_cases as sc
from oracle import superpoint_oracle as so


def assert_conditions(case, what):
    assert case["conditions"], what
    failed = [name for name, ok in case["conditions"] if not ok]
    assert not failed, f"{what}: {failed}"


def test_tile_sizes_are_the_kernels():
    assert [sc.tile(r) for r in sc.RADII] == [32, 32, 32, 24, 14, 4]


@pytest.mark.parametrize("radius", sc.RADII)
def test_chain_cases_meet_the_conditions(radius):
    c = sc.chain_case(radius)
    assert_conditions(c, f"chains, R = {radius}")
    n = len(c["score"])
    assert n == 2 * len(c["specs"]) == 2 * (3 * 5 * radius + 6) and c["score"].shape[1:] == (sc.CHAIN_H, sc.CHAIN_W)
    for j in range(0, n, 2):
        full, twin, pts = c["score"][j], c["score"][j + 1], c["points"][j]
        assert int((full != 0).sum()) == 8 and int((twin != 0).sum()) == 7
        assert full[pts[0]] == np.float32(0.9) and twin[pts[0]] == 0 and np.array_equal(np.delete(full.ravel(), pts[0][0] * sc.CHAIN_W + pts[0][1]),
                                                                                         np.delete(twin.ravel(), pts[0][0] * sc.CHAIN_W + pts[0][1]))
        # the fate of peak 5 is decided by peak 0, five radii away along the chain
        assert max(abs(pts[5][0] - pts[0][0]), abs(pts[5][1] - pts[0][1])) == 5 * radius
        assert c["nms"][j][pts[5]] == 0 and c["nms"][j + 1][pts[5]] == sc.CHAIN_PEAKS[5]
        for i, yx in enumerate(c["yx"][j:j + 2]):
            assert sorted(map(tuple, yx.tolist())) == sorted(pts[q] for q in c["kept"][j + i])


@pytest.mark.parametrize("radius", sc.RADII)
@pytest.mark.parametrize("shape", sc.QUANT_SHAPES)
@pytest.mark.parametrize("levels", sc.QUANT_LEVELS)
def test_quantised_cases_meet_the_conditions(levels, shape, radius):
    c = sc.quant_case(levels, shape, radius)
    assert_conditions(c, f"L = {levels}, {shape}, R = {radius}")
    assert c["score"].shape == (2,) + shape and c["score"].min() > 0 and len(np.unique(c["score"])) <= levels
    assert all(len(yx) > 0 for yx in c["yx"])


def test_the_restated_nms_trace_is_the_oracles():
    s = sc.quant_case(256, (72, 104), 3)["score"][0]
    nms, added = sc.nms_trace(s, 3)
    assert np.array_equal(nms, so.simple_nms(s, 3)) and len(added) == 2
    lone = np.zeros((16, 16), np.float32)
    lone[8, 8] = 1
    assert sc.nms_trace(lone, 2)[1] == [0, 0] and not sc.has_plateau(so.simple_nms(lone, 2))


def test_radius0_case_meets_the_conditions():
    c = sc.radius0_case()
    assert_conditions(c, "R = 0")
    assert np.array_equal(c["nms"].view(np.uint32), c["score"].view(np.uint32))


@pytest.mark.parametrize("border", sc.SCAN_BORDERS)
@pytest.mark.parametrize("shape", sc.SCAN_SHAPES)
def test_row_scan_cases_meet_the_conditions(shape, border):
    c = sc.scan_case(shape, border)
    assert_conditions(c, f"{shape}, border {border}")
    assert c["score"].shape == (2,) + shape and (shape[0] + 1023) // 1024 == {1032: 2, 2056: 3, 8: 1}[shape[0]]
    assert c["capacity"] > max(c["ncand"]) and [len(s) for s in c["sc"]] == c["ncand"]
    assert set(np.unique(c["score"]).tolist()) == {0.0, 0.125, 0.25, 0.375, 0.5}
    for yx in c["yx"]:
        assert yx[:, 0].min() >= border and yx[:, 0].max() < shape[0] - border and yx[:, 1].min() >= border and yx[:, 1].max() < shape[1] - border


def test_border_and_truncation_cases_meet_the_conditions():
    for border in (8, 12):
        assert_conditions(sc.border_case(border), f"border {border}")
    c = sc.truncation_case()
    assert_conditions(c, "truncation")
    assert c["ncand"][0] <= sc.TRUNC_CAPACITY < c["ncand"][1]


@pytest.mark.parametrize("kind", sc.TOPK_KINDS)
def test_topk_cases_meet_the_conditions(kind):
    for k in sc.TOPK_K:
        c = sc.topk_case(kind, k)
        assert_conditions(c, f"{kind}, k = {k}")
        assert c["ncand"] == [4096] and len(c["sc"][0]) == k and (np.diff(c["sc"][0]) <= 0).all()
        if kind == "low":
            assert c["ties"] > c["kept"] >= 1
            cut = c["sc"][0][-1]                           # the kept ties are the lowest pixel indices among the candidates equal to the cut
            tied = np.nonzero(c["score"].ravel() == cut)[0][:c["kept"]]
            kept = c["yx"][0][c["sc"][0] == cut]
            assert np.array_equal(kept[:, 0] * 64 + kept[:, 1], tied)


def test_all_equal_and_quota_cases_meet_the_conditions():
    for k in sc.ALL_EQUAL_K:
        assert_conditions(sc.all_equal_case(k), f"all equal, k = {k}")
    quotas = {}
    for kind in sc.QUOTA_KINDS:
        c = sc.quota_case(kind)
        assert_conditions(c, kind)
        quotas[kind] = (c["quota"], c["ties"])
    assert quotas["across_chunks"] == (1500, 3996) and quotas["all_ties"][0] == quotas["all_ties"][1] > 1024


def test_mixed_batch_case_meets_the_conditions():
    assert_conditions(sc.mixed_batch_case(), "mixed batch")


@pytest.mark.parametrize("k", sc.LARGE_K)
def test_large_k_cases_meet_the_conditions(k):
    c = sc.large_case(k)
    assert_conditions(c, f"k = {k}")
    assert len(c["sc"][0]) == k and len(np.unique(c["sc"][0])) < k


def test_reuse_sequence_returns_to_its_first_configuration():
    seq = sc.REUSE_SEQUENCE
    assert seq[0] == seq[-1] == 3000 and -1 in seq and min(q for q in seq if q > 0) == 10
    for k in seq:
        assert_conditions(sc.reuse_case(k), f"reuse, k = {k}")
    assert sc.reuse_case(seq[0]) is sc.reuse_case(seq[-1])


@pytest.mark.parametrize("align_corners", [True, False])
@pytest.mark.parametrize("shape", sc.DESC_SHAPES)
def test_descriptor_cases_meet_the_conditions(shape, align_corners):
    c = sc.descriptor_case(shape, align_corners)
    assert_conditions(c, f"{shape}, align_corners = {align_corners}")
    assert c["capacity"] > len(c["kp"]) and all(s.tolist() == [1.0] * len(c["kp"]) for s in c["sc"])
    for r64, r32 in zip(c["ref64"], c["ref32"]):
        assert r64.dtype == np.float64 and r32.dtype == np.float32
        bound = sc.descriptor_bound(r64, r32)
        assert bound.shape == (len(c["kp"]),) and (bound >= 4 * sc.ULP32).all() and bound.max() < 2e-6     # the rule stays far below the old flat 2e-6
        live = np.abs(r64).max(axis=0) > 0
        np.testing.assert_allclose(np.linalg.norm(r64[:, live], axis=0), 1.0, atol=1e-12)


def test_the_reference_sampler_follows_the_oracle_on_ordinary_descriptors():
    """sample_reference in fp32 against so.sample_descriptors on so-normalised standard-normal descriptors, both align modes, bit for bit;
    in fp64 within fp32 rounding of it."""
    raw = sc.dense_normal(1, 5, 9)[0]
    dense = (raw / np.maximum(np.sqrt((raw ** 2).sum(axis=0, keepdims=True)), np.float32(1e-12))).astype(np.float32)
    kp = np.random.RandomState(2).randint(0, [72, 40], (50, 2)).astype(np.float32)
    for align in (True, False):
        want = so.sample_descriptors(kp, dense, 8, align)
        assert np.array_equal(sc.sample_reference(kp, raw, align, np.float32)[0], want)
        np.testing.assert_allclose(sc.sample_reference(kp, raw, align, np.float64)[0], want, atol=1e-6)
