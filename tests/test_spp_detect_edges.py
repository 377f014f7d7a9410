"""The extractor head (spp_detect_kernels.hip: NMS, threshold / border, row scan, compaction, radix top-k, rank, scatter, descriptor
sampling) on constructed score maps and dense descriptors, through spp_detect, against oracle/superpoint_oracle.py.  The cases and what
each reaches are in tests/spp_cases.py; tests/test_spp_cases.py asserts their conditions on the CPU.  Every discrete output -- the NMS
map, both counts, the keypoints with their order, the scores -- is compared by equality.  Descriptors: |HIP - fp64| <= 4 x |fp32 oracle -
fp64| + 4 ulps of fp32, per keypoint (DESIGN 13's rule).  The module's weights are never read: spp_detect takes the dense tensors."""
import numpy as np
import pytest
import torch

import spp_cases as sc
from onepose_amd import SuperPoint

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def mod():
    return SuperPoint({}).to(DEV).eval()


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def detect(mod, score, dense, cfg, align=True, capacity=None):
    """spp_detect into outputs that start out dirty -> numpy (keypoints, scores, descriptors, counts, nms)."""
    out = mod.engine.detect(gpu(score), gpu(dense), cfg, align, capacity=capacity, return_nms=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def run_case(mod, c, capacity=None, lo=0, hi=None, dense=None, align=True):
    """Images lo .. hi of a case through one call, every discrete output against the oracle's.  -> the call's outputs."""
    score = c["score"][lo:hi]
    b, h, w = score.shape
    dense = sc.dense_normal(b, h // 8, w // 8) if dense is None else dense
    if capacity is None and c["cfg"]["max_keypoints"] < 0:
        capacity = max(c["ncand"][lo:hi]) + 5                       # room for all, and no multiple of the sampler's 16
    kp, scores, desc, counts, nms = detect(mod, score, dense, c["cfg"], align, capacity)
    np.testing.assert_array_equal(nms.view(np.uint32), c["nms"][lo:hi].view(np.uint32))
    for i in range(b):
        yx, want, ncand = c["yx"][lo + i], c["sc"][lo + i], c["ncand"][lo + i]
        n = len(yx) if c["cfg"]["max_keypoints"] >= 0 else min(len(yx), capacity)
        assert counts[i].tolist() == [n, ncand], f"image {lo + i}: counts {counts[i].tolist()}, expected {[n, ncand]}"
        np.testing.assert_array_equal(kp[i, :n], yx[:n, ::-1].astype(np.float32), err_msg=f"image {lo + i}")
        np.testing.assert_array_equal(scores[i, :n], want[:n], err_msg=f"image {lo + i}")
        if n:
            np.testing.assert_allclose(np.linalg.norm(desc[i][:, :n], axis=0), 1.0, atol=1e-5)
    return kp, scores, desc, counts, nms


# ---- A  NMS ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", sc.RADII)
def test_nms_chains_reach_five_radii(mod, radius):
    """Eight peaks at spacing R, along a row, a column and the diagonal, peak 0 at every distance 1 .. 5 R before a tile boundary and on
    the image's first / last row and column: the map keeps peaks 0, 2, 4, its twin without peak 0 keeps 1, 3, 5 -- the fate of peak 5 is
    decided five radii away, in another tile."""
    c = sc.chain_case(radius)
    for lo in range(0, len(c["score"]), sc.CHAIN_BATCH):
        hi = min(lo + sc.CHAIN_BATCH, len(c["score"]))
        *_, nms = run_case(mod, c, lo=lo, hi=hi)
        for j in range(lo, hi):
            on = {i for i, yx in enumerate(c["points"][j]) if nms[j - lo][yx] != 0}
            assert on == ({0, 2, 4}, {1, 3, 5})[j % 2], (c["specs"][j // 2], j % 2, on)


@pytest.mark.parametrize("radius", sc.RADII)
@pytest.mark.parametrize("shape", sc.QUANT_SHAPES)
@pytest.mark.parametrize("levels", sc.QUANT_LEVELS)
def test_nms_quantised_maps(mod, levels, shape, radius):
    """Maps of 16 / 256 levels: equal floats in every window, plateaus, both suppression rounds at work, survivors on the tile edges."""
    run_case(mod, sc.quant_case(levels, shape, radius))


def test_nms_radius0_is_a_bitwise_copy(mod):
    run_case(mod, sc.radius0_case(), capacity=40 * 72)


# ---- B  threshold, border, row scan, compaction ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", sc.SCAN_BORDERS)
@pytest.mark.parametrize("shape", sc.SCAN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_scan_over_tall_and_wide_maps(mod, shape, border):
    """1032 / 2056 rows: a thread of rowscan_kernel owns 2 / 3 consecutive rows; 1032 columns: 17 chunks per row.  Scores equal to the
    threshold survive the NMS and are not kept."""
    c = sc.scan_case(shape, border)
    _, scores, _, counts, _ = run_case(mod, c, capacity=c["capacity"])
    for i in range(2):
        assert (scores[i, :counts[i, 0]] > np.float32(sc.SCAN_THRESHOLD)).all()


@pytest.mark.parametrize("border", [8, 12])
def test_border_at_least_half_the_height_keeps_nothing(mod, border):
    *_, counts, _ = run_case(mod, sc.border_case(border), capacity=16)
    assert counts.tolist() == [[0, 0], [0, 0]]


def test_truncation_of_one_image_of_a_batch(mod):
    c = sc.truncation_case()
    kp, _, _, counts, _ = run_case(mod, c, capacity=sc.TRUNC_CAPACITY)
    assert counts.tolist() == [[c["ncand"][0]] * 2, [sc.TRUNC_CAPACITY, c["ncand"][1]]]
    pix = kp[1][:, 1] * 32 + kp[1][:, 0]
    assert (np.diff(pix) > 0).all()


# ---- C  top-k -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sc.TOPK_K)
@pytest.mark.parametrize("kind", sc.TOPK_KINDS)
def test_radix_select_digit_by_digit(mod, kind, k):
    """4096 candidates whose scores differ in the low, the middle or the top radix digit only; k at 1, around the 1024-candidate chunk,
    and one short of everything.  `low`: the cut score is shared by more candidates than are kept."""
    run_case(mod, sc.topk_case(kind, k))


@pytest.mark.parametrize("k", sc.ALL_EQUAL_K)
def test_all_equal_scores_keep_the_first_k_pixels(mod, k):
    kp, *_ = run_case(mod, sc.all_equal_case(k))
    np.testing.assert_array_equal(kp[0, :k, 1] * 64 + kp[0, :k, 0], np.arange(k))


@pytest.mark.parametrize("kind", sc.QUOTA_KINDS)
def test_tie_quota_across_chunks(mod, kind):
    """A quota of 1500 of 3996 ties (carried over the 1024-candidate chunks), and a quota that takes every tie."""
    run_case(mod, sc.quota_case(kind))


@pytest.mark.parametrize("capacity", sc.MIXED_CAPACITIES)
def test_mixed_batch_at_the_edges_of_engagement(mod, capacity):
    """One call: an image without candidates, one with exactly k (kept in row-major order), one with k + 1 (sorted, one dropped)."""
    c = sc.mixed_batch_case()
    *_, counts, _ = run_case(mod, c, capacity=capacity)
    assert counts.tolist() == [[0, 0], [sc.MIXED_K, sc.MIXED_K], [sc.MIXED_K, sc.MIXED_K + 1]]


@pytest.mark.parametrize("k", sc.LARGE_K)
def test_rank_kernel_second_trips(mod, k):
    """k above 4096 (a second trip over j) and above 16384 (over i), equal scores far apart among the survivors."""
    run_case(mod, sc.large_case(k), capacity=k)


def test_workspace_reuse_across_configurations(mod):
    """One module, one shape: k = 3000, keep-all, k = 10, k = 3000 -- each the oracle's, the first and the last bitwise equal."""
    outs = []
    for k in sc.REUSE_SEQUENCE:
        outs.append(run_case(mod, sc.reuse_case(k), capacity=4096))
    first, last = outs[0], outs[-1]
    for a, b in zip(first[:2], last[:2]):
        assert np.array_equal(a[:, :3000].view(np.uint32), b[:, :3000].view(np.uint32))
    assert np.array_equal(first[2][:, :, :3000].view(np.uint32), last[2][:, :, :3000].view(np.uint32))


# ---- D  descriptor sampling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align_corners", [True, False], ids=["align", "noalign"])
@pytest.mark.parametrize("shape", sc.DESC_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_descriptors_at_corners_edges_and_special_cells(mod, shape, align_corners):
    """Keypoints on the corners, the edge midpoints, both sides of a cell centre and inside; one all-zero cell, one scaled by 1e15; maps
    of one cell, one row and one column of cells.  Per keypoint |HIP - fp64| <= 4 |fp32 oracle - fp64| + 4 ulps; a keypoint whose taps
    all lie in the zero cell (or outside the map) has an exactly zero descriptor.

    Measured on the MI355X: worst |HIP - fp64| / bound 0.058 (8x64-align, image 1, keypoint (3, 0): 3.0e-8, fp32 oracle 1.1e-8); largest
    |HIP - fp64| of any case 3.0e-8, the fp32 oracle's 9.3e-8.  Before contraction was switched off in sample_kernel's align_corners = 0
    arm, 40x72-noalign failed: 8.3e-7 at keypoint (67, 35) of image 1, 1.53 x the bound (fp32 oracle 1.7e-8); after, 0.047 x at worst."""
    c = sc.descriptor_case(shape, align_corners)
    n = len(c["kp"])
    score, dense = c["score"], c["dense"]
    kp, scores, desc, counts, nms = detect(mod, score, dense, c["cfg"], align_corners, c["capacity"])
    np.testing.assert_array_equal(nms, c["nms"])
    worst = 0.0
    for i in range(2):
        assert counts[i].tolist() == [n, n]
        np.testing.assert_array_equal(kp[i, :n], c["kp"])
        np.testing.assert_array_equal(scores[i, :n], np.ones(n, np.float32))
        got = desc[i][:, :n]
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - c["ref64"][i]).max(axis=0)
        e32 = np.abs(c["ref32"][i].astype(np.float64) - c["ref64"][i]).max(axis=0)
        bound = sc.descriptor_bound(c["ref64"][i], c["ref32"][i])
        j = int(np.argmax(err / bound))
        print(f"\n{shape[0]}x{shape[1]} align_corners={int(align_corners)} image {i}: worst |HIP - fp64| / bound {err[j] / bound[j]:.3f} at keypoint "
              f"({int(c['kp'][j, 0])}, {int(c['kp'][j, 1])}) (HIP {err[j]:.3e}, fp32 oracle {e32[j]:.3e}); max |HIP - fp64| {err.max():.3e}, "
              f"max |fp32 oracle - fp64| {e32.max():.3e}, worst HIP / max(fp32 oracle, 4 ulps) {(err / np.maximum(e32, 4 * sc.ULP32)).max():.3f}")
        worst = max(worst, float((err / bound).max()))
        zero = c["zero_kp"][i]
        assert not got[:, zero].any(), "a keypoint with every tap in the zero cell must have an exactly zero descriptor"
        assert (err <= bound).all(), (f"image {i}: keypoints {np.nonzero(err > bound)[0].tolist()} exceed the bound: |HIP - fp64| {err[err > bound]}, "
                                      f"bound {bound[err > bound]}")
    assert worst <= 1.0
