"""The per-layer references of tests/spp_layer_reference.py against each other and against the numpy oracle, and the path
conditions of its cases against the launch code.  No GPU.  The walk case (4 x 136 x 512) is held to its path conditions here; its
float64 chain and yardsticks (seconds of CPU time) are evaluated by the GPU test that needs them."""
import os
import re

import numpy as np
import pytest

import spp_layer_reference as R
from oracle import superpoint_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in R.CASES if c != R.WALK_CASE]
CAP_ULPS = 64          # sanity cap on a yardstick's own error, in fp32 ulps of the plane's scale (measured: 1.1 .. 17)
ATOL_SCORE = 1e-5      # tests/test_spp_hip_parity.py


def ids(cases):
    return [R.case_id(c) for c in cases]


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_chain64_agrees_with_the_numpy_oracle(case):
    sd, ref = R.weights(), R.reference(case)
    for i, im in enumerate(R.images(case)):
        feat = so.encoder(sd, im[0])
        s = np.abs(ref[7][i]).max()
        assert np.abs(feat - ref[7][i]).max() <= CAP_ULPS * R.EPS32 * s
        lg = ref[9][i]
        e = np.exp(lg - lg.max(axis=0, keepdims=True))
        p = (e / e.sum(axis=0, keepdims=True))[:-1]
        h, w = p.shape[1:]
        sm = p.transpose(1, 2, 0).reshape(h, w, 8, 8).transpose(0, 2, 1, 3).reshape(h * 8, w * 8)
        np.testing.assert_allclose(so.score_map(sd, feat), sm, atol=ATOL_SCORE)
        raw = so.conv2d(so.relu(so.conv2d(feat, sd["convDa.weight"], sd["convDa.bias"])), sd["convDb.weight"], sd["convDb.bias"])
        assert np.abs(raw - ref[10][i]).max() <= CAP_ULPS * R.EPS32 * np.abs(ref[10][i]).max()


@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_yardstick_errors_are_nonzero_and_small(case, precision):
    """A yardstick that equals float64 measures nothing, one that is far from it is wrong."""
    for stage in range(R.NSTAGES):
        _, e_ref, s = R.errors(R.yardstick(case, precision)[stage], case, stage, precision)
        print(f"{R.case_id(case)} {precision} stage {stage} {R.STAGE_NAMES[stage]}: e_ref {e_ref:.3e} = {e_ref / (R.EPS32 * s):.2f} ulps of {s:.3f}")
        assert 0.0 < e_ref <= CAP_ULPS * R.EPS32 * s


def test_fused_first_layer_differs_from_the_direct_one():
    """The two first-layer arithmetics are different functions: fused_first must matter to the yardstick."""
    sd, img = R.weights(), R.images((1, 8, 8))[0, 0]
    a, b = R.chain16x4_seq(sd, img, True)[0], R.chain16x4_seq(sd, img, False)[0]
    assert not np.array_equal(a, b) and np.abs(a - b).max() < 1e-5
    np.testing.assert_array_equal(b, R.chain32_seq(sd, img)[0])


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_two_term_split_reproduces_its_operands(case):
    """2^-22 relative, or 2^-25 absolute where the second term is subnormal; both terms are fp16 values within +-65504."""
    operands = [v for v in R.weights().values()] + [R.images(case)] + R.yardstick(case, "fp16x4")[:9]
    for x in operands:
        hi, lo = R.fp16_split(x)
        for t in (hi, lo):
            assert np.array_equal(t, t.astype(np.float16).astype(np.float32)) and np.abs(t).max() <= 65504
        two = R.two_term(x)
        assert np.array_equal(two.astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64))     # hi + lo is exact in fp32
        err = np.abs(two.astype(np.float64) - np.asarray(x, np.float64))
        assert np.all(err <= np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -25))
    big = np.array([7e4, -1e9, 65504.0, 65519.0, 65520.0], np.float32)
    assert np.array_equal(R.fp16_split(big)[0], np.array([65504, -65504, 65504, 65504, 65504], np.float32))
    assert np.array_equal(R.fp16_split(np.array([3e-8, 2.0 ** -24], np.float32))[0], np.array([2.0 ** -24, 2.0 ** -24], np.float32))


def test_torch_backend_is_bitwise_the_numpy_one():
    """The walk case's yardstick runs on torch CPU tensors: same product, same addition, same order."""
    sd, img = R.weights(), R.images((1, 22, 126))[0, 0]
    for fused in (True, False):
        for a, b in zip(R.chain16x4_seq(sd, img, fused), R.chain16x4_seq(sd, img, fused, "torch")):
            assert np.array_equal(a, b)
    x = np.random.RandomState(0).standard_normal((64, 5, 40)).astype(np.float32)
    w, bias = sd["conv2a.weight"], sd["conv2a.bias"]
    ref = R.conv_seq(x, w, bias)
    old, R.BLOCK_COLUMNS = R.BLOCK_COLUMNS, 80           # blocks of two rows: blocking changes no bit
    try:
        assert np.array_equal(R.conv_seq(x, w, bias), ref) and np.array_equal(R.conv_seq(x, w, bias, "torch"), ref)
    finally:
        R.BLOCK_COLUMNS = old


def test_conv_seq_is_the_convolution():
    rs = np.random.RandomState(1)
    x = rs.standard_normal((64, 7, 9)).astype(np.float32)
    sd = R.weights()
    for name in ("conv2a", "convDb"):
        w, b = sd[name + ".weight"], sd[name + ".bias"]
        xx = x if w.shape[1] == 64 else rs.standard_normal((256, 3, 5)).astype(np.float32)
        np.testing.assert_allclose(R.conv_seq(xx, w, b), so.conv2d(xx, w, b), atol=2e-5)
    img = R.images((1, 15, 9))[0, 0]
    want = so.conv2d(img[None], sd["conv1a.weight"], sd["conv1a.bias"])
    np.testing.assert_allclose(R.conv1a_fma(img, sd["conv1a.weight"], sd["conv1a.bias"]), want, atol=1e-6)
    np.testing.assert_allclose(R.conv1a_split(img, sd["conv1a.weight"], sd["conv1a.bias"]), want, atol=1e-6)


# ---- the cases reach what they are there for ---------------------------------------------------------------------------------
def seg(w, n):
    return (w + n - 1) // n


def res(case):
    _, h, w = case
    return [(h >> k, w >> k) for k in (1, 2, 3)]


def test_launch_code_still_chooses_as_the_cases_assume():
    """The path conditions below restate launch_dense; if its rules or the tile table change, the cases must be looked at again."""
    with open(os.path.join(ROOT, "onepose_amd", "csrc", "spp_conv_kernels.hip")) as f:
        src = f.read()
    assert re.search(r"fits = \[\]\(const FeatLayout& L\) \{ return \(L\.H & 1\) == 0 && L\.W % 64 == 0; \}", src)
    assert re.search(r"return w\.prec == 4 && fuse_conv1\(\) && \(w\.L1\.H & 1\) == 0;", src)
    # tile ids conv1b .. convDb: 0 = 64 x 128 columns (64-pixel patch rows), 1 = 64 x 64 (32-pixel patch rows)
    assert re.search(r"static int tiles\[NGEMM\] = \{0, 0, 0, 1, 1, 1, 1, 1, 1, 1\};", src)
    assert re.search(r": 64;\s*$", [l for l in src.splitlines() if "SPP_C1_SLOTS" in l][0])           # 64 workgroups per XCD


def test_cases_meet_their_path_conditions():
    # one cell; every layer a single partial tile
    assert res((1, 8, 8)) == [(4, 4), (2, 2), (1, 1)]

    c = (3, 12, 130)
    (h2, w2), (h4, w4), (h8, w8) = res(c)
    assert (h2, w2) == (6, 65) and seg(w2, 64) == 2 and w2 % 64 == 1            # second 64-pixel segment: one pixel
    assert (h4, w4) == (3, 32) and h4 % 2 == 1 and seg(w4, 32) == 1 and w4 % 32 == 0   # patch row below the image; one full segment
    assert (h8, w8) == (1, 16) and c[0] == 3
    assert R.fused_first(c[1]) and not R.resident(h2, w2) and not R.resident(h4, w4)
    per = (c[0] * (c[1] // 2) * seg(c[2], 64) + 7) // 8
    assert any((i * (c[1] // 2) * seg(c[2], 64)) % per for i in range(1, c[0]))         # an image boundary inside an XCD band

    c = (1, 22, 126)
    (h2, w2), (h4, w4), (h8, w8) = res(c)
    assert (h2 % 2, h4 % 2) == (1, 1) and w2 == 63 and w4 == 31 and (h8, w8) == (2, 15)

    c = (2, 16, 264)
    (h2, w2), (h4, w4), (h8, w8) = res(c)
    assert (h2, w2) == (8, 132) and seg(w2, 64) == 3 and w2 % 64 == 4
    assert (h4, w4) == (4, 66) and seg(w4, 32) == 3 and w4 % 32 == 2
    assert (h8, w8) == (2, 33) and seg(w8, 32) == 2 and w8 % 32 == 1
    assert not R.resident(h2, w2) and not R.resident(h4, w4)

    c = (2, 8, 256)
    (h2, w2), (h4, w4), _ = res(c)
    assert R.fused_first(c[1]) and R.resident(h2, w2) and R.resident(h4, w4) and h4 // 2 == 1 and c[0] == 2

    c = (1, 18, 256)
    (h2, w2), (h4, w4), _ = res(c)
    assert R.fused_first(c[1]) and h2 % 2 == 1 and not R.resident(h2, w2) and R.resident(h4, w4)

    c = (1, 15, 9)
    assert not R.fused_first(c[1]) and 0 in R.stages_of(c, "fp16x4") and 0 in R.stages_of(c, "fp32")

    b, h, w = c = R.WALK_CASE
    (h2, w2), (h4, w4), _ = res(c)
    assert R.fused_first(h) and R.resident(h2, w2) and R.resident(h4, w4)
    per, slots = R.resident_walk(b, h, w)
    assert (per, slots) == (272, 64) and b * (h // 2) * seg(w, 64) == 2176       # first layer: every workgroup walks 4 - 5 items
    assert all((i * 136) % per for i in (1, 3))                                 # image boundaries 136 and 408 inside a band
    per, slots = R.resident_walk(b, h2, w2)
    assert (per, slots) == (68, 64)                                             # conv2a / conv2b: four workgroups per XCD take a second item
    per, slots = R.resident_walk(b, h4, w4, rows=128)
    assert per <= 64                                                            # conv3a (two items per patch) does not walk here
    assert R.stages_of(c, "fp16x4") == [1, 2, 3, 4, 5] == R.stages_of(c, "fp32")
    for case in SMALL:
        assert R.stages_of(case, "fp32") == list(range(11))
        assert R.stages_of(case, "fp16x4") == list(range(1 if case[1] % 2 == 0 else 0, 11))
