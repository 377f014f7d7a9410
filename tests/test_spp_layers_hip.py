"""The SuperPoint dense stack layer by layer (``spp_dense_stage``, include/superpoint.h) against the float64 chain of
tests/spp_layer_reference.py, in both arithmetics, always from a POISONED workspace: every byte 0xFF (NaN as fp32, NaN as fp16)
before every call, into an output that is NaN-filled too.  The library promises to work in any caller-provided workspace: a pad
ring nobody zeroed, a pad column a flat kernel did not overwrite or a tail a kernel reads puts a NaN into the accumulator of a
border pixel of the NEXT stage.  Behind a ReLU that pixel reads 0 (fmaxf(NaN, 0) is 0: measured with `b3` left out of the ring
zeroing, e_hip = s from stage 5 on and not one NaN), so the ring check is the error bound there and "finite everywhere" at the
logits and descriptors.

Per stage: e_hip <= 4 e_ref + 4 eps_fp32 s (DESIGN section 13 restated for fp32 outputs), with e_hip = max |HIP - chain64|,
e_ref = max |yardstick - chain64|, s = max |chain64|; the yardstick is the sequential-k fp32 chain for ``fp32`` and its two-term
fp16 form (with the fused first layer the shape implies) for ``fp16x4``.  The three numbers are printed per stage.

The walk case (4 x 136 x 512: the persistent kernels take a second, third ... item per workgroup in the first layer, conv2a and
conv2b) runs stages 1 .. 5.  Its yardstick is the torch-backend sequential-k chain of ALL FOUR images (10 s per arithmetic on 8
CPU threads, bitwise the numpy form: tests/test_spp_layer_reference.py), not a restriction to images 0 and 3.  The conv3a walk
(two items per patch) needs more than 512 k pixels and stays with tests/test_spp_hip_parity.py's 4 x 512 x 512 test.  Its score
map is checked for being finite, its descriptors for being stage 10 bit for bit; the comparison with the numpy oracle's score map
is left to the other cases (four encoder evaluations of the oracle take 26 s there, and at 278 k pixels two fp32 evaluations
of a softmax over logits up to 20 are themselves up to 1.1e-5 apart: measured |HIP - float64| 1.04e-5, |oracle - float64| 3.4e-6).

Measured on the MI355X, e_hip / e_ref over the eight cases: fp32 0.66 .. 1.71 (stage 0: 1.00, bit for bit the fma chain),
fp16x4 0.55 .. 1.44; the largest e_hip / bound is 0.35 (fp32, 2 x 8 x 256, stage 5) and 0.29 (fp16x4, 2 x 8 x 256, stage 1).
The whole file takes 12 s, 6 s of it on the two walk-case yardsticks (16 CPU threads).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import spp_layer_reference as R  # noqa: E402
from onepose_amd import _native_spp  # noqa: E402
from oracle import superpoint_oracle as so  # noqa: E402

ATOL_SCORE = 1e-5                       # tests/test_spp_hip_parity.py
BATCH_STAGES = (1, 3, 5, 7, 10)         # one per kernel family
PARAMS = [pytest.param(c, p, id=f"{R.case_id(c)}-{p}") for c in R.CASES for p in R.PRECISIONS]
BATCHED = [pytest.param(c, p, id=f"{R.case_id(c)}-{p}") for c in R.CASES if c[0] > 1 for p in R.PRECISIONS]


@functools.lru_cache(maxsize=None)
def module(precision):
    from onepose_amd import SuperPoint
    m = SuperPoint({}, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.weights().items()}, strict=True)
    return m.cuda().eval()


@functools.lru_cache(maxsize=4)
def workspace(b, h, w):
    nbytes = _native_spp.load().spp_workspace_bytes(b, h, w)
    assert nbytes > 0
    return torch.empty(nbytes, device="cuda", dtype=torch.uint8)


def poisoned(b, h, w):
    ws = workspace(b, h, w)
    ws.fill_(0xFF)
    return ws


def run_stage(precision, img, stage):
    """``stage`` of ``img`` [b, 1, H, W] (device) from a poisoned workspace into a NaN-filled output."""
    b, _, h, w = img.shape
    c, k = _native_spp.DENSE_STAGES[stage]
    out = torch.full((b, c, h >> k, w >> k), float("nan"), device="cuda", dtype=torch.float32)
    return module(precision).engine.dense_stage(img, stage, workspace=poisoned(b, h, w), out=out)


@functools.lru_cache(maxsize=None)
def device_images(case):
    return torch.from_numpy(R.images(case)).cuda()


@functools.lru_cache(maxsize=None)
def hip_stages(case, precision):
    return {s: run_stage(precision, device_images(case), s) for s in R.stages_of(case, precision)}


@pytest.mark.parametrize("case,precision", PARAMS)
def test_every_stage_is_finite_and_within_four_times_the_yardstick(case, precision):
    got = hip_stages(case, precision)
    bad = []
    for stage, t in got.items():
        out = t.cpu().numpy()
        finite = bool(np.isfinite(out).all())
        e_hip, e_ref, s = R.errors(out, case, stage, precision)          # e_hip is NaN where the output is not finite
        limit = R.bound(e_ref, s)
        print(f"{R.case_id(case)} {precision} stage {stage:2d} {R.STAGE_NAMES[stage]:20s}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  s {s:.3e}  "
              f"e_hip/e_ref {e_hip / e_ref:.2f}  bound {limit:.3e}")
        if not finite:
            where = np.argwhere(~np.isfinite(out))
            bad.append(f"stage {stage}: {len(where)} non-finite values, first at (image, channel, y, x) = {where[0].tolist()}")
        elif not e_hip <= limit:
            bad.append(f"stage {stage}: e_hip {e_hip:.3e} > 4 * {e_ref:.3e} + 4 eps * {s:.3e} = {limit:.3e}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("case,precision", PARAMS)
def test_stage_10_is_spp_dense_and_its_score_map_survives_the_poison(case, precision):
    b, h, w = case
    img = device_images(case)
    score, dense = module(precision).engine.dense(img, workspace=poisoned(b, h, w))
    d10 = hip_stages(case, precision)[10] if 10 in R.stages_of(case, precision) else run_stage(precision, img, 10)
    assert torch.equal(dense, d10)
    score = score.cpu().numpy()
    assert np.isfinite(score).all() and np.isfinite(dense.cpu().numpy()).all()
    if case == R.WALK_CASE:             # runs stages 1 .. 5 (module docstring); the bitwise and finite parts above cost nothing
        return
    sd = R.weights()
    for i in range(b):
        np.testing.assert_allclose(score[i], so.score_map(sd, so.encoder(sd, R.images(case)[i, 0])), atol=ATOL_SCORE)


@pytest.mark.parametrize("case,precision", BATCHED)
def test_an_image_alone_gives_the_same_bits(case, precision):
    got = hip_stages(case, precision)
    stages = [s for s in BATCH_STAGES if s in got]
    assert len(stages) >= 3
    img = device_images(case)
    for i in range(case[0]):
        for s in stages:
            alone = run_stage(precision, img[i:i + 1].contiguous(), s)
            assert torch.equal(alone[0], got[s][i]), f"image {i}, stage {s}: {int((alone[0] != got[s][i]).sum())} values differ"


@pytest.mark.parametrize("case,precision", PARAMS)
def test_two_runs_in_a_repoisoned_workspace_are_bitwise_equal(case, precision):
    for s, first in hip_stages(case, precision).items():
        again = run_stage(precision, device_images(case), s)
        assert torch.equal(first, again), f"stage {s}: {int((first != again).sum())} values differ"


def test_refusals():
    from onepose_amd._native import NativeError
    img = device_images((1, 8, 8))
    with pytest.raises(NativeError, match="does not exist in this configuration"):
        run_stage("fp16x4", img, 0)                                # even H: conv1a's plane is never written
    assert torch.isfinite(run_stage("fp16x4", device_images((1, 15, 9)), 0)).all()     # odd H: it is
    eng = module("fp32").engine
    c, _ = _native_spp.DENSE_STAGES[0]
    out = torch.empty(1, c, 8, 8, device="cuda")
    for stage in (-1, 11):
        with pytest.raises(NativeError, match="stage must be in"):
            eng.call("spp_dense_stage", img.device, eng.packed_weights(img.device), img, 1, 8, 8, stage, out, workspace(1, 8, 8),
                     workspace(1, 8, 8).numel(), 0)
    with pytest.raises(NativeError, match="workspace too small"):
        eng.call("spp_dense_stage", img.device, eng.packed_weights(img.device), img, 1, 8, 8, 0, out, workspace(1, 8, 8), 16, 0)
    with pytest.raises(NativeError, match="unknown bits"):
        eng.call("spp_dense_stage", img.device, eng.packed_weights(img.device), img, 1, 8, 8, 0, out, workspace(1, 8, 8),
                 workspace(1, 8, 8).numel(), 0x1)
