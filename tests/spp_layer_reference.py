"""Per-layer references of the SuperPoint dense stack (``spp_dense_stage``, include/superpoint.h), no GPU needed.

TEST INFRASTRUCTURE ONLY.  Three evaluations of the same eleven tensors (stage 0 .. 10 of ``spp_dense_stage``), one image at a time:

``chain64``        float64 (torch conv2d / max_pool2d on the CPU): what the others are measured against.
``chain32_seq``    the yardstick of the fp32 MFMA path: fp32, every GEMM convolution accumulated SEQUENTIALLY over k in the
                   kernels' order (k = tap * Cin + ci, tap = 3 (dy + 1) + (dx + 1); accumulator from zero, one rounded product
                   added per k, bias last).  An MFMA accumulator chain over K = 576 / 1152 is of this kind; the BLAS oracle
                   (oracle/superpoint_oracle.py: one blocked sgemm per tap) is up to 3x closer to float64 than any sequential
                   chain can be, so a bound built on it would refuse a correct kernel.  conv1a is the direct kernel's arithmetic:
                   accumulator = bias, then nine fused multiply-adds in tap order.
``chain16x4_seq``  the yardstick of ``precision="fp16x4"``, from the arithmetic superpoint.h documents: ``chain32_seq`` with every
                   GEMM-convolution operand replaced by its two-term value hi + lo, hi = RNE_fp16(x), lo = RNE_fp16(x - hi),
                   saturating at +-65504, subnormals kept (hi + lo is exact in fp32).  Weights are split once, activations as they
                   enter a layer; the GEMM bias stays fp32.  ``fused_first`` (even H): conv1a too runs on split pixels, split
                   weights and a split bias (the fused kernel's column of ones), accumulated from zero over the nine taps and then
                   the bias; otherwise conv1a is the fp32 FMA form above.

``backend="torch"`` evaluates the same rounded product and the same addition per k with torch CPU tensors (threads) instead of
numpy, for the one case numpy is too slow for; tests/test_spp_layer_reference.py holds the two to bitwise equality.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from onepose_amd import synthetic

F32 = np.float32
EPS32 = 2.0 ** -23
FP16_MAX = F32(65504.0)
STAGE_NAMES = ("relu(conv1a)", "pool(relu(conv1b))", "relu(conv2a)", "pool(relu(conv2b))", "relu(conv3a)", "pool(relu(conv3b))",
               "relu(conv4a)", "relu(conv4b)", "relu(convPa|convDa)", "logits", "descriptors")
NSTAGES = len(STAGE_NAMES)

# (b, H, W): the smallest shapes at which each tiling of spp_conv_kernels.hip can still go wrong (what each one reaches:
# PATHS below, asserted by tests/test_spp_layer_reference.py), and the one at which the persistent kernels walk
CASES = [(1, 8, 8), (3, 12, 130), (1, 22, 126), (2, 16, 264), (2, 8, 256), (1, 18, 256), (1, 15, 9), (4, 136, 512)]
WALK_CASE = (4, 136, 512)
WEIGHT_SEED = 3
PRECISIONS = ("fp32", "fp16x4")


def case_id(case):
    return "x".join(map(str, case))


def image_seed(case):
    b, h, w = case
    return 1000 * b + 7 * h + w


# ---- which kernels a shape reaches: a restatement of launch_dense's choices (spp_conv_kernels.hip) --------------------------
def fused_first(h):
    """fp16x4: conv1a is recomputed inside the fused first-layer kernel (even H)."""
    return h % 2 == 0


def resident(h, w):
    """fp16x4: the resident-block kernel takes a 64-input-channel 3x3 layer at resolution h x w (launch_dense's `fits`)."""
    return h % 2 == 0 and w % 64 == 0


def resident_walk(b, h, w, rows=64, slots=64):
    """(items per XCD band, workgroups per XCD) of the resident-block kernel: a workgroup takes a second item when the first
    exceeds the second."""
    items = b * (h // 2) * ((w + 63) // 64) * (rows // 64)
    per = (items + 7) // 8
    return per, min(per, slots)


def stages_of(case, precision):
    """The stages spp_dense_stage can export for this case (conv1a's plane does not exist under the fused first layer); the walk
    case stops at stage 5: the walking kernels end at stage 3 and stage 5 checks what they feed."""
    first = 1 if precision == "fp16x4" and fused_first(case[1]) else 0
    return list(range(max(first, 1), 6)) if case == WALK_CASE else list(range(first, NSTAGES))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights():
    return synthetic.make_spp_state_dict(WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def images(case):
    b, h, w = case
    return synthetic.make_image(b, h, w, image_seed(case))


# ---- float64 -----------------------------------------------------------------------------------------------------------------
def chain64(sd, img):
    """img [H, W] -> the eleven stage tensors in float64 (numpy)."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    conv = lambda x, n: torch.nn.functional.conv2d(x, t(sd[n + ".weight"]), t(sd[n + ".bias"]), padding=sd[n + ".weight"].shape[-1] // 2)  # noqa: E731
    relu, pool = torch.relu, lambda x: torch.nn.functional.max_pool2d(x, 2, 2)
    out = []
    x = relu(conv(t(img)[None, None], "conv1a")); out.append(x)
    x = pool(relu(conv(x, "conv1b"))); out.append(x)
    x = relu(conv(x, "conv2a")); out.append(x)
    x = pool(relu(conv(x, "conv2b"))); out.append(x)
    x = relu(conv(x, "conv3a")); out.append(x)
    x = pool(relu(conv(x, "conv3b"))); out.append(x)
    x = relu(conv(x, "conv4a")); out.append(x)
    x = relu(conv(x, "conv4b")); out.append(x)
    hd = torch.cat([relu(conv(x, "convPa")), relu(conv(x, "convDa"))], dim=1); out.append(hd)
    out.append(conv(hd[:, :256], "convPb"))
    out.append(conv(hd[:, 256:], "convDb"))
    return [o[0].numpy() for o in out]


# ---- the two-term fp16 split -------------------------------------------------------------------------------------------------
def fp16_split(x):
    """x fp32 -> (hi, lo) as fp32 arrays holding fp16 values: hi = RNE_fp16(x), lo = RNE_fp16(x - hi), both saturating at
    +-65504 instead of overflowing, subnormals kept (tests/studies/split_bf16_study.py::fp16_split, plus the saturation)."""
    x = np.asarray(x, F32)
    rne = lambda v: np.clip(v, -FP16_MAX, FP16_MAX).astype(np.float16).astype(F32)  # noqa: E731
    hi = rne(x)
    return hi, rne(x - hi)


def two_term(x):
    hi, lo = fp16_split(x)
    return hi + lo                     # exact: 11 + 11 significand bits, exponents at most 11 apart (or lo subnormal)


# ---- sequential-k convolutions -----------------------------------------------------------------------------------------------
BLOCK_COLUMNS = 8192                   # columns per accumulator block: [Cout][8192] fp32 stays in the cache across the K steps


def conv_seq(x, w, b, backend="numpy"):
    """Stride-1 'same' convolution, fp32: for every output, acc = 0; for k = tap * Cin + ci in order: acc += fl(w_k * x_k); + bias.
    x [C, H, W], w [O, C, k, k], b [O] -> [O, H, W].  Column blocks are independent, so blocking changes no bit."""
    x, w, b = np.ascontiguousarray(x, F32), np.ascontiguousarray(w, F32), np.asarray(b, F32)
    o, c, k, _ = w.shape
    _, h, wd = x.shape
    p = k // 2
    xp = np.zeros((c, h + 2 * p, wd + 2 * p), F32)
    xp[:, p:p + h, p:p + wd] = x
    out = np.empty((o, h, wd), F32)
    rows = max(1, BLOCK_COLUMNS // wd)
    use_torch = backend == "torch"
    if use_torch:
        wt = torch.from_numpy(w)
    for r0 in range(0, h, rows):
        r1 = min(h, r0 + rows)
        n = (r1 - r0) * wd
        if use_torch:
            acc, tmp = torch.zeros(o, n), torch.empty(o, n)
        else:
            acc, tmp = np.zeros((o, n), F32), np.empty((o, n), F32)
        for dy in range(k):
            for dx in range(k):
                bm = np.ascontiguousarray(xp[:, r0 + dy:r1 + dy, dx:dx + wd]).reshape(c, n)
                if use_torch:
                    bm = torch.from_numpy(bm)
                    for ci in range(c):
                        torch.mul(wt[:, ci, dy, dx, None], bm[ci, None, :], out=tmp)
                        acc.add_(tmp)
                else:
                    for ci in range(c):
                        np.multiply(w[:, ci, dy, dx, None], bm[ci, None, :], out=tmp)
                        np.add(acc, tmp, out=acc)
        acc = acc.numpy() if use_torch else acc
        out[:, r0:r1] = (acc + b[:, None]).reshape(o, r1 - r0, wd)
    return out


def _taps(img):
    """[9, H, W] fp32: tap t = 3 (dy + 1) + (dx + 1) of every pixel, zeros outside the image."""
    h, w = img.shape
    xp = np.zeros((h + 2, w + 2), F32)
    xp[1:-1, 1:-1] = img
    return np.stack([xp[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])


def conv1a_fma(img, w, b):
    """The direct first layer: acc = bias; acc = fma(w_t, x_t, acc) for the nine taps in order.  A fused multiply-add of fp32
    operands is the float64 sum (the product is exact there) rounded to fp32."""
    taps = _taps(img).astype(np.float64)
    w9 = np.asarray(w, np.float64).reshape(-1, 9)
    acc = np.broadcast_to(np.asarray(b, F32)[:, None, None], (w9.shape[0],) + img.shape).copy()
    for t in range(9):
        acc = (acc.astype(np.float64) + w9[:, t, None, None] * taps[t][None]).astype(F32)
    return acc


def conv1a_split(img, w, b):
    """The fused first layer: pixels, weights and bias as two-term values, acc = 0; nine taps in order, then bias * 1."""
    taps = two_term(_taps(img))
    w9 = two_term(np.asarray(w, F32).reshape(-1, 9))
    acc = np.zeros((w9.shape[0],) + img.shape, F32)
    for t in range(9):
        acc += w9[:, t, None, None] * taps[t][None]
    return acc + two_term(np.asarray(b, F32))[:, None, None]


def max_pool2(x):
    c, h, w = x.shape
    return x[:, :h // 2 * 2, :w // 2 * 2].reshape(c, h // 2, 2, w // 2, 2).max(axis=(2, 4))


def _chain_seq(sd, img, split, fused, backend):
    op = two_term if split else (lambda a: np.asarray(a, F32))
    relu = lambda a: np.maximum(a, F32(0))  # noqa: E731
    conv = lambda x, n: conv_seq(op(x), op(sd[n + ".weight"]), sd[n + ".bias"], backend)  # noqa: E731
    img = np.asarray(img, F32)
    out = []
    x = relu((conv1a_split if split and fused else conv1a_fma)(img, sd["conv1a.weight"], sd["conv1a.bias"])); out.append(x)
    x = max_pool2(relu(conv(x, "conv1b"))); out.append(x)
    x = relu(conv(x, "conv2a")); out.append(x)
    x = max_pool2(relu(conv(x, "conv2b"))); out.append(x)
    x = relu(conv(x, "conv3a")); out.append(x)
    x = max_pool2(relu(conv(x, "conv3b"))); out.append(x)
    x = relu(conv(x, "conv4a")); out.append(x)
    x = relu(conv(x, "conv4b")); out.append(x)
    hd = np.concatenate([relu(conv(x, "convPa")), relu(conv(x, "convDa"))]); out.append(hd)
    out.append(conv(hd[:256], "convPb"))
    out.append(conv(hd[256:], "convDb"))
    return out


def chain32_seq(sd, img, backend="numpy"):
    return _chain_seq(sd, img, False, False, backend)


def chain16x4_seq(sd, img, fused_first, backend="numpy"):
    return _chain_seq(sd, img, True, fused_first, backend)


# ---- per case, computed once and shared ---------------------------------------------------------------------------------------
def _stack(per_image, last):
    return [np.stack([t[s] for t in per_image]) for s in range(last + 1)]


def _last_stage(case):
    return 5 if case == WALK_CASE else NSTAGES - 1


@functools.lru_cache(maxsize=None)
def reference(case):
    """[stage] -> float64 [b, C, Hk, Wk] (the walk case: stages 0 .. 5)."""
    return _stack([chain64(weights(), im[0]) for im in images(case)], _last_stage(case))


@functools.lru_cache(maxsize=None)
def yardstick(case, precision):
    """[stage] -> fp32 [b, C, Hk, Wk]: chain32_seq for fp32, chain16x4_seq with the shape's fused_first for fp16x4.  The walk case
    runs the torch backend (a real sequential-k fp32 evaluation of all four images, bitwise what numpy gives), stages 0 .. 5."""
    backend = "torch" if case == WALK_CASE else "numpy"
    if precision == "fp32":
        per = [chain32_seq(weights(), im[0], backend) for im in images(case)]
    else:
        per = [chain16x4_seq(weights(), im[0], fused_first(case[1]), backend) for im in images(case)]
    return _stack(per, _last_stage(case))


def errors(got, case, stage, precision):
    """(e_got, e_ref, s): max |got - chain64|, max |yardstick - chain64|, max |chain64| of one stage."""
    ref = reference(case)[stage]
    return (float(np.abs(np.asarray(got, np.float64) - ref).max()),
            float(np.abs(yardstick(case, precision)[stage].astype(np.float64) - ref).max()), float(np.abs(ref).max()))


def bound(e_ref, s):
    """DESIGN section 13 for fp32 outputs: 4x the reference's own error plus 4 ulps of the output scale."""
    return 4.0 * e_ref + 4.0 * EPS32 * s
