"""What the tracker's flow step costs per frame on one GPU, against two yardsticks.

    python tools/flow_bench.py [--passes 5] [--warmup 3] [--points 300,1000,4096] [--variant-lib FILE] [--hip-only] [--out FILE]

Shape: the tracker's -- a 512 x 512 crop, 15 x 15 window, 3 levels, 10 iterations, eps 0.03 -- on the planted texture of
tests/flow_cases.py under a 4-px shift, n = 300 (the tracker's), 1000 and 4096 points.  Per n:
  pyramid  FlowTracker.pyramid of the new frame (device events around a window of repeats)
  track    FlowTracker.track: one flow_track launch (device events)
  device   FlowTracker.flow_track_device: track -> RANSAC-EPnP -> reprojection mean (device events)
  numpy    the oracle of tests/flow_oracle.py on the host, n = 300 only (host clock; one run per pass)     -- yardstick (a)
  eager    the same algorithm in stock PyTorch eager integer ops on the same GPU, vectorised over the points, every
           iteration masked (host clock + synchronise); the Scharr planes are built outside the timed region    -- yardstick (b)
Before anything is timed the three results are compared for equality (points bit for bit).  ``--variant-lib`` names a second
build of libdet_hip.so (the A/B arm of DESIGN section 18: -DFLOW_STAGE_SECOND_IMAGE); its ``track`` is timed in the same
passes, interleaved.  Prints (and writes to --out, default profiles/flow_bench.json) one JSON object: per variant the median
and min-max over the passes of ms per call.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flow_cases as fc  # noqa: E402
import flow_oracle as fo  # noqa: E402
from onepose_amd import FlowTracker, _native_det  # noqa: E402

SIZE, SHIFT, WIN, MAX_LEVEL, MAX_ITER, EPS = 512, (4, 0), (15, 15), 2, 10, 0.03
NUMPY_MAX_POINTS = 300


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make_scene(n, seed=1):
    """The planted pair, n keyframe points at least 20 px inside, their 3D points under a known pose and the query's K."""
    rs = np.random.RandomState(seed)
    first, second = fc.image_pair(SIZE, SIZE, SHIFT, sigma=0.08, seed=seed)
    K = np.array([[1200.0, 0, SIZE / 2], [0, 1200.0, SIZE / 2], [0, 0, 1]])
    uv = rs.uniform(20, SIZE - 21, (n, 2))
    z = rs.uniform(0.5, 0.7, n)
    X = (np.concatenate([(uv - K[:2, 2]) / 1200.0, np.ones((n, 1))], axis=1) * z[:, None]).astype(np.float32)     # pose = identity
    kpts = ((X.astype(np.float64) @ K.T)[:, :2] / X[:, 2:].astype(np.float64)).astype(np.float32)
    K_query = K.copy()
    K_query[0, 2] += SHIFT[0]
    K_query[1, 2] += SHIFT[1]
    return first, second, kpts, X, K_query


# ---- yardstick (b): the same algorithm, stock eager ops ------------------------------------------------------------------

def reflect(x, n):
    if n == 1:
        return torch.zeros_like(x)
    p = 2 * (n - 1)
    x = torch.remainder(x, p)
    return torch.where(x >= n, p - x, x)


def eager_scharr(img):
    H, W = img.shape
    ar = lambda n: torch.arange(n, device=img.device)  # noqa: E731
    ym, yp, xm, xp = reflect(ar(H) - 1, H), reflect(ar(H) + 1, H), reflect(ar(W) - 1, W), reflect(ar(W) + 1, W)
    g = lambda r, c: img[r][:, c]  # noqa: E731
    ix = 3 * (g(ym, xp) - g(ym, xm)) + 10 * (img[:, xp] - img[:, xm]) + 3 * (g(yp, xp) - g(yp, xm))
    iy = 3 * (g(yp, xm) - g(ym, xm)) + 10 * (img[yp] - img[ym]) + 3 * (g(yp, xp) - g(ym, xp))
    return ix, iy


def eager_origin(pos, size):
    half = torch.tensor([(WIN[0] - 1) / 2, (WIN[1] - 1) / 2], dtype=torch.float64, device=pos.device)
    c = pos - half
    ip = torch.floor(c)
    ok = (ip[:, 0] >= -WIN[0]) & (ip[:, 0] < size[1]) & (ip[:, 1] >= -WIN[1]) & (ip[:, 1] < size[0])
    a, b = (c - ip).unbind(1)
    w00 = torch.round((1.0 - a) * (1.0 - b) * 16384.0).long()
    w01 = torch.round(a * (1.0 - b) * 16384.0).long()
    w10 = torch.round((1.0 - a) * b * 16384.0).long()
    w = [x[:, None, None] for x in (w00, w01, w10, 16384 - w00 - w01 - w10)]
    return torch.where(ok[:, None], ip, torch.zeros_like(ip)).long(), w, ok


def eager_sample(plane, ip, w, rounding, shift, zero_outside):
    H, W = plane.shape
    ys = ip[:, 1, None] + torch.arange(WIN[1] + 1, device=plane.device)
    xs = ip[:, 0, None] + torch.arange(WIN[0] + 1, device=plane.device)
    if zero_outside:
        inside = ((ys >= 0) & (ys < H))[:, :, None] & ((xs >= 0) & (xs < W))[:, None, :]
        blk = plane[ys.clamp(0, H - 1)[:, :, None], xs.clamp(0, W - 1)[:, None, :]] * inside
    else:
        blk = plane[reflect(ys, H)[:, :, None], reflect(xs, W)[:, None, :]]
    patch = blk[:, :-1, :-1] * w[0] + blk[:, :-1, 1:] * w[1] + blk[:, 1:, :-1] * w[2] + blk[:, 1:, 1:] * w[3]
    return (patch + rounding) >> shift


def eager_track(levels_i, levels_j, derivs, pts):
    """levels_*: int64 planes per level; derivs: (ix, iy) per level of the first image; pts [n, 2] fp32 on the GPU."""
    n, dev = len(pts), pts.device
    p = pts.double()
    L = len(levels_i) - 1
    status = torch.ones(n, dtype=torch.int32, device=dev)
    trace = torch.zeros(n, L + 1, 2, dtype=torch.int32, device=dev)
    area2, eps2 = float(2 * WIN[0] * WIN[1]), EPS * EPS
    code_of = lambda mask, value, code: torch.where(mask, torch.full_like(code, value), code)  # noqa: E731
    nxt = None
    for l in range(L, -1, -1):
        size = levels_i[l].shape
        prev = p * 2.0 ** -l
        nxt = prev.clone() if l == L else 2.0 * nxt
        ip, w, ok = eager_origin(prev, size)
        ival = eager_sample(levels_i[l], ip, w, 256, 9, False)
        ix, iy = eager_sample(derivs[l][0], ip, w, 8192, 14, True), eager_sample(derivs[l][1], ip, w, 8192, 14, True)
        a11, a12, a22 = ((ix * ix).sum((1, 2)).double() * fo.SCALE, (ix * iy).sum((1, 2)).double() * fo.SCALE,
                         (iy * iy).sum((1, 2)).double() * fo.SCALE)
        D = a11 * a22 - a12 * a12
        min_eig = (a22 + a11 - torch.sqrt((a11 - a22) * (a11 - a22) + 4.0 * a12 * a12)) / area2
        good = ok & ~((min_eig < fo.MIN_EIG_THRESHOLD) | (D < fo.MIN_DET))
        code = torch.full((n,), fo.EXIT_SKIPPED, dtype=torch.int32, device=dev)
        code = code_of(ok, fo.EXIT_REJECTED, code)
        code = code_of(good, fo.EXIT_ITERATION_CAP, code)
        active, ran, pd = good.clone(), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, 2, dtype=torch.float64, device=dev)
        for j in range(MAX_ITER):
            ipj, wj, okj = eager_origin(nxt, size)
            code = code_of(active & ~okj, fo.EXIT_LEFT_RANGE, code)
            active = active & okj
            ran = torch.where(active, torch.full_like(ran, j + 1), ran)
            diff = eager_sample(levels_j[l], ipj, wj, 256, 9, False) - ival
            b1, b2 = (diff * ix).sum((1, 2)).double() * fo.SCALE, (diff * iy).sum((1, 2)).double() * fo.SCALE
            d = torch.stack([(a12 * b2 - a22 * b1) / D, (a12 * b1 - a11 * b2) / D], dim=1)
            nxt = torch.where(active[:, None], nxt + d, nxt)
            conv = active & (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= eps2)
            code = code_of(conv, fo.EXIT_CONVERGED, code)
            active = active & ~conv
            if j > 0:
                osc = active & ((d + pd).abs() < fo.OSCILLATION).all(dim=1)
                nxt = torch.where(osc[:, None], nxt - 0.5 * d, nxt)
                code = code_of(osc, fo.EXIT_OSCILLATION, code)
                active = active & ~osc
            pd = d
        if l == 0:
            status = torch.where(code >= fo.EXIT_LEFT_RANGE, torch.zeros_like(status), status)
        trace[:, l, 0], trace[:, l, 1] = ran, code
    status = torch.where(eager_origin(nxt, levels_i[0].shape)[2], status, torch.zeros_like(status))
    matches0 = torch.where(status == 1, torch.arange(n, device=dev), torch.full((n,), -1, device=dev, dtype=torch.int64))
    return nxt.float(), status, matches0, trace


# ---- timing -------------------------------------------------------------------------------------------------------------------

def time_events(fn, reps, dev):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def time_host(fn, reps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / reps * 1e3


def window_reps(fn, dev):
    return max(5, int(300.0 / max(time_events(fn, 3, dev), 1e-3)))          # a window of about 0.3 s


def measure(n, a, dev, tracker, variant):
    first, second, kpts, X, K_query = make_scene(n)
    g_first, g_second, g_kpts, g_X = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (first, second, kpts, X))
    pyr_kf, pyr_query = tracker.pyramid(g_first), tracker.pyramid(g_second)
    variants = {"pyramid": (lambda: tracker.pyramid(g_second), time_events, None),
                "track": (lambda: tracker.track(pyr_kf, pyr_query, g_kpts), time_events, None),
                "device": (lambda: tracker.flow_track_device(pyr_kf, pyr_query, g_kpts, g_X, K_query), time_events, None)}
    row = {"points": n, "image": [SIZE, SIZE], "window": list(WIN), "levels": pyr_kf.levels, "max_iter": MAX_ITER, "eps": EPS,
           "launches": {"pyramid": pyr_kf.levels - 1, "track": 1, "reproj": 1}}
    nxt, status, m0, trace = (t.cpu().numpy() for t in tracker.track(pyr_kf, pyr_query, g_kpts, trace=True))
    row["tracked"] = int(status.sum())
    row["worst_error_px"] = round(float(np.abs(nxt - (kpts + np.array(SHIFT, np.float32)))[status == 1].max()), 5)
    it0 = trace[:, 0, 0]
    row["level0_iterations"] = {str(int(k)): int((it0 == k).sum()) for k in np.unique(it0)}
    if variant is not None:
        v_kf, v_query = variant.pyramid(g_first), variant.pyramid(g_second)
        got = variant.track(v_kf, v_query, g_kpts)
        assert got[0].cpu().numpy().tobytes() == nxt.tobytes() and np.array_equal(got[1].cpu().numpy(), status), "the variant library differs"
        variants["track_variant"] = (lambda: variant.track(v_kf, v_query, g_kpts), time_events, None)
    if not a.hip_only:
        lev_i, lev_j = ([p.level(l).long() for l in range(p.levels)] for p in (pyr_kf, pyr_query))
        derivs = [eager_scharr(x) for x in lev_i]
        eager = lambda: eager_track(lev_i, lev_j, derivs, g_kpts)  # noqa: E731
        e = [t.cpu().numpy() for t in eager()]
        assert e[0].tobytes() == nxt.tobytes() and np.array_equal(e[1], status) and np.array_equal(e[2], m0) and np.array_equal(e[3], trace), \
            "the eager restatement differs from the HIP tracker"
        variants["eager"] = (eager, time_host, 3)
        if n <= NUMPY_MAX_POINTS:
            pi, pj = fo.Pyramid(first, pyr_kf.levels), fo.Pyramid(second, pyr_kf.levels)
            oracle = lambda: fo.track(pi, pj, kpts, None, WIN, MAX_ITER, EPS)  # noqa: E731
            o = oracle()
            assert o[0].tobytes() == nxt.tobytes() and np.array_equal(o[1], status) and np.array_equal(o[3], trace), "the oracle differs"
            variants["numpy"] = (oracle, time_host, 1)
        else:
            row["numpy"] = f"not measured: n = {NUMPY_MAX_POINTS} only"
    for fn, _, reps in variants.values():
        for _ in range(1 if reps == 1 else a.warmup):
            fn()
    torch.cuda.synchronize(dev)
    reps_of = {k: (reps or window_reps(fn, dev)) for k, (fn, _, reps) in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(a.passes):
        for k, (fn, timer, _) in variants.items():
            times[k].append(timer(fn, reps_of[k], dev))
    row["repeats_per_window"] = reps_of
    row["ms"] = {k: spread(t) for k, t in times.items()}
    base = statistics.median(times["track"])
    row["over_hip_track"] = {k: round(statistics.median(times[k]) / base, 2) for k in ("eager", "numpy", "track_variant") if k in times}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", default="300,1000,4096")
    ap.add_argument("--variant-lib", default=None, help="a second build of libdet_hip.so whose flow_track is timed alongside")
    ap.add_argument("--hip-only", action="store_true", help="skip the two yardsticks (for a profiler run of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_bench.json"))
    a = ap.parse_args()
    assert a.passes >= 5, "at least 5 passes: the spread is part of the result"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    tracker = FlowTracker(WIN, MAX_LEVEL, MAX_ITER, EPS)
    variant = None
    if a.variant_lib:
        _native_det.LIB_PATH, _native_det._lib = os.path.abspath(a.variant_lib), None       # bind() reads both through the module
        variant = FlowTracker(WIN, MAX_LEVEL, MAX_ITER, EPS)
        assert variant.lib is not tracker.lib
    rows = [measure(int(n), a, dev, tracker, variant) for n in a.points.split(",")]
    res = {"metric": "flow_ms_per_call", "workload": f"pyramidal LK, {SIZE} x {SIZE}, window {WIN[0]} x {WIN[1]}, planted texture, {SHIFT[0]}-px shift",
           "variants": {"pyramid": "FlowTracker.pyramid of the new frame (device events)", "track": "one flow_track launch (device events)",
                        "device": "flow_track_device: track, RANSAC-EPnP (10000 hypotheses), reprojection mean (device events)",
                        "track_variant": "flow_track of --variant-lib (device events)",
                        "numpy": "tests/flow_oracle.py on the host (host clock)",
                        "eager": "the same algorithm in stock PyTorch eager ops on the same GPU, all iterations masked (host clock + synchronise)"},
           "variant_lib": os.path.basename(a.variant_lib) if a.variant_lib else None,
           "device": torch.cuda.get_device_name(dev), "passes": a.passes, "warmup": a.warmup, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
