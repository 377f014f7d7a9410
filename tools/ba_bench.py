"""What the HIP bundle adjustment costs per solve on one GPU, against two yardsticks.

    python tools/ba_bench.py [--passes 5] [--warmup 3] [--shapes small,tracker,limits] [--hip-only] [--out FILE]

Shapes: the tracker's window (21 cameras, about 3000 points, about 15 000 observations), a small one (5 cameras, 300 points)
and one at the limits of the C ABI (32 cameras, 32768 points, 262144 observations); 5 iterations, nothing fixed, 0.5 px noise, as
the reference calls it.  Per shape:
  hip     BundleAdjuster.solve: one ba_solve call, timed with device events around a window of repeats
  numpy   the oracle of tests/ba_oracle.py on the host (host clock; one run per pass)            -- yardstick (a)
  eager   the same LM through stock PyTorch eager ops on the same GPU with a dense solve          -- yardstick (b)
A yardstick a shape is too large for says so instead of a number.  Before anything is timed the three cost traces are compared.
Prints (and writes to --out, default profiles/ba_bench.json) one JSON object: per variant the median and min-max over the passes
of ms per solve, and the launch count of one ba_solve call.
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

import ba_oracle as bo  # noqa: E402
from onepose_amd import BundleAdjuster  # noqa: E402

ITERATIONS = 5
SHAPES = {"tracker": (21, 3000, 5), "small": (5, 300, 5), "limits": (32, 32768, 8)}        # cameras, points, observations per point
EAGER_MAX_UNKNOWNS = 12000          # the dense matrix of the eager yardstick is (6C + 3P)^2 doubles
NUMPY_MAX_OBSERVATIONS = 20000


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make_problem(C, P, per_point, seed):
    rng = np.random.default_rng(seed)
    points = rng.uniform(-0.1, 0.1, (P, 3))
    cams = np.concatenate([rng.uniform(-0.3, 0.3, (C, 3)), rng.uniform(-0.05, 0.05, (C, 2)), rng.uniform(0.5, 0.7, (C, 1))], axis=1)
    intr = np.tile([600.0, 600.0, 320.0, 240.0], (C, 1))
    k = min(per_point, C)
    obs_cam = np.concatenate([rng.choice(C, size=k, replace=False) for _ in range(P)]).astype(np.int32)
    obs_pt = np.repeat(np.arange(P, dtype=np.int32), k)
    order = rng.permutation(len(obs_cam))
    obs_cam, obs_pt = obs_cam[order], obs_pt[order]
    xy = bo.reproject(cams, intr, points, obs_cam, obs_pt) + rng.normal(scale=0.5, size=(len(obs_cam), 2))
    start = cams + np.concatenate([rng.normal(scale=0.01, size=(C, 3)), rng.normal(scale=0.005, size=(C, 3))], axis=1)
    return start, intr, points + rng.normal(scale=0.003, size=(P, 3)), obs_cam, obs_pt, xy


def launch_count(C, P, iterations):
    """init + the radix passes of the two sorts + offsets + 11 launches per iteration (include/mapping/bundle_adjust.h)"""
    passes = lambda K: 1 + (K >> 6 != 0) + (K >> 12 != 0)  # noqa: E731
    return 1 + passes(C) + passes(P) + 1 + 11 * iterations


# ---- yardstick (b): the same LM, stock eager ops, dense solve ---------------------------------------------------------------

def eager_residual(cam, K, p, xy):
    a = cam[:, :3]
    theta2 = (a * a).sum(dim=1)
    pos = theta2 > 0
    theta = torch.sqrt(torch.where(pos, theta2, torch.ones_like(theta2)))
    w = a / theta[:, None]
    c, s = torch.cos(theta)[:, None], torch.sin(theta)[:, None]
    full = p * c + torch.cross(w, p, dim=1) * s + w * ((w * p).sum(dim=1, keepdim=True) * (1.0 - c))
    q = torch.where(pos[:, None], full, p + torch.cross(a, p, dim=1)) + cam[:, 3:6]
    return torch.stack([K[:, 0] * (q[:, 0] / q[:, 2]) + K[:, 2], K[:, 1] * (q[:, 1] / q[:, 2]) + K[:, 3]], dim=1) - xy


def eager_lm(cams, intr, points, obs_cam, obs_pt, xy, iterations=ITERATIONS):
    cams, points = cams.clone(), points.clone()
    C, P = len(cams), len(points)
    n, K = 6 * C + 3 * P, intr[obs_cam]
    ar_c, ar_p = torch.arange(C, device=cams.device), torch.arange(P, device=cams.device)
    mu, nu, trace = bo.MU0, 2.0, []
    for _ in range(iterations):
        cam = cams[obs_cam].detach().requires_grad_(True)
        p = points[obs_pt].detach().requires_grad_(True)
        r = eager_residual(cam, K, p, xy)
        rows = [torch.autograd.grad(r[:, k].sum(), [cam, p], retain_graph=True) for k in range(2)]
        Jc, Jp, r = torch.stack([rows[0][0], rows[1][0]], dim=1), torch.stack([rows[0][1], rows[1][1]], dim=1), r.detach()
        H = torch.zeros(n, n, dtype=torch.float64, device=cams.device)
        Hcc, Hcp, Hpp = H[:6 * C, :6 * C].view(C, 6, C, 6), H[:6 * C, 6 * C:].view(C, 6, P, 3), H[6 * C:, 6 * C:].view(P, 3, P, 3)
        U = torch.zeros(C, 6, 6, dtype=torch.float64, device=cams.device).index_add_(0, obs_cam, Jc.transpose(1, 2) @ Jc)
        V = torch.zeros(P, 3, 3, dtype=torch.float64, device=cams.device).index_add_(0, obs_pt, Jp.transpose(1, 2) @ Jp)
        Hcc[ar_c, :, ar_c, :] = U
        Hpp[ar_p, :, ar_p, :] = V
        Hcp.permute(0, 2, 1, 3).index_put_((obs_cam, obs_pt), Jc.transpose(1, 2) @ Jp, accumulate=True)
        H[6 * C:, :6 * C] = H[:6 * C, 6 * C:].T
        g = torch.cat([torch.zeros(C, 6, dtype=torch.float64, device=cams.device).index_add_(0, obs_cam, (Jc * r[:, :, None]).sum(1)).reshape(-1),
                       torch.zeros(P, 3, dtype=torch.float64, device=cams.device).index_add_(0, obs_pt, (Jp * r[:, :, None]).sum(1)).reshape(-1)])
        A = H + torch.diag(H.diagonal().clamp(bo.DIAG_MIN, bo.DIAG_MAX) / mu)
        delta = torch.linalg.solve(A, -g)
        dc, dp = delta[:6 * C].view(C, 6), delta[6 * C:].view(P, 3)
        u = (Jc @ dc[obs_cam][:, :, None] + Jp @ dp[obs_pt][:, :, None])[:, :, 0]
        md = -((r * u).sum() + 0.5 * (u * u).sum())
        cost = 0.5 * (r * r).sum()
        rc = eager_residual((cams + dc)[obs_cam], K, (points + dp)[obs_pt], xy)
        cand = 0.5 * (rc * rc).sum()
        cost, cand, md = cost.item(), cand.item(), md.item()          # the host decides, as a stock implementation would
        rho = (cost - cand) / md
        accepted = bool(np.isfinite(cand) and md > 0 and rho > bo.MIN_RHO)
        trace.append([cost, cand, md, rho, mu, float(accepted)])
        if accepted:
            v = 2.0 * rho - 1.0
            mu, nu = min(mu / max(1.0 / 3.0, 1.0 - v * v * v), bo.MU_MAX), 2.0
            cams, points = cams + dc, points + dp
        else:
            mu, nu = mu / nu, 2.0 * nu
    return cams, points, np.array(trace)


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


def measure(name, a, dev, ba):
    C, P, per_point = SHAPES[name]
    host = make_problem(C, P, per_point, 100 + C)
    M = len(host[3])
    gpu = [torch.from_numpy(x).to(dev) for x in host]
    hip = lambda: ba.solve(*gpu, num_iterations=ITERATIONS, num_success_iterations=ITERATIONS)  # noqa: E731
    variants = {"hip": (hip, time_events, None)}
    row = {"shape": name, "cameras": C, "points": P, "observations": M, "iterations": ITERATIONS, "launches_per_solve": launch_count(C, P, ITERATIONS)}
    trace = hip()[2].cpu().numpy()
    row["accepted"] = int((trace[:, 5] == 1).sum())
    row["cost_first_last"] = [float(trace[0, 0]), float(trace[-1, 1])]
    if a.hip_only:
        row["numpy"] = row["eager"] = "not measured: --hip-only"
    elif M <= NUMPY_MAX_OBSERVATIONS:
        oracle = lambda: bo.lm(*host, num_iterations=ITERATIONS, num_success_iterations=ITERATIONS)  # noqa: E731
        variants["numpy"] = (oracle, time_host, 1)
        row["max_relative_cost_gap_to_numpy"] = float(np.max(np.abs(trace[:, :2] - oracle()[2][:, :2]) / np.abs(trace[:, :2])))
    else:
        row["numpy"] = f"not measured: {M} observations (the oracle's dense cross blocks are sized for tests)"
    if a.hip_only:
        pass
    elif 6 * C + 3 * P <= EAGER_MAX_UNKNOWNS:
        long_idx = [gpu[0], gpu[1], gpu[2], gpu[3].long(), gpu[4].long(), gpu[5]]
        eager = lambda: eager_lm(*long_idx)  # noqa: E731
        variants["eager"] = (eager, time_host, None)
        row["max_relative_cost_gap_to_eager"] = float(np.max(np.abs(trace[:, :2] - eager()[2][:, :2]) / np.abs(trace[:, :2])))
    else:
        row["eager"] = f"not measured: the dense matrix of {6 * C + 3 * P} unknowns does not fit a stock dense solve"
    for fn, _, reps in variants.values():
        for _ in range(1 if reps == 1 else a.warmup):
            fn()
    torch.cuda.synchronize(dev)
    once = time_events(hip, 3, dev)
    reps_hip = max(5, int(300.0 / max(once, 1e-3)))         # a window of about 0.3 s
    times = {k: [] for k in variants}
    for _ in range(a.passes):
        for k, (fn, timer, reps) in variants.items():
            times[k].append(timer(fn, reps_hip if k == "hip" else (reps or 3), dev))
    row["repeats_per_window"] = {"hip": reps_hip, "numpy": 1, "eager": 3}
    row["ms_per_solve"] = {k: spread(t) for k, t in times.items()}
    base = statistics.median(times["hip"])
    row["yardstick_over_hip"] = {k: round(statistics.median(t) / base, 2) for k, t in times.items() if k != "hip"}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="small,tracker,limits")
    ap.add_argument("--hip-only", action="store_true", help="skip the two yardsticks (for a profiler run of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_bench.json"))
    a = ap.parse_args()
    assert a.passes >= 5, "at least 5 passes: the spread is part of the result"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ba = BundleAdjuster()
    rows = [measure(name, a, dev, ba) for name in a.shapes.split(",")]
    res = {"metric": "ba_ms_per_solve", "workload": f"windowed bundle adjustment, {ITERATIONS} LM iterations, nothing fixed, 0.5 px noise",
           "variants": {"hip": "one ba_solve call (device events)", "numpy": "tests/ba_oracle.py on the host (host clock)",
                        "eager": "the same LM in stock PyTorch eager ops on the same GPU, dense solve, host decisions (host clock + synchronise)"},
           "device": torch.cuda.get_device_name(dev), "passes": a.passes, "warmup": a.warmup, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
