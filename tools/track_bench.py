"""What the tracker's map update step costs on one GPU, against two yardsticks, and where one tracked frame spends its time.

    python tools/track_bench.py [--passes 5] [--warmup 3] [--sizes 1024,4096] [--out FILE]

trk_update at n_kf = n_q = 1024 and 4096 (3/4 of the keypoints paired, about half of the pairs with a known 3D point, 0.3 px
noise, 10 % gross outliers).  Per size:
  hip     MapUpdater.update: one trk_update call (three launches), timed with device events around a window of repeats
  numpy   the oracle of tests/track_oracle.py on the host, the matcher's output copied down first (host clock)  -- yardstick (a)
  eager   the same step in stock PyTorch eager ops on the same GPU: batched torch.linalg.eigh for the DLT, torch.median with
          the even-count fix for the gate (host clock + synchronise)                                          -- yardstick (b)
Before anything is timed, every discrete outcome of the two yardsticks (pairs, ids, counts, unmatched list) is checked equal
to the HIP result.  Then one BATracker.track frame on the flow sequence of tests/track_cases.py at 1024 keypoints a frame,
split by host clock (synchronised) into flow + PnP, match, update, solve and the host bookkeeping that is left.
Prints (and writes to --out, default profiles/track_bench.json) one JSON object: medians and min-max over the passes.
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

import track_cases as tc  # noqa: E402
import track_oracle as orc  # noqa: E402
from onepose_amd import BATracker, MapUpdater  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


# ---- yardstick (b): the same step, stock eager ops -----------------------------------------------------------------------------

def eager_project(X, K, T):
    c = X @ T[:3, :3].T + T[:3, 3]
    h = c @ K.T
    return h[:, :2] / h[:, 2:]


def eager_median(d):
    """numpy's median: torch.median gives the lower of the two middle values of an even count."""
    n = d.numel()
    if n == 0:
        return d.new_full((), float("nan"))
    lo = torch.median(d)
    return lo if n % 2 else (lo + torch.kthvalue(d, n // 2 + 1).values) / 2


def eager_update(m0, kf_xy, q_xy, ids, points, K_kf, K_q, pose_kf, pose_q, gate=tc.GATE, max_reproj=tc.MAX_REPROJ, max_z=tc.MAX_Z):
    n_q, n_points = q_xy.shape[0], points.shape[0]
    i = torch.nonzero((m0 >= 0) & (m0 < n_q))[:, 0]
    j = m0[i].long()
    pid = ids[i].long()
    kk = torch.nonzero((pid >= 0) & (pid < n_points))[:, 0]
    cc = torch.nonzero(pid == -1)[:, 0]
    d = (eager_project(points[pid[kk]], K_q, pose_q) - q_xy[j[kk]].double()).norm(dim=1)
    med = eager_median(d) * gate
    keep = d < med
    P1, P2 = K_kf @ pose_kf[:3], K_q @ pose_q[:3]
    a, b = kf_xy[i[cc]].double(), q_xy[j[cc]].double()
    A = torch.stack([a[:, :1] * P1[2] - P1[0], a[:, 1:] * P1[2] - P1[1], b[:, :1] * P2[2] - P2[0], b[:, 1:] * P2[2] - P2[1]], dim=1)
    _, V = torch.linalg.eigh(A.transpose(1, 2) @ A)
    X = V[:, :3, 0] / V[:, 3:, 0]
    rep_q = (eager_project(X, K_q, pose_q) - b).norm(dim=1)
    rep_kf = (eager_project(X, K_kf, pose_kf) - a).norm(dim=1)
    finite = torch.isfinite(X).all(dim=1) & torch.isfinite(rep_q) & torch.isfinite(rep_kf)
    kept = finite & ~((rep_q > max_reproj) | (rep_kf > max_reproj) | (X[:, 2] > max_z))
    q_ids = torch.full_like(pid, -1)
    q_ids[kk[keep]] = pid[kk[keep]]
    new = cc[kept]
    q_ids[new] = n_points + torch.arange(new.numel(), device=new.device)
    named = torch.zeros(n_q, dtype=torch.bool, device=m0.device)
    named[j] = True
    return i, j, q_ids, X[kept], torch.nonzero(~named)[:, 0], med


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


def measure_update(n, a, dev, updater):
    c = tc.update_problem(n, n, "half", noise=0.3, seed=500 + n, outliers=0.1)
    gpu = [torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in tc.INPUTS]
    hip = lambda: updater.update(*gpu)  # noqa: E731
    numpy_ = lambda: orc.update(gpu[0].cpu().numpy(), *(c[k] for k in tc.INPUTS[1:]))  # noqa: E731
    eager = lambda: eager_update(*gpu)  # noqa: E731

    out = hip()
    summary = out.summary.cpu().numpy().tolist()
    m, kept, free = summary[0], summary[4], summary[7]
    u = numpy_()
    assert u.summary.tolist() == summary and np.array_equal(u.q_pt_ids, out.q_pt_ids.cpu().numpy())
    assert np.array_equal(u.pair_q, out.pair_q.cpu().numpy()) and np.array_equal(u.unmatched_q, out.unmatched_q.cpu().numpy())
    ei, ej, eids, eX, efree, emed = eager()
    assert torch.equal(ei.int(), out.pair_kf[:m]) and torch.equal(ej.int(), out.pair_q[:m]) and torch.equal(eids.int(), out.q_pt_ids[:m])
    assert torch.equal(efree.int(), out.unmatched_q[:free]) and eX.shape[0] == kept
    row = {"n_kf": n, "n_q": n, "summary": summary, "launches_per_update": 3,
           "eager_median_relative_gap": float(abs(emed.item() - out.median.item()) / out.median.item()),
           "eager_new_points_max_relative_gap": float(((eX - out.new_points[:kept]).norm(dim=1) / out.new_points[:kept].norm(dim=1)).max())}
    variants = {"hip": (hip, time_events), "numpy": (numpy_, time_host), "eager": (eager, time_host)}
    for k, (fn, _) in variants.items():
        for _ in range(1 if k == "numpy" else a.warmup):
            fn()
    once = time_events(hip, 3, dev)
    reps = {"hip": max(5, int(200.0 / max(once, 1e-3))), "numpy": 1, "eager": 5}        # a window of about 0.2 s
    times = {k: [] for k in variants}
    for _ in range(a.passes):
        for k, (fn, timer) in variants.items():
            times[k].append(timer(fn, reps[k], dev))
    row["repeats_per_window"] = reps
    row["ms_per_update"] = {k: spread(t) for k, t in times.items()}
    base = statistics.median(times["hip"])
    row["yardstick_over_hip"] = {k: round(statistics.median(t) / base, 2) for k, t in times.items() if k != "hip"}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


PARTS = {"_flow_pnp": "flow_pnp", "_match": "match", "_update": "update", "_ba": "solve"}


def measure_frame(a, dev):
    """ms per BATracker.track frame, and per core, on frames 4 .. 12 of the flow sequence (the init counter has run out)."""
    seq = tc.flow_sequence(n_frames=12, n_points=1000, n_db=1000, n_extra=24)
    passes = []
    for _ in range(a.passes + 1):           # the first pass warms up (workspaces, lazy loads) and is dropped
        s = seq.copy()
        t = BATracker(device=dev)
        clock = dict.fromkeys(PARTS.values(), 0.0)

        def timed(name, fn):
            def run(*args):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                out = fn(*args)
                torch.cuda.synchronize(dev)
                clock[name] += (time.perf_counter() - t0) * 1e3
                return out
            return run

        for attr, name in PARTS.items():
            setattr(t, attr, timed(name, getattr(t, attr)))
        t.update_kf(s.kf)
        t.add_kf(s.kf)
        rows = []
        for k, frame in enumerate(s.frames):
            for name in clock:
                clock[name] = 0.0
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            t.track(frame, auto_mode=False)
            torch.cuda.synchronize(dev)
            total = (time.perf_counter() - t0) * 1e3
            if k >= 3:
                rows.append(dict(clock, total=total, host=total - sum(clock.values())))
        passes.append({key: statistics.median(r[key] for r in rows) for key in rows[0]})
    passes = passes[1:]
    return {"sequence": "tests/track_cases.flow_sequence, 1024 keypoints a frame, 512 x 512 images, frames 4-12", "keypoints_per_frame": 1024,
            "ms_per_frame": {key: spread([p[key] for p in passes]) for key in passes[0]},
            "note": "host clock with a synchronise around every core, so the parts do not overlap; host = total - the four cores"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.json"))
    a = ap.parse_args()
    assert a.passes >= 5, "at least 5 passes: the spread is part of the result"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    updater = MapUpdater()
    rows = [measure_update(int(n), a, dev, updater) for n in a.sizes.split(",")]
    res = {"metric": "trk_update_ms", "workload": "map update step of the keyframe tracker; one tracked frame",
           "variants": {"hip": "one trk_update call (device events)", "numpy": "tests/track_oracle.py on the host, matches copied down (host clock)",
                        "eager": "the same step in stock PyTorch eager ops on the same GPU (host clock + synchronise)"},
           "device": torch.cuda.get_device_name(dev), "passes": a.passes, "warmup": a.warmup, "update": rows, "frame": measure_frame(a, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
