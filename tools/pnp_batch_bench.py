"""What one batched RANSAC-EPnP call gains over solving the frames one by one, on one GPU.

    python tools/pnp_batch_bench.py [--batches 1,4,8,32] [--passes 5] [--warmup 2] [--frames-per-window 256] [--out FILE]

The `bench.py --pnp` workload (500 correspondences, 40 % outliers, 0.5 px noise, 10000 hypotheses), a different problem per frame.
For every b, three ways of solving b frames, alternating inside every pass:
  batch   one pnp_ransac_epnp_batch call
  loop    b pnp_ransac_epnp calls on one stream: what a user of the single-frame entry point does (the yardstick)
  ring    the same b calls dealt over a StreamRing, four frames in flight
and at b = 8 the matches form (1000 query keypoints, 500 of them matched): pnp_ransac_epnp_matches_batch against a loop of
pnp_ransac_epnp_matches.  All calls are raw library calls on buffers allocated once, timed by a host clock around enough repeats to
fill a window of --frames-per-window frames, ending in a device synchronise.  Before anything is timed the batch's answers are
compared with the loop's, bit for bit.  Prints (and writes to --out, default profiles/pnp_batch_bench.json) one JSON object: per
variant the median and min-max over the passes of ms per frame, and the loop's median over the variant's.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from onepose_amd import _native_pnp, pnp, synthetic  # noqa: E402
from onepose_amd.runtime import StreamRing  # noqa: E402

N, OUTLIERS, NOISE, SCALE = 500, 0.4, 0.5, 1000.0
N1 = 1000                        # query keypoints of the matches form


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def host(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


class Frames:
    """b problems and every buffer the three variants need, allocated once."""

    def __init__(self, b, dev, lib, ring, matches):
        self.b, self.lib, self.ring, self.matches, self.iters = b, lib, ring, matches, pnp.ITERATIONS
        probs = [synthetic.make_pnp_problem(N, OUTLIERS, NOISE, 8 + i) for i in range(b)]
        self.k = np.ascontiguousarray(np.stack([p["K"] for p in probs]).reshape(b, 9))
        self.seeds = np.arange(b, dtype=np.uint64)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        if matches:
            rs = np.random.RandomState(1)
            kp2 = rs.uniform(0, 512, (b, N1, 2)).astype(np.float32)
            m0 = -np.ones((b, N1), np.int64)
            for i, p in enumerate(probs):
                q = np.sort(rs.choice(N1, N, replace=False))
                kp2[i, q], m0[i, q] = p["pts_2d"], rs.permutation(N)
                probs[i] = dict(p, pts_3d=p["pts_3d"][np.argsort(m0[i, q])])     # database order: matches0 points back at the pairs
            self.cap = N1
            self.a2, self.a3, self.m0 = up(kp2), up(np.stack([p["pts_3d"] for p in probs])), up(m0)
        else:
            self.cap = N
            self.a2, self.a3 = up(np.stack([p["pts_2d"] for p in probs])), up(np.stack([p["pts_3d"] for p in probs]))
        self.counts = np.full(b, self.cap, np.int32)
        slots = len(ring.streams)
        new = lambda *shape, dtype: torch.empty(*shape, device=dev, dtype=dtype)      # noqa: E731
        self.ws_batch = new(lib.pnp_batch_workspace_bytes(b, self.cap, self.iters), dtype=torch.uint8)
        self.ws = [new(lib.pnp_workspace_bytes(self.cap, self.iters), dtype=torch.uint8) for _ in range(slots)]
        self.out_batch = (new(b, 3, 4, dtype=torch.float64), new(b, self.cap, dtype=torch.int32), new(b, 4, dtype=torch.int32))
        self.out_loop = (new(b, 3, 4, dtype=torch.float64), new(b, self.cap, dtype=torch.int32), new(b, 4, dtype=torch.int32))
        self.main = torch.cuda.current_stream(dev).cuda_stream

    def batch(self):
        pose, mask, info = self.out_batch
        tail = (self.b, self.cap)
        if self.matches:
            rc = self.lib.pnp_ransac_epnp_matches_batch(
                self.a2.data_ptr(), self.a3.data_ptr(), self.m0.data_ptr(), host(self.k, ctypes.c_double), host(self.counts, ctypes.c_int32),
                host(self.seeds, ctypes.c_uint64), *tail, N, 0, SCALE, pnp.REPROJ_ERROR, self.iters, pose.data_ptr(), mask.data_ptr(),
                info.data_ptr(), self.ws_batch.data_ptr(), self.ws_batch.numel(), self.main)
        else:
            rc = self.lib.pnp_ransac_epnp_batch(
                self.a3.data_ptr(), self.a2.data_ptr(), host(self.k, ctypes.c_double), host(self.counts, ctypes.c_int32),
                host(self.seeds, ctypes.c_uint64), *tail, SCALE, pnp.REPROJ_ERROR, self.iters, pose.data_ptr(), mask.data_ptr(), info.data_ptr(),
                self.ws_batch.data_ptr(), self.ws_batch.numel(), self.main)
        _native_pnp.check(rc, "the batched solve")

    def one(self, i, ws, stream):
        pose, mask, info = (t[i] for t in self.out_loop)
        k = host(self.k[i], ctypes.c_double)
        if self.matches:
            rc = self.lib.pnp_ransac_epnp_matches(self.a2[i].data_ptr(), self.a3[i].data_ptr(), self.m0[i].data_ptr(), N1, k, SCALE, pnp.REPROJ_ERROR,
                                                  self.iters, int(self.seeds[i]), pose.data_ptr(), mask.data_ptr(), info.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), stream)
        else:
            rc = self.lib.pnp_ransac_epnp(self.a3[i].data_ptr(), self.a2[i].data_ptr(), k, SCALE, N, pnp.REPROJ_ERROR, self.iters, int(self.seeds[i]),
                                          pose.data_ptr(), mask.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        _native_pnp.check(rc, "the single-frame solve")

    def loop(self):
        for i in range(self.b):
            self.one(i, self.ws[0], self.main)

    def ring_loop(self):
        streams = self.ring.streams
        for i in range(self.b):
            self.one(i, self.ws[i % len(streams)], streams[i % len(streams)].cuda_stream)


def timed(fn, reps, b, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / (reps * b) * 1e3


def measure(f, a, dev, variants):
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize(dev)
    f.batch()
    f.loop()
    torch.cuda.synchronize(dev)
    equal = all(torch.equal(x.view(torch.int64) if x.dtype is torch.float64 else x, y.view(torch.int64) if y.dtype is torch.float64 else y)
                for x, y in zip(f.out_batch, f.out_loop))
    assert equal, "the batch does not answer what the loop answers"
    reps = max(3, -(-a.frames_per_window // f.b))
    times = {name: [] for name in variants}
    for _ in range(a.passes):
        for name, fn in variants.items():
            times[name].append(timed(fn, reps, f.b, dev))
    row = {"b": f.b, "correspondences": N, "capacity": f.cap, "iterations": f.iters, "repeats_per_window": reps, "bitwise_equal_to_loop": equal,
           "solved": int(f.out_batch[2][:, 0].sum()), "ms_per_frame": {name: spread(t) for name, t in times.items()}}
    base = statistics.median(times["loop"])
    row["loop_over_variant"] = {name: round(base / statistics.median(t), 3) for name, t in times.items() if name != "loop"}
    row["batch_beats_loop_by_more_than_the_spread"] = bool(
        base - statistics.median(times["batch"]) > max(max(times["loop"]) - min(times["loop"]), max(times["batch"]) - min(times["batch"])))
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,8,32")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames-per-window", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_batch_bench.json"))
    a = ap.parse_args()
    ring = StreamRing("cuda:0")                    # first: it may still size the runtime's queue pool
    assert a.passes >= 5, "at least 5 passes: the spread is part of the result"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _native_pnp.load()
    rows = []
    for b in (int(x) for x in a.batches.split(",")):
        f = Frames(b, dev, lib, ring, matches=False)
        rows.append(measure(f, a, dev, {"batch": f.batch, "loop": f.loop, "ring": f.ring_loop}))
    f = Frames(8, dev, lib, ring, matches=True)
    matches = measure(f, a, dev, {"batch": f.batch, "loop": f.loop})
    matches["query_keypoints"] = N1
    res = {"metric": "pnp_ms_per_frame", "workload": f"RANSAC-EPnP, {N} correspondences ({int(OUTLIERS * 100)} % outliers, {NOISE} px noise), "
                                                      f"{pnp.ITERATIONS} hypotheses, a different problem per frame",
           "variants": {"batch": "one batched call", "loop": "b single-frame calls on one stream (the yardstick)",
                        "ring": f"b single-frame calls over {len(ring.streams)} streams"},
           "hw_queues": ring.hw_queues, "device": torch.cuda.get_device_name(dev), "passes": a.passes, "warmup": a.warmup,
           "plain": rows, "matches_b8": matches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
