"""What one ragged frame batch of the GATsSPG matcher (gatsspg_forward_frames) gains over matching the frames one by one against the
same resident database, on one GPU.

    python tools/gats_frames_bench.py [--shapes 500x2000,1000x7000] [--batches 4,8,16] [--precisions fp32,fp16x4] [--passes 5]
                                      [--warmup 2] [--frames-per-window 128] [--out FILE]

For every shape (cap1 x n2), b, count pattern (all frames at cap1 / counts drawn in [0.5, 1] cap1 with a fixed seed) and arithmetic,
three ways of matching b frames, alternating inside every pass:
  loop    b gatsspg_forward_cached(b = 1) calls on one stream: what a user of the single-frame entry point does (the yardstick)
  ring    the same b calls dealt over a StreamRing, four frames in flight
  frames  one gatsspg_forward_frames call
The two forms of the GATs layer inside a frame batch are timed against each other at the layer (gatsspg_gats_layer_frames, cached leaf
logits, b frames on one workspace; "gats_layer" in the output, microseconds per launch): "stride0" = the per-frame kernel with the
database at frame stride 0, every frame re-reading the leaves, and "shared" = the kernel that reads each leaf tile once for a group of
4 frames.  A forward has three such launches.  All calls are raw library calls on buffers allocated once, timed by a host clock around enough repeats to
fill a window of --frames-per-window frames, ending in a device synchronise.  Before anything is timed the batch's answers are
compared with the loop's, bit for bit.  Prints (and writes to --out, default profiles/gats_frames_bench.json) one JSON object: per
cell the median and min-max over the passes of ms per frame, the loop's median over the variant's, and the bytes of database
resident in each form.
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

from onepose_amd import GATsSuperGlue, _native, synthetic  # noqa: E402
from onepose_amd.runtime import StreamRing  # noqa: E402

HP = {"descriptor_dim": 256, "keypoints_encoder": [32, 64, 128], "match_type": "softmax", "scale_factor": 0.07, "match_threshold": 0.2,
      "include_self": True, "additional": False, "with_linear_transform": False}
NUM_LEAF = 8


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


class Cell:
    """b frames against one database and every buffer the three variants need, allocated once."""

    def __init__(self, model, db, cap1, n2, counts, dev, ring):
        self.b, self.cap1, self.n2, self.counts, self.db, self.ring = len(counts), cap1, n2, counts, db, ring
        self.eng, self.lib = model.engine, model.engine.lib
        self.packed, self.flags = self.eng.packed_weights(dev), self.eng.flags()
        rs = np.random.RandomState(7)
        q = rs.standard_normal((self.b, 256, cap1)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        self.dq = torch.from_numpy(q).to(dev)
        self.q = [self.dq[i, :, :n].contiguous()[None] for i, n in enumerate(counts)]
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, device=dev, dtype=dtype)      # noqa: E731
        outs = lambda b, n1: (new(b, n1, n2), new(b, n1, dtype=torch.int64), new(b, n2, dtype=torch.int64), new(b, n1), new(b, n2))   # noqa: E731
        self.out_frames = outs(self.b, cap1)
        self.out_loop = [outs(1, n) for n in counts]
        slots = len(ring.streams)
        self.ws_frames = new(self.lib.gatsspg_workspace_bytes(self.b, cap1, n2, NUM_LEAF), dtype=torch.uint8)
        # a workspace per ring stream and one for the loop on the main stream: two forwards that may be in flight at once never share
        # one (with different counts they carve it differently -- the arg-max indices one reads would be the other's floats)
        self.ws = [new(self.lib.gatsspg_workspace_bytes(1, cap1, n2, NUM_LEAF), dtype=torch.uint8) for _ in range(slots)]
        self.ws_loop = new(self.lib.gatsspg_workspace_bytes(1, cap1, n2, NUM_LEAF), dtype=torch.uint8)
        self.n1 = (ctypes.c_int32 * self.b)(*counts)
        self.main = torch.cuda.current_stream(dev).cuda_stream
        self.cache_bytes = db.cache.numel() * 4

    def frames(self):
        rc = self.lib.gatsspg_forward_frames(self.packed.data_ptr(), self.dq.data_ptr(), self.n1, self.db.desc2d_db.data_ptr(), self.db.cache.data_ptr(),
                                             self.cache_bytes, self.b, self.cap1, self.n2, NUM_LEAF, self.flags, HP["scale_factor"], HP["match_threshold"],
                                             *[t.data_ptr() for t in self.out_frames], self.ws_frames.data_ptr(), self.ws_frames.numel(), self.main)
        _native.check(rc, "gatsspg_forward_frames")

    def one(self, i, ws, stream):
        rc = self.lib.gatsspg_forward_cached(self.packed.data_ptr(), self.q[i].data_ptr(), self.db.desc2d_db.data_ptr(), self.db.cache.data_ptr(),
                                             self.cache_bytes, 1, self.counts[i], self.n2, NUM_LEAF, self.flags, HP["scale_factor"], HP["match_threshold"],
                                             *[t.data_ptr() for t in self.out_loop[i]], ws.data_ptr(), ws.numel(), stream)
        _native.check(rc, "gatsspg_forward_cached")

    def loop(self):
        for i in range(self.b):
            self.one(i, self.ws_loop, self.main)

    def ring_loop(self):
        streams = self.ring.streams
        for i in range(self.b):
            self.one(i, self.ws[i % len(streams)], streams[i % len(streams)].cuda_stream)

    def equal(self):
        ok = True
        for i, n in enumerate(self.counts):
            for f, o in zip(self.out_frames, self.out_loop[i]):
                ok = ok and torch.equal(f[i, :n] if f.shape[1] == self.cap1 else f[i], o[0])
        return ok


def timed(fn, reps, b, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / (reps * b) * 1e3


def measure(c, a, dev):
    variants = {"loop": c.loop, "ring": c.ring_loop, "frames": c.frames}
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
            torch.cuda.synchronize(dev)     # the variants run on different streams and write the same output buffers: never side by side
    c.frames()
    c.loop()
    torch.cuda.synchronize(dev)
    equal = c.equal()
    assert equal, "the frame batch does not answer what the loop answers"
    reps = max(3, -(-a.frames_per_window // c.b))
    times = {name: [] for name in variants}
    for _ in range(a.passes):
        for name, fn in variants.items():
            times[name].append(timed(fn, reps, c.b, dev))
    base = statistics.median(times["loop"])
    gain = base - statistics.median(times["frames"])
    return {"repeats_per_window": reps, "bitwise_equal_to_loop": equal, "ms_per_frame": {name: spread(t) for name, t in times.items()},
            "loop_over_variant": {name: round(base / statistics.median(t), 3) for name, t in times.items() if name != "loop"},
            "frames_beats_loop_by_more_than_the_loops_spread": bool(gain > max(times["loop"]) - min(times["loop"]))}


def measure_gats_layer(model, db, cap1, n2, b, a, dev):
    """us per launch of one GATs layer over b frames: the per-frame kernel at database stride 0 against the shared-leaf kernel."""
    eng, lib = model.engine, model.engine.lib
    packed, flags = eng.packed_weights(dev), eng.flags()
    ws = torch.zeros(lib.gatsspg_workspace_bytes(b, cap1, n2, NUM_LEAF), device=dev, dtype=torch.uint8)
    tiles = (n2 + 3) // 4
    ll = db.cache[2 * 256 * n2 + 4 * (64 * 64 + 64 + 8):][:tiles * 32].contiguous()       # leaf logits of GATs layer 1 in a b = 1 cache
    st = torch.cuda.current_stream(dev).cuda_stream

    def run(shared):
        _native.check(lib.gatsspg_gats_layer_frames(packed.data_ptr(), 1, db.desc2d_db.data_ptr(), ll.data_ptr(), b, cap1, n2, NUM_LEAF, flags,
                                                    shared, ws.data_ptr(), ws.numel(), st), "gatsspg_gats_layer_frames")
    variants = {"stride0": lambda: run(0), "shared": lambda: run(1)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    times = {name: [] for name in variants}
    for _ in range(a.passes):
        for name, fn in variants.items():
            times[name].append(timed(fn, 40, 1, dev) * 1e3)
    gain = statistics.median(times["stride0"]) - statistics.median(times["shared"])
    noise = max(max(t) - min(t) for t in times.values())
    return {"cap1": cap1, "n2": n2, "b": b, "leaf_bytes": 4 * db.desc2d_db.numel(), "us_per_launch": {name: spread(t) for name, t in times.items()},
            "stride0_over_shared": round(statistics.median(times["stride0"]) / statistics.median(times["shared"]), 3),
            "shared_wins_by_more_than_the_spread": bool(gain > noise)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="500x2000,1000x7000")
    ap.add_argument("--batches", default="4,8,16")
    ap.add_argument("--precisions", default="fp32,fp16x4")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames-per-window", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gats_frames_bench.json"))
    a = ap.parse_args()
    ring = StreamRing("cuda:0")                    # first: it may still size the runtime's queue pool
    assert a.passes >= 5, "at least 5 passes: the spread is part of the result"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synthetic.make_state_dict(0).items()}
    rows, resident, layers = [], {}, []
    for shape in a.shapes.split(","):
        cap1, n2 = (int(x) for x in shape.split("x"))
        dbn = synthetic.make_inputs(1, 4, n2, NUM_LEAF, seed=3)
        dbt = {k: torch.from_numpy(dbn[k]).to(dev) for k in ("descriptors3d_db", "descriptors2d_db")}
        for prec in a.precisions.split(","):
            model = GATsSuperGlue(HP, precision=prec).eval()
            model.load_state_dict(sd, strict=True)
            model = model.to(dev)
            db = model.prepare_database(dbt)
            one = 4 * (dbt["descriptors3d_db"].numel() + dbt["descriptors2d_db"].numel() + db.cache.numel())
            if prec == a.precisions.split(",")[0]:      # the GATs layer is fp32 in every arithmetic
                for b in (int(x) for x in a.batches.split(",")):
                    layers.append(measure_gats_layer(model, db, cap1, n2, b, a, dev))
                    print(json.dumps(layers[-1]), file=sys.stderr, flush=True)
            for b in (int(x) for x in a.batches.split(",")):
                resident[f"{shape} b={b}"] = {"loop": one, "ring": one, "frames": one, "uniform_batch_forward_cached": b * one}
                rs = np.random.RandomState(100 + b)
                for pattern, counts in (("equal", [cap1] * b), ("ragged", [int(x) for x in rs.randint(cap1 // 2, cap1 + 1, b)])):
                    row = {"cap1": cap1, "n2": n2, "b": b, "precision": prec, "counts": pattern, "n1": counts}
                    row.update(measure(Cell(model, db, cap1, n2, counts, dev, ring), a, dev))
                    print(json.dumps(row), file=sys.stderr, flush=True)
                    rows.append(row)
            del model, db
            torch.cuda.empty_cache()
    res = {"metric": "gatsspg_ms_per_frame", "workload": "GATsSPG cached forward, random weights, b frames of one object against ONE resident database",
           "variants": {"loop": "b gatsspg_forward_cached(b = 1) calls on one stream (the yardstick)",
                        "ring": f"the same b calls over {len(ring.streams)} streams",
                        "frames": "one gatsspg_forward_frames call"},
           "gats_layer": layers,
           "hw_queues": ring.hw_queues, "device": torch.cuda.get_device_name(dev), "passes": a.passes, "warmup": a.warmup,
           "database_bytes_resident": resident, "cells": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
