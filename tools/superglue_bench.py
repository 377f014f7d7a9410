"""SuperGlue 2D-2D matcher throughput on one GPU: HIP module vs the stock PyTorch eager restatement (outdoor config).

    python tools/superglue_bench.py [--steps 10] [--warmup 3] [--shapes 512x512,1024x1024,...]

Prints one JSON line: per shape pairs/s and ms per pair one at a time and with 4 pairs in flight (StreamRing), algorithmic
GFLOP per pair, the fraction of the fp32-MFMA peak, the eager restatement's ms per pair, and the time of the Sinkhorn stage alone.

    python tools/superglue_bench.py --ragged [--passes 5] [--steps 3]

The ragged leg instead: b pairs (4, 15, 16) at 512 and 1024 keypoints, with equal counts and with n0, n1 drawn uniformly in
[0.5, 1] x cap, through SuperGlue.match_pairs (one ragged batch, packing included) beside the same pairs one forward at a time
and 4 in flight; per leg the median and the min / max over the passes, in ms per pair.  Prints {"ragged": [...]}.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from onepose_amd import configure_hip_queues  # noqa: E402

configure_hip_queues()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from onepose_amd import StreamRing, SuperGlue, synthetic  # noqa: E402
import superglue_oracle as so  # noqa: E402

PEAK_TFLOPS = 157.3
OUTDOOR = {"GNN_layers": ["self", "cross"] * 9, "sinkhorn_iterations": 100, "match_threshold": 0.7}


def gflop(n, m, layers=18):
    per_side = lambda a, b: 2 * (2 * a + 2 * b) * 256 ** 2 + 4 * a * b * 256 + 2 * a * (512 ** 2 + 512 * 256)  # noqa: E731
    total = 0.0
    for i in range(layers):
        cross = i % 2 == 1
        total += per_side(n, m if cross else n) + per_side(m, n if cross else m)
    total += 2 * (n + m) * 256 ** 2 + 2 * n * m * 256          # final_proj + score GEMM
    return total / 1e9


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def spread(fn, passes, steps, pairs):
    """ms per pair: median, min, max over `passes` timings of `steps` calls of fn (fn handles `pairs` pairs)."""
    t = sorted(timed(fn, steps, 1) / pairs for _ in range(passes))
    return {"median": round(t[len(t) // 2], 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def ragged_leg(model, dev, ring, passes, steps):
    rows = []
    rs = np.random.RandomState(3)
    for cap in (512, 1024):
        for b in (4, 15, 16):
            for draw in ("equal", "ragged"):
                counts = [(cap, cap)] * b if draw == "equal" else [tuple(int(x) for x in rs.randint(cap // 2, cap + 1, 2)) for _ in range(b)]
                items = []
                for k, (n, m) in enumerate(counts):
                    inp = synthetic.make_superglue_inputs(1, n, m, 512, 512, seed=11 + k)
                    d = {key: torch.from_numpy(inp[key]).to(dev) for key in ("keypoints0", "keypoints1", "scores0", "scores1",
                                                                             "descriptors0", "descriptors1")}
                    d["image0"] = d["image1"] = torch.empty(1, 1, 512, 512, device="meta")
                    items.append(d)

                def serial():
                    for d in items:
                        model(d)

                def four():
                    for d in items:
                        with ring.next():
                            model(d)
                g = sum(gflop(n, m) for n, m in counts) / b
                row = {"cap": cap, "b": b, "draw": draw, "mean_n0": round(float(np.mean([c[0] for c in counts])), 1),
                       "mean_n1": round(float(np.mean([c[1] for c in counts])), 1),
                       "serial_ms_per_pair": spread(serial, passes, steps, b), "four_in_flight_ms_per_pair": spread(four, passes, steps, b),
                       "ragged_ms_per_pair": spread(lambda: model.match_pairs(items, max_items=b), passes, steps, b)}
                row["speedup_vs_serial"] = round(row["serial_ms_per_pair"]["median"] / row["ragged_ms_per_pair"]["median"], 2)
                row["ragged_beats_serial_by_more_than_its_spread"] = bool(
                    row["serial_ms_per_pair"]["median"] - row["ragged_ms_per_pair"]["median"]
                    > row["serial_ms_per_pair"]["max"] - row["serial_ms_per_pair"]["min"])
                row["frac_fp32_mfma_peak_ragged"] = round(g / row["ragged_ms_per_pair"]["median"] / PEAK_TFLOPS, 4)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", action="store_true", help="run the ragged-batch leg only")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="512x512,1024x1024,2048x2048,4096x4096,1024x2048")
    ap.add_argument("--eager-steps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synthetic.make_superglue_state_dict(10, 18)
    model = SuperGlue(OUTDOOR).eval()
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.to(dev)
    params = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd.items()}
    ring = StreamRing(dev)
    if a.ragged:
        print(json.dumps({"metric": "superglue_ragged_ms_per_pair", "config": "outdoor",
                          "ragged": ragged_leg(model, dev, ring, a.passes, min(a.steps, 3))}))
        return
    rows = []
    for shp in a.shapes.split(","):
        n, m = (int(x) for x in shp.split("x"))
        inp = synthetic.make_superglue_inputs(1, n, m, 512, 512, seed=11)
        d = {k: torch.from_numpy(inp[k]).to(dev) for k in ("keypoints0", "keypoints1", "scores0", "scores1", "descriptors0",
                                                           "descriptors1")}
        d["image0"] = d["image1"] = torch.empty(1, 1, 512, 512, device=dev)
        ms = timed(lambda: model(d), a.steps, a.warmup)

        def four():
            for _ in range(4):
                with ring.next():
                    model(d)
        ms4 = timed(four, max(1, a.steps // 2), 1) / 4
        sc = torch.randn(1, n, m, device=dev)
        ms_sk = timed(lambda: model.engine.sinkhorn(sc, 1.0, 100), a.steps, a.warmup)
        ed = dict(d, image_size0=(512, 512), image_size1=(512, 512))
        with torch.no_grad():
            ms_eager = timed(lambda: so.forward_torch(params, ed, OUTDOOR), a.eager_steps, 1)
        g = gflop(n, m)
        rows.append({"n0": n, "n1": m, "ms_per_pair": round(ms, 3), "pairs_per_s": round(1e3 / ms, 1),
                     "ms_per_pair_4_in_flight": round(ms4, 3), "pairs_per_s_4_in_flight": round(1e3 / ms4, 1),
                     "gflop_per_pair": round(g, 1), "frac_fp32_mfma_peak": round(g / ms / PEAK_TFLOPS, 4),
                     "sinkhorn_ms": round(ms_sk, 3), "eager_ms_per_pair": round(ms_eager, 3),
                     "speedup_vs_eager": round(ms_eager / ms, 2)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"metric": "superglue_pairs_per_s", "config": "outdoor", "shapes": rows}))


if __name__ == "__main__":
    main()
