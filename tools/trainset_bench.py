"""Training batches from a resident object database on one GPU: ``TrainingSet.batch`` (one ``gts_build_batch``,
include/gatsspg_trainset.h) beside (a) the reference-semantics host path -- ``database_io.build_features3d_leaves`` per sample, numpy
pads, upload -- and (b) a stock PyTorch-ROCm eager restatement on the same GPU (argsort of random keys, ``gather``), same object,
same shapes.

    python tools/trainset_bench.py [--steps 10] [--warmup 3] [--passes 5] [--out profiles/trainset_bench.json]

Shapes: (b, shape2d, shape3d, num_leaf) = (8, 1000, 2000, 8) (configs/experiment/train_GATsSPG.yaml) and (1, 1000, 7000, 8), on a
synthetic object of as many 3D points as shape3d with 2..20 observations each and 16 images of 800..1200 keypoints.  The three
implementations alternate inside every pass of one process; every timing window is at least `steps` calls and at least 0.25 s of
them, host clock around them, ending in a synchronise -> median, min, max in ms; `spread` is the larger max - min of the HIP and the
eager leg (the host leg, two orders of magnitude slower, has its own).  The three draw different random numbers (a hash, numpy's generator, torch's): what is compared is the time to make a batch of the same shape and
rule, not its bits.  `model`: bytes computed from the shape alone (no counter was read).  `training_step`: one ``training_loss``
forward + backward at the first shape with the batch made by each implementation inside the timed step.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import onepose_amd  # noqa: E402
from onepose_amd import database_io, synthetic  # noqa: E402
from onepose_amd.training import MatchingLoss, training_loss  # noqa: E402
from onepose_amd.trainset import TrainingSet  # noqa: E402

HP = dict(descriptor_dim=256, keypoints_encoder=[32, 64, 128], match_type="softmax", scale_factor=0.07, match_threshold=0.2,
          include_self=True, additional=False, with_linear_transform=False)
WINDOW_S = 0.25
HW = (512, 512)


def make_object(n_points, seed):
    rs = np.random.RandomState(seed)
    counts = rs.randint(2, 21, size=n_points)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    K = int(offsets[-1])
    n_kpts = rs.randint(800, 1201, size=16)
    features = []
    for n in n_kpts:
        pos = rs.permutation(HW[0] * HW[1])[:n]
        features.append({"keypoints": np.stack([pos % HW[1], pos // HW[1]], axis=1).astype(np.float32),
                         "descriptors": rs.standard_normal((256, n)).astype(np.float32), "scores": rs.uniform(0.1, 1, n).astype(np.float32)})
    pairs = [np.stack([np.sort(rs.permutation(n)[:300]), rs.permutation(n_points)[:300]]).astype(np.int64) for n in n_kpts]
    return dict(point_offsets=offsets, counts=counts, collect=rs.standard_normal((K, 256)).astype(np.float32),
                points3d=rs.uniform(-0.1, 0.1, (n_points, 3)).astype(np.float32), mean_desc=rs.standard_normal((256, n_points)).astype(np.float32),
                features=features, pairs=pairs)


# ---- (a) the reference-semantics host path ----
def host_batch(obj, ids, shape2d, shape3d, L, dev, rs):
    out = {k: [] for k in ("keypoints2d", "descriptors2d_query", "keypoints3d", "descriptors3d_db", "descriptors2d_db")}
    for v in ids:
        f = obj["features"][v]
        kp, d = f["keypoints"][:shape2d], f["descriptors"][:, :shape2d]
        while len(kp) < shape2d:                                        # pad_keypoints2d_random, data_utils.py:60-82
            n_pad = shape2d - len(kp)
            cand = np.stack([rs.randint(0, HW[0], n_pad), rs.randint(0, HW[1], n_pad)], axis=1).astype(np.float32)
            keep = ~(cand[:, None, :] == kp[None, :, :]).all(-1).any(1)
            kp = np.concatenate([kp, cand[keep]])
            d = np.concatenate([d, np.ones((256, int(keep.sum())), np.float32)], axis=1)
        k3 = obj["points3d"][:shape3d]
        k3 = np.concatenate([k3, rs.rand(shape3d - len(k3), 3).astype(np.float32) - 0.5])
        d3, _ = database_io.pad_features3d_random(obj["mean_desc"], np.zeros((obj["mean_desc"].shape[1], 1), np.float32), shape3d)
        leaves, _ = database_io.build_features3d_leaves(obj["collect_t"], obj["collect_scores"], obj["counts"], shape3d, L, rng=rs)
        for k, a in zip(out, (kp, d, k3, d3, leaves)):
            out[k].append(a)
    return {k: torch.from_numpy(np.stack(v)).to(dev) for k, v in out.items()}


# ---- (b) stock PyTorch-ROCm eager on the same GPU ----
class EagerSet:
    def __init__(self, obj, dev):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.dev = dev
        self.table = torch.cat([t(obj["collect"]), torch.ones(1, 256, device=dev)])           # row K: the dustbin
        self.K = obj["collect"].shape[0]
        self.counts, self.starts = t(obj["counts"].astype(np.int64)), t(obj["point_offsets"][:-1].astype(np.int64))
        self.width = int(obj["counts"].max())
        self.points3d, self.mean_desc = t(obj["points3d"]), t(obj["mean_desc"])
        self.features = [{k: t(v) for k, v in f.items()} for f in obj["features"]]

    def batch(self, ids, shape2d, shape3d, L):
        dev, b, n = self.dev, len(ids), min(len(self.counts), shape3d)
        width = max(self.width, L)
        real = torch.arange(width, device=dev)[None, :] < self.counts[:n, None]                # [n, width]
        keys = torch.rand(b, n, width, device=dev) + (~real)[None]
        chosen = keys.argsort(dim=2)[:, :, :L]                                                 # real candidates first, in random order
        chosen = torch.gather(chosen, 2, torch.rand(b, n, L, device=dev).argsort(dim=2))       # the dustbin mixed in
        src = torch.where(torch.gather(real[None].expand(b, -1, -1), 2, chosen), self.starts[None, :n, None] + chosen, self.K)
        leaves = torch.ones(b, 256, shape3d * L, device=dev)
        leaves[:, :, :n * L] = self.table[src.reshape(b, n * L)].transpose(1, 2)
        k3 = torch.cat([self.points3d[:n], torch.rand(shape3d - n, 3, device=dev) - 0.5])[None].expand(b, -1, -1).contiguous()
        d3 = torch.ones(b, 256, shape3d, device=dev)
        d3[:, :, :n] = self.mean_desc[:, :n]
        kq, dq = torch.empty(b, shape2d, 2, device=dev), torch.ones(b, 256, shape2d, device=dev)
        for s, v in enumerate(ids):
            f = self.features[v]
            m = min(f["keypoints"].shape[0], shape2d)
            kq[s, :m], dq[s, :, :m] = f["keypoints"][:m], f["descriptors"][:, :m]
            if m < shape2d:                                              # one draw, no redraw: the cheapest an eager pad can be
                kq[s, m:] = torch.stack([torch.randint(0, HW[0], (shape2d - m,), device=dev), torch.randint(0, HW[1], (shape2d - m,), device=dev)], 1).float()
        return {"keypoints2d": kq, "descriptors2d_query": dq, "keypoints3d": k3, "descriptors3d_db": d3, "descriptors2d_db": leaves}


def timed(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def legs(fns, passes, steps, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    calls = {k: max(steps, int(WINDOW_S * 1e3 / timed(fn, steps)) + 1) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(passes):
        for k, fn in fns.items():
            t[k].append(timed(fn, calls[k]))
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "calls_per_window": calls[k]}
            for k, v in t.items()}


def bytes_model(b, shape2d, shape3d, L, n):
    """written: the five tensors; read: one 1 KB row per real leaf at most, the copied parts, leaf_src twice"""
    written = 4 * b * (256 * (shape3d * L + shape3d + shape2d) + 3 * shape3d + 2 * shape2d)
    read = 4 * b * (256 * (min(n, shape3d) * L + min(n, shape3d) + shape2d)) + 2 * 4 * b * shape3d * L
    return {"written_mbytes": round(written / 1e6, 2), "read_mbytes_at_most": round(read / 1e6, 2), "note": "computed from the shape; not measured"}


def shape_row(b, shape2d, shape3d, L, dev, a):
    obj = make_object(shape3d, seed=shape3d)
    obj["collect_t"], obj["collect_scores"] = np.ascontiguousarray(obj["collect"].T), np.zeros((obj["collect"].shape[0], 1), np.float32)
    ts = TrainingSet.from_arrays(obj["point_offsets"], obj["collect"], obj["points3d"], obj["mean_desc"], obj["features"], pairs=obj["pairs"],
                                 image_size=HW, device=dev)
    eager, rs, ids = EagerSet(obj, dev), np.random.RandomState(0), list(range(b))
    epoch = [0]

    def hip():
        epoch[0] += 1
        return ts.batch(ids, epoch[0], shape2d, shape3d, L)[0]

    fns = {"hip_ms": hip, "host_ms": lambda: host_batch(obj, ids, shape2d, shape3d, L, dev, rs), "eager_ms": lambda: eager.batch(ids, shape2d, shape3d, L)}
    shapes = {k: {n: tuple(v.shape) for n, v in fn().items() if n != "image_size"} for k, fn in fns.items()}
    assert shapes["hip_ms"] == shapes["host_ms"] == shapes["eager_ms"], shapes        # what is timed makes the same tensors
    row = {"b": b, "shape2d": shape2d, "shape3d": shape3d, "num_leaf": L, "points": shape3d, "collected": int(obj["collect"].shape[0]),
           **legs(fns, a.passes, a.steps, a.warmup), "model": bytes_model(b, shape2d, shape3d, L, shape3d)}
    row["spread_ms"] = round(max(row[k]["max"] - row[k]["min"] for k in ("hip_ms", "eager_ms")), 4)       # of the two legs the verdict compares
    row["host_spread_ms"] = round(row["host_ms"]["max"] - row["host_ms"]["min"], 4)
    row["host_over_hip"] = round(row["host_ms"]["median"] / row["hip_ms"]["median"], 2)
    row["eager_over_hip"] = round(row["eager_ms"]["median"] / row["hip_ms"]["median"], 2)
    row["hip_below_eager_by_more_than_the_spread"] = bool(row["hip_ms"]["median"] + row["spread_ms"] < row["eager_ms"]["median"])
    moved = row["model"]["written_mbytes"] + row["model"]["read_mbytes_at_most"]
    row["hip_model_gbytes_per_s"] = round(moved / row["hip_ms"]["median"], 1)
    return row, (ts, eager, obj, ids)


def step_row(made, shape2d, shape3d, L, dev, a):
    ts, eager, obj, ids = made
    model = onepose_amd.GATsSuperGlue(dict(HP)).to(dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(5).items()}, strict=True)
    crit = MatchingLoss()
    target = ts.batch(ids, 0, shape2d, shape3d, L)[1]
    rs, epoch = np.random.RandomState(1), [0]

    def step(data):
        model.zero_grad(set_to_none=True)
        training_loss(model, data, target, crit).backward()

    def hip():
        epoch[0] += 1
        step(ts.batch(ids, epoch[0], shape2d, shape3d, L)[0])

    fns = {"fed_by_hip_ms": hip, "fed_by_host_ms": lambda: step(host_batch(obj, ids, shape2d, shape3d, L, dev, rs)),
           "fed_by_eager_ms": lambda: step(eager.batch(ids, shape2d, shape3d, L))}
    row = {"b": len(ids), "shape2d": shape2d, "shape3d": shape3d, "num_leaf": L, **legs(fns, a.passes, max(1, a.steps // 3), max(1, a.warmup // 2))}
    row["spread_ms"] = round(max(row[k]["max"] - row[k]["min"] for k in fns), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainset_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "trainset_bench needs a GPU (TrainingSet has no CPU path to time)"
    dev = torch.device("cuda:0")
    res = {"metric": "training_batch_build_ms", "steps": a.steps, "passes": a.passes, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "torch": torch.__version__, "numpy": np.__version__, "batch": []}
    first = None
    for shape in ((8, 1000, 2000, 8), (1, 1000, 7000, 8)):
        row, made = shape_row(*shape, dev, a)
        first = first or made
        res["batch"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if not a.no_step:
        res["training_step"] = step_row(first, 1000, 2000, 8, dev, a)
        print(json.dumps(res["training_step"]), file=sys.stderr, flush=True)
    res["per_kernel_times"] = "not measured"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
