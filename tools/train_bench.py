"""The matcher's training head on one GPU: forward + backward of ``MatchingLoss(impl="hip")`` (one chain of HIP launches,
include/gatsspg_train.h) beside ``impl="eager"`` (the reference head in stock PyTorch ops) on the same GPU, same inputs: unit-norm
descriptors that require grad and the dense int16 target of the reference's datamodule, all resident.

    python tools/train_bench.py [--steps 10] [--warmup 3] [--passes 5] [--out profiles/train_bench.json]

Legs: the head alone at (8, 1000, 2000) (configs/experiment/train_GATsSPG.yaml: batch 8) and (1, 1000, 7000); one whole
``training_loss`` step (stock-torch trunk + head, forward + backward, 8 leaves) at (8, 1000, 2000) with each head, and the head's share
of it.  The two implementations alternate inside every pass of one process; every timing window is at least `steps` calls and at
least 0.25 s of them, with the host clock around them, and ends in a synchronise -> median, min, max in ms; `spread` is the larger
max - min of the two.  `hip_sparse_ms` is the HIP head fed the sparse pairs instead (gtr_build_target writes the class matrix on the
device), for information.

`model`: bytes and flops of every launch of the HIP chain computed from the shape alone (no counter was read); per-kernel times are
NOT measured by this tool (take rocprofv3 --kernel-trace --stats in a run of its own for them).
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

import onepose_amd  # noqa: E402
from onepose_amd import synthetic  # noqa: E402
from onepose_amd.training import MatchingLoss, SparseTarget, training_loss  # noqa: E402
import train_oracle  # noqa: E402

HP = dict(descriptor_dim=256, keypoints_encoder=[32, 64, 128], match_type="softmax", scale_factor=0.07, match_threshold=0.2,
          include_self=True, additional=False, with_linear_transform=False)


def launch_model(b, n, m):
    """Bytes moved to / from HBM (every operand counted once per launch, partial-sum buffers left out: < 2 %) and flops of the HIP chain."""
    ldn, ldm, d = -(-n // 128) * 128, -(-m // 64) * 64, 256
    e = 4 * b * ldn * ldm
    x, y = 4 * b * d * n, 4 * b * d * m
    px, py = 4 * b * d * ldn, 4 * b * d * ldm
    rows = [
        ("pack + transposed pack", x + 2 * y + px + 2 * py, 0),
        ("score + exp tile kernel", px + py + e, 2 * b * ldn * ldm * d),
        ("loss terms pass", e + b * n * m, 0),
        ("dS pass (E in place)", 2 * e + b * n * m, 0),
        ("dx contraction", e + py + x, 2 * b * ldn * ldm * d),
        ("dy contraction", e + px + y, 2 * b * ldn * ldm * d),
    ]
    return {"launches": [{"launch": k, "mbytes": round(v / 1e6, 2), "gflop": round(f / 1e9, 3)} for k, v, f in rows],
            "total_mbytes": round(sum(v for _, v, _ in rows) / 1e6, 1), "total_gflop": round(sum(f for _, _, f in rows) / 1e9, 2),
            "note": "computed from the shape; not measured"}


def timed(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


WINDOW_S = 0.25     # a timing window shorter than this measures the clock and the scheduler as much as the kernels


def legs(fns, passes, steps, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    calls = {k: max(steps, int(WINDOW_S * 1e3 / timed(fn, steps)) + 1) for k, fn in fns.items()}     # calls per window, per leg
    t = {k: [] for k in fns}
    for _ in range(passes):
        for k, fn in fns.items():
            t[k].append(timed(fn, calls[k]))
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "calls_per_window": calls[k]}
            for k, v in t.items()}


def verdict(row, hip="hip_ms", eager="eager_ms"):
    h, e = row[hip], row[eager]
    row["spread_ms"] = round(max(h["max"] - h["min"], e["max"] - e["min"]), 4)
    row["eager_over_hip"] = round(e["median"] / h["median"], 2)
    row["hip_below_eager_by_more_than_the_spread"] = bool(h["median"] + row["spread_ms"] < e["median"])


def head_row(b, n, m, dev, a):
    x, y, pairs, target = train_oracle.make_head_case(b=b, n=n, m=m, k=min(n, m) // 3, seed=b * 1000 + m, noise=0.8)
    x, y = torch.from_numpy(x).to(dev).requires_grad_(), torch.from_numpy(y).to(dev).requires_grad_()
    target = torch.from_numpy(target).to(dev)
    sparse = SparseTarget([torch.from_numpy(p).to(dev) for p in pairs], n, m)
    crit = {impl: MatchingLoss(impl=impl) for impl in ("hip", "eager")}

    def step(impl, tgt):
        x.grad = y.grad = None
        crit[impl](x, y, tgt).backward()

    step("hip", target)
    gh, lh = (x.grad.clone(), y.grad.clone()), crit["hip"](x, y, target).item()
    step("eager", target)
    le = crit["eager"](x, y, target).item()
    agree = {"loss_hip": lh, "loss_eager": le,
             "dx_max_rel_diff": float((gh[0] - x.grad).abs().max() / x.grad.abs().max()),
             "dy_max_rel_diff": float((gh[1] - y.grad).abs().max() / y.grad.abs().max())}
    assert abs(lh - le) <= 1e-5 * abs(le) and max(agree["dx_max_rel_diff"], agree["dy_max_rel_diff"]) < 1e-4, agree   # what is timed computes the same
    row = {"b": b, "n": n, "m": m, "agreement": agree,
           **legs({"hip_ms": lambda: step("hip", target), "eager_ms": lambda: step("eager", target), "hip_sparse_ms": lambda: step("hip", sparse)},
                  a.passes, a.steps, a.warmup), "model": launch_model(b, n, m)}
    verdict(row)
    row["hip_model_gbytes_per_s"] = round(row["model"]["total_mbytes"] / row["hip_ms"]["median"], 1)
    return row


def step_row(b, n, m, num_leaf, dev, a):
    d, tg = synthetic.make_inputs(b=b, n1=n, n2=m, num_leaf=num_leaf, seed=5, planted=True, noise=(0.3, 0.5), with_targets=True)
    data = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    target = torch.zeros(b, n, m, dtype=torch.int16, device=dev)
    for bi in range(b):
        target[bi, torch.arange(tg.shape[1]), torch.from_numpy(tg[bi]).long()] = 1
    model = onepose_amd.GATsSuperGlue(dict(HP)).to(dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(5).items()}, strict=True)
    crit = {impl: MatchingLoss(impl=impl) for impl in ("hip", "eager")}

    def step(impl):
        model.zero_grad(set_to_none=True)
        training_loss(model, data, target, crit[impl]).backward()

    with torch.no_grad():
        mx, my = onepose_amd.matching_descriptors(model, data)
    mx, my = mx.clone().requires_grad_(), my.clone().requires_grad_()

    def head(impl):
        mx.grad = my.grad = None
        crit[impl](mx, my, target).backward()

    row = {"b": b, "n": n, "m": m, "num_leaf": num_leaf,
           **legs({"hip_ms": lambda: step("hip"), "eager_ms": lambda: step("eager"), "head_alone_hip_ms": lambda: head("hip"),
                   "head_alone_eager_ms": lambda: head("eager")}, a.passes, max(1, a.steps // 3), max(1, a.warmup // 2))}
    verdict(row)
    for impl in ("hip", "eager"):
        row[f"head_share_of_step_{impl}"] = round(row[f"head_alone_{impl}_ms"]["median"] / row[f"{impl}_ms"]["median"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "train_bench needs a GPU (impl='hip' has no CPU path to time)"
    dev = torch.device("cuda:0")
    res = {"metric": "matching_head_forward_backward_ms", "steps": a.steps, "passes": a.passes, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "numpy": np.__version__, "head": []}
    for shape in ((8, 1000, 2000), (1, 1000, 7000)):
        res["head"].append(head_row(*shape, dev, a))
        print(json.dumps(res["head"][-1]), file=sys.stderr, flush=True)
    if not a.no_step:
        res["training_step"] = step_row(8, 1000, 2000, 8, dev, a)
        print(json.dumps(res["training_step"]), file=sys.stderr, flush=True)
    res["per_kernel_times"] = "not measured"
    res["all_ok"] = bool(all(r["hip_below_eager_by_more_than_the_spread"] for r in res["head"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
