"""Nearest-neighbour matcher on one GPU: the HIP module (similarity fused with the top-2 selection: the n0 x n1 matrix is never
written) beside (a) the stock PyTorch eager restatement of the reference (einsum, two topk, the wheres) on the same GPU, (b) the
SuperGlue figure for the same shape from profiles/sg_bench.json / profiles/det_bench.json and (c) the share of the fp32-MFMA peak
that the WHOLE call reaches on the contraction's algorithmic flops (2 n0 n1 256; pack, selection and finalize are in the time).

    python tools/nn_matcher_bench.py [--steps 20] [--warmup 3] [--passes 5] [--sizes 1024,2048,4096] [--no-detector] [--out FILE]

Legs: one pair at a time at n x n; 16 pairs at 1024 x 1024 through match_pairs (packing included) and through the ragged entry on
packed tensors; the detector's 15 views of 1024 against one shared query plane; one detect_device with the NN matcher
(tools/detector_bench.py's planted features).  Every leg: warm-up, then `passes` timings of `steps` calls with the host clock
around the calls plus a synchronise -> median, min, max in ms.  `ok`: the fused path is no slower than the eager restatement by
more than the run-to-run spread recorded here (the larger max - min of the two).  Prints and writes one JSON object.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from onepose_amd import LocalFeatureObjectDetector, NearestNeighbour, SuperPoint, synthetic  # noqa: E402
import nn_oracle as orc  # noqa: E402

PEAK_TFLOPS = 157.3
CONF = {"ratio_threshold": 0.8, "distance_threshold": 0.7, "do_mutual_check": True}
K = np.array([[1063.2, 0.0, 318.7], [0.0, 1071.9, 243.1], [0.0, 0.0, 1.0]])


def eager_side(sim, ratio, distance):
    """One direction of the reference in stock PyTorch: top 2 along the last axis, the two distance tests, match and score."""
    val, ind = sim.topk(2 if ratio else 1, dim=-1)
    dist = 2 * (1 - val)
    keep = torch.ones_like(ind[..., 0], dtype=torch.bool)
    if ratio:
        keep = keep & (dist[..., 0] <= ratio ** 2 * dist[..., 1])
    if distance:
        keep = keep & (dist[..., 0] <= distance ** 2)
    return torch.where(keep, ind[..., 0], ind.new_tensor(-1)), torch.where(keep, (val[..., 0] + 1) / 2, val.new_tensor(0))


@torch.no_grad()
def eager(d0, d1, conf=CONF):
    """The eager restatement: the similarity matrix is written once and read by both topk."""
    sim = torch.einsum("bdn,bdm->bnm", d0, d1)
    m0, s0 = eager_side(sim, conf["ratio_threshold"], conf["distance_threshold"])
    m1, s1 = eager_side(sim.transpose(1, 2), conf["ratio_threshold"], conf["distance_threshold"])
    if conf["do_mutual_check"]:
        back = torch.gather(m1, -1, m0.clamp(min=0))
        m0 = torch.where((m0 > -1) & (back == torch.arange(m0.shape[-1], device=m0.device)), m0, m0.new_tensor(-1))
    return m0, m1, s0, s1


def timed(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def legs(fns, passes, steps, warmup):
    """{name: {median, min, max}} in ms per call; the legs alternate inside every pass."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    t = {k: [] for k in fns}
    for _ in range(passes):
        for k, fn in fns.items():
            t[k].append(timed(fn, steps))
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in t.items()}


def verdict(row, fused, eager_key):
    f, e = row[fused], row[eager_key]
    spread = max(f["max"] - f["min"], e["max"] - e["min"])
    row["eager_over_fused"] = round(e["median"] / f["median"], 2)
    row["ok_no_slower_than_eager_beyond_spread"] = bool(f["median"] <= e["median"] + spread)


def agree(got, ref, what):
    """What is timed computes what the eager restatement computes (fp32 both: a near-tie may flip, a handful at most)."""
    diff = sum(int((g != r).sum()) for g, r in zip(got[:2], ref[:2]))
    total = sum(g.numel() for g in got[:2])
    assert diff <= max(2, total // 500), f"{what}: {diff} of {total} matches differ from the eager restatement"
    return diff


def profile_json(name):
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--no-detector", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nn_matcher_bench needs a GPU (there is no CPU path to time)"
    dev = torch.device("cuda:0")
    nn = NearestNeighbour(CONF)
    up = lambda x: torch.from_numpy(x).to(dev)      # noqa: E731
    sg, det = profile_json("sg_bench.json"), profile_json("det_bench.json")
    res = {"metric": "nn_matcher_ms", "conf": CONF, "steps": a.steps, "passes": a.passes, "warmup": a.warmup,
           "peak_tflops_fp32_mfma": PEAK_TFLOPS, "single": []}

    for n in (int(x) for x in a.sizes.split(",")):
        d0, d1 = (up(x)[None] for x in orc.make_pair(n, n, seed=n))
        data = {"descriptors0": d0, "descriptors1": d1}
        out = nn(data)
        diff = agree([out[k] for k in orc.OUT_KEYS], eager(d0, d1), f"{n} x {n}")
        row = {"n0": n, "n1": n, "matches_differing_from_eager": diff, "rows_matched": int((out["matches0"] > -1).sum()),
               **legs({"fused_ms": lambda: nn(data), "eager_ms": lambda: eager(d0, d1)}, a.passes, a.steps, a.warmup)}
        verdict(row, "fused_ms", "eager_ms")
        gflop = 2.0 * n * n * 256 / 1e9
        row["gflop"] = round(gflop, 3)
        row["frac_fp32_mfma_peak_whole_call"] = round(gflop / row["fused_ms"]["median"] / PEAK_TFLOPS, 4)
        ref = next((s for s in (sg or {}).get("shapes", []) if s["n0"] == n and s["n1"] == n), None)
        if ref:
            row["superglue_ms_per_pair"] = ref["ms_per_pair"]
            row["superglue_over_fused"] = round(ref["ms_per_pair"] / row["fused_ms"]["median"], 1)
        res["single"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    # 16 pairs at 1024 x 1024
    b, n = 16, 1024
    pairs = [orc.make_pair(n, n, seed=100 + i) for i in range(b)]
    items = [{"descriptors0": up(p[0])[None], "descriptors1": up(p[1])[None]} for p in pairs]
    p0, p1 = torch.cat([i["descriptors0"] for i in items]), torch.cat([i["descriptors1"] for i in items])
    got = nn.engine.match_ragged(p0, p1, [n] * b, [n] * b)
    diff = agree(got, eager(p0, p1), "16 pairs")
    row = {"pairs": b, "n0": n, "n1": n, "matches_differing_from_eager": diff,
           **legs({"match_pairs_ms": lambda: nn.match_pairs(items, max_items=b),
                   "ragged_packed_ms": lambda: nn.engine.match_ragged(p0, p1, [n] * b, [n] * b),
                   "eager_batched_ms": lambda: eager(p0, p1),
                   "eager_loop_ms": lambda: [eager(i["descriptors0"], i["descriptors1"]) for i in items]}, a.passes, a.steps, a.warmup)}
    verdict(row, "ragged_packed_ms", "eager_batched_ms")
    row["match_pairs_ok_against_eager_loop"] = bool(
        row["match_pairs_ms"]["median"] <= row["eager_loop_ms"]["median"] + max(row["match_pairs_ms"]["max"] - row["match_pairs_ms"]["min"],
                                                                                row["eager_loop_ms"]["max"] - row["eager_loop_ms"]["min"]))
    row["frac_fp32_mfma_peak_whole_call"] = round(b * 2.0 * n * n * 256 / 1e9 / row["ragged_packed_ms"]["median"] / PEAK_TFLOPS, 4)
    ref = next((r for r in (sg or {}).get("ragged", {}).get("rows", []) if (r["cap"], r["b"], r["draw"]) == (n, b, "equal")), None)
    if ref:
        row["superglue_ragged_ms_16_pairs"] = round(ref["ragged_ms_per_pair"]["median"] * b, 3)
        row["superglue_over_fused"] = round(row["superglue_ragged_ms_16_pairs"] / row["ragged_packed_ms"]["median"], 1)
    res["ragged_16_pairs"] = row
    print(json.dumps(row), file=sys.stderr, flush=True)

    # the detector's case: 15 views of 1024 against one query plane
    V = 15
    q = up(orc.make_pair(n, n, seed=200)[1])
    views = torch.cat([up(orc.make_pair(n, n, seed=201 + v)[0])[None] for v in range(V)])
    qx = q[None].expand(V, -1, -1)
    got = nn.engine.match_ragged(views, q, [n] * V, [n] * V)
    row = {"views": V, "n0": n, "n1": n, "matches_differing_from_eager": agree(got, eager(views, qx), "15 views"),
           **legs({"shared_plane_ms": lambda: nn.engine.match_ragged(views, q, [n] * V, [n] * V),
                   "eager_batched_ms": lambda: eager(views, qx)}, a.passes, a.steps, a.warmup)}
    verdict(row, "shared_plane_ms", "eager_batched_ms")
    row["frac_fp32_mfma_peak_whole_call"] = round(V * 2.0 * n * n * 256 / 1e9 / row["shared_plane_ms"]["median"] / PEAK_TFLOPS, 4)
    ref = next((s for s in (det or {}).get("shapes", []) if s["views"] == V and s["query_keypoints"] == n), None)
    if ref:
        row["superglue_ragged_ms_15_views"] = ref["matcher_ragged_ms"]["median"]
        row["superglue_over_fused"] = round(ref["matcher_ragged_ms"]["median"] / row["shared_plane_ms"]["median"], 1)
    res["detector_15_views_shared_plane"] = row
    print(json.dumps(row), file=sys.stderr, flush=True)

    if not a.no_detector:      # one whole detect with the NN matcher, on detector_bench's planted features
        from detector_bench import PlantedFeatures, planted_features
        import detector_oracle as do
        h, w = 480, 640
        ext = SuperPoint({"nms_radius": 4, "max_keypoints": n}).eval()
        ext.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_spp_state_dict(0).items()}, strict=True)
        frame = torch.from_numpy(do.to_u8(synthetic.make_image(1, h, w, 100)).astype(np.float32) / np.float32(255)).to(dev)
        refs = [torch.from_numpy(synthetic.make_image(1, h, w, 101 + i)).to(dev) for i in range(V)]
        d = LocalFeatureObjectDetector(PlantedFeatures(ext, *planted_features(V, n, h, w, dev)), nn, ref_images=refs)
        d.detect_device(frame, K, 512)
        info = d.last["info"].cpu().numpy()
        row = {"frame": f"{h}x{w}", "views": V, "keypoints": n, "matches_per_view": info[:, 1].tolist(), "inliers_per_view": info[:, 3].tolist(),
               **legs({"detect_device_ms": lambda: d.detect_device(frame, K, 512)}, a.passes, a.steps, a.warmup)}
        row["frames_per_s"] = round(1e3 / row["detect_device_ms"]["median"], 1)
        ref = next((s for s in (det or {}).get("shapes", []) if s["frame"] == f"{h}x{w}"), None)
        if ref:
            row["superglue_detect_device_ms"] = ref["detect_device_ms"]["median"]
            row["superglue_over_nn"] = round(ref["detect_device_ms"]["median"] / row["detect_device_ms"]["median"], 1)
        row["note"] = "match quality is traded for speed; no accuracy comparison against SuperGlue was made (planted features with identical descriptors)"
        res["detector_detect_device"] = row
        print(json.dumps(row), file=sys.stderr, flush=True)

    res["all_ok"] = bool(all(r["ok_no_slower_than_eager_beyond_spread"] for r in res["single"])
                         and res["ragged_16_pairs"]["ok_no_slower_than_eager_beyond_spread"]
                         and res["ragged_16_pairs"]["match_pairs_ok_against_eager_loop"]
                         and res["detector_15_views_shared_plane"]["ok_no_slower_than_eager_beyond_spread"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
