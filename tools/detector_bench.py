"""2D object detector throughput on one GPU: detect_device (SuperPoint -> V SuperGlue forwards -> HIP tail) per frame, the time
split by HIP events, and the tail against what a user had to do without it: matcher outputs copied to the host and the numpy
restatement (tests/detector_oracle.py, same hash and hypothesis count) run there.

    python tools/detector_bench.py [--steps 10] [--warmup 3] [--passes 5] [--views 15] [--shapes 480x640,512x512] [--out FILE]

Prints (and writes to --out, default profiles/det_bench.json) one JSON object: per frame shape frames/s of detect_device, median
ms and min-max over the passes of extractor / V matcher forwards / tail, the host tail's ms, their ratio and the tail's share
of a whole detect.
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

from onepose_amd import LocalFeatureObjectDetector, SuperGlue, SuperPoint, synthetic  # noqa: E402
import detector_oracle as do  # noqa: E402

OUTDOOR = {"GNN_layers": ["self", "cross"] * 9, "sinkhorn_iterations": 100, "match_threshold": 0.2}
K = np.array([[1063.2, 0.0, 318.7], [0.0, 1071.9, 243.1], [0.0, 0.0, 1.0]])


class PlantedFeatures(torch.nn.Module):
    """Runs the real extractor on every image (so its time is in the figures) and returns prepared features instead: the
    synthetic-weight SuperPoint's descriptors do not discriminate, SuperGlue then returns no match at all and the tail would be
    timed on its all-views-fail branch.  The prepared views hold the frame's keypoints under a similarity each, with the
    frame's descriptors (about 60 % of them) -- what a trained extractor gives on views of one object."""

    def __init__(self, real, views, query):
        super().__init__()
        self.real, self.views, self.query, self.calls = real, views, query, 0

    def forward(self, img):
        self.real(img)
        f = self.views[self.calls] if self.calls < len(self.views) else self.query
        self.calls += 1
        return {k: [v] for k, v in f.items()}


def planted_features(V, n, h, w, dev):
    rs = np.random.RandomState(5)

    def feats(kpts):
        d = rs.normal(size=(256, len(kpts))).astype(np.float32)
        return {"keypoints": kpts.astype(np.float32), "scores": rs.uniform(0.1, 0.9, len(kpts)).astype(np.float32),
                "descriptors": d / np.linalg.norm(d, axis=0, keepdims=True)}

    q = feats(np.stack([rs.uniform(0, w - 1, n), rs.uniform(0, h - 1, n)], -1))
    views = []
    for v in range(V):
        f = feats(np.stack([rs.uniform(0, w - 1, n), rs.uniform(0, h - 1, n)], -1))
        k = int(n * rs.uniform(0.45, 0.75))
        p0, p1 = rs.permutation(n)[:k], rs.permutation(n)[:k]
        ang, sc, t = rs.uniform(-0.5, 0.5), rs.uniform(0.6, 1.5), rs.uniform(-40, 120, 2)
        R = sc * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        f["keypoints"][p0] = ((q["keypoints"][p1] - t) @ np.linalg.inv(R).T + rs.normal(0, 1.0, (k, 2))).astype(np.float32)
        f["descriptors"][:, p0] = q["descriptors"][:, p1]
        views.append(f)
    up = lambda f: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in f.items()}      # noqa: E731
    return [up(f) for f in views], up(q)


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def host_tail(det, kpts1, frame, crop):
    """The parent commit's route: every matcher output to the host (local_feature_2D_detector.py:85-91), geometry in numpy."""
    k1 = kpts1.cpu().numpy()
    k0 = [v["keypoints"].cpu().numpy() for v in det.db_dict.values()]
    m0 = [det.matches0[i, :len(k)].cpu().numpy() for i, k in enumerate(k0)]
    tail = do.detect_tail(k0, m0, k1, [tuple(v["size"]) for v in det.db_dict.values()], tuple(frame.shape[-2:]),
                          iterations=det.iterations, seed=det.seed)
    u8 = do.to_u8(frame[0, 0].cpu().numpy())
    return tail, do.crop_resize(u8, tail["bbox"], crop), do.k_crop(tail["bbox"], K, crop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--views", type=int, default=15)
    ap.add_argument("--shapes", default="480x640,512x512")
    ap.add_argument("--max-keypoints", type=int, default=1024)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "detector_bench needs a GPU (there is no CPU path to time)"
    dev = torch.device("cuda:0")
    ext = SuperPoint({"nms_radius": 4, "max_keypoints": a.max_keypoints}).eval()
    ext.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_spp_state_dict(0).items()}, strict=True)
    sg = SuperGlue(OUTDOOR).eval()
    # pass-through weights: equal descriptors survive the 18 layers, so the planted views really match the frame
    sg.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_superglue_passthrough_state_dict(10, 18).items()},
                       strict=True)
    rows = []
    for shp in a.shapes.split(","):
        h, w = (int(x) for x in shp.split("x"))
        frame = torch.from_numpy(do.to_u8(synthetic.make_image(1, h, w, 100)).astype(np.float32) / np.float32(255)).to(dev)
        refs = [torch.from_numpy(synthetic.make_image(1, h, w, 101 + i)).to(dev) for i in range(a.views)]
        planted = PlantedFeatures(ext, *planted_features(a.views, a.max_keypoints, h, w, dev))
        det = LocalFeatureObjectDetector(planted, sg, ref_images=refs)
        ext_run = planted
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

        def staged():
            f = det._check_frame(frame)
            ev[0].record()
            d = ext_run(f)
            k1, s1, d1 = d["keypoints"][0], d["scores"][0], d["descriptors"][0].contiguous()
            ev[1].record()
            det._match_views(k1, s1, d1, f.shape[-2:])
            ev[2].record()
            out = det._tail(k1, f.shape[-2:])
            crop, K_crop, info = det.crop_device(f, out["bbox"], K, a.crop)
            ev[3].record()
            return k1, out, crop, K_crop

        for _ in range(a.warmup):
            k1, out, crop, K_crop = staged()
            det.detect_device(frame, K, a.crop)
        torch.cuda.synchronize()
        # what is timed computes what the host route computes
        tail, ref_crop, ref_K = host_tail(det, k1, frame, a.crop)
        assert np.array_equal(out["bbox"].cpu().numpy(), tail["bbox"]) and np.array_equal(out["info"].cpu().numpy(), tail["info"])
        if tail["bbox"][2] > tail["bbox"][0] and tail["bbox"][3] > tail["bbox"][1]:
            assert crop[0, 0].cpu().numpy().tobytes() == ref_crop.tobytes() and K_crop.cpu().numpy().tobytes() == ref_K.tobytes()
        t_ext, t_match, t_tail, t_host, t_whole, t_loop, t_ragged = [], [], [], [], [], [], []
        qd = ext_run(det._check_frame(frame))
        q1 = (qd["keypoints"][0], qd["scores"][0], qd["descriptors"][0].contiguous())
        for _ in range(a.passes):                      # the two routes alternate inside every pass
            e, m, t = [], [], []
            for _ in range(a.steps):
                staged()
                torch.cuda.synchronize()
                e.append(ev[0].elapsed_time(ev[1]))
                m.append(ev[1].elapsed_time(ev[2]))
                t.append(ev[2].elapsed_time(ev[3]))
            t_ext.append(statistics.mean(e))
            t_match.append(statistics.mean(m))
            t_tail.append(statistics.mean(t))
            t0 = time.perf_counter()
            for _ in range(max(1, a.steps // 5)):
                host_tail(det, k1, frame, a.crop)
            t_host.append((time.perf_counter() - t0) / max(1, a.steps // 5) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                det.detect_device(frame, K, a.crop)
            torch.cuda.synchronize()
            t_whole.append((time.perf_counter() - t0) / a.steps * 1e3)
            for flag, acc in ((False, t_loop), (True, t_ragged)):      # the matcher alone: one forward per view / one ragged batch
                det.ragged = flag
                det._match_views(*q1, frame.shape[-2:])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    det._match_views(*q1, frame.shape[-2:])
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) / a.steps * 1e3)
        info = out["info"].cpu().numpy()
        whole = statistics.median(t_whole)
        rows.append({"frame": f"{h}x{w}", "views": a.views, "query_keypoints": int(k1.shape[0]), "ref_keypoints": det.n0_host,
                     "matches_per_view": info[:, 1].tolist(), "inliers_per_view": info[:, 3].tolist(), "iterations": det.iterations,
                     "detect_device_ms": spread(t_whole), "frames_per_s": round(1e3 / whole, 2),
                     "extractor_ms": spread(t_ext), "matcher_forwards_ms": spread(t_match), "tail_ms": spread(t_tail),
                     "host_tail_ms": spread(t_host), "matcher_loop_ms": spread(t_loop), "matcher_ragged_ms": spread(t_ragged),
                     "ragged_beats_loop_by_more_than_its_spread": bool(
                         statistics.median(t_loop) - statistics.median(t_ragged) > max(t_loop) - min(t_loop)),
                     "host_over_native_tail": round(statistics.median(t_host) / statistics.median(t_tail), 1),
                     "tail_share_of_detect": round(statistics.median(t_tail) / whole, 4)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    res = {"metric": "detector_frames_per_s", "matcher": "SuperGlue outdoor config, pass-through synthetic weights", "features": "SuperPoint runs and is timed; its outputs are replaced by planted features (see PlantedFeatures)", "steps": a.steps,
           "passes": a.passes, "warmup": a.warmup, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
