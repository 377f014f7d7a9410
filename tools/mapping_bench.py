"""Per-stage times of the object database builder's HIP tail (libmap_hip.so) on a synthetic scan of realistic size, beside the
time of the same stage through the numpy oracle (tests/mapping_oracle.py) on the host -- a numpy yardstick, what a user of the
commit before this library would have had to run; it is NOT COLMAP and no ratio against COLMAP is claimed.

    python tools/mapping_bench.py [--views 100] [--points 52000] [--dropout 0.925] [--neighbours 10] [--passes 7] [--out profiles/map_bench.json]

The defaults give about 100 views of at most 4096 keypoints (SuperPoint's cap in the builder), 1000 pairs and 50 k tracks.

Each stage: 2 warm-up calls, then ``--passes`` timed calls (host clock around the call and a device synchronisation); median, min
and max are reported.  The oracle's triangulation is timed on every 25th track and scaled (labelled so in the output)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapping_oracle as mo  # noqa: E402
from onepose_amd import mapping, synthetic  # noqa: E402


def timed(fn, passes, warmup=2):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, round((time.perf_counter() - t0) * 1e3, 2)


def matching_stage(feats, pairs, dev, passes):
    """The matcher of build_from_features on a subset of the scan's pairs: one forward per pair against ragged batches of 16
    (SuperGlue.match_pairs), ms per pair over the passes; the matches are asserted equal."""
    import time
    from onepose_amd import SuperGlue
    sg = SuperGlue({"GNN_layers": ["self", "cross"] * 9, "sinkhorn_iterations": 100, "match_threshold": 0.7}).eval()
    sg.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_superglue_passthrough_state_dict(10, 18).items()}, strict=True)
    sg = sg.to(dev)
    t = {k: [{n: torch.from_numpy(np.ascontiguousarray(f[n])).to(dev)[None] for n in ("keypoints", "scores", "descriptors")} for f in feats]
         for k in (0,)}[0]
    items = [{"keypoints0": t[i]["keypoints"], "scores0": t[i]["scores"], "descriptors0": t[i]["descriptors"], "keypoints1": t[j]["keypoints"],
              "scores1": t[j]["scores"], "descriptors1": t[j]["descriptors"], "image0": torch.empty(1, 1, 480, 640, device="meta"),
              "image1": torch.empty(1, 1, 480, 640, device="meta")} for i, j in pairs]
    loop = lambda: [sg(d)["matches0"] for d in items]                 # noqa: E731
    batched = lambda: [r["matches0"] for r in sg.match_pairs(items, max_items=16)]     # noqa: E731
    assert all(torch.equal(x, y) for x, y in zip(loop(), batched()))
    out = {"pairs": len(items), "keypoints_per_image": [min(int(d["keypoints0"].shape[1]) for d in items), max(int(d["keypoints0"].shape[1]) for d in items)]}
    for name, fn in (("loop_ms_per_pair", loop), ("pair_batch_16_ms_per_pair", batched)):
        ts = []
        for _ in range(passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / len(items) * 1e3)
        ts.sort()
        out[name] = {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}
    out["ragged_beats_loop_by_more_than_its_spread"] = bool(out["loop_ms_per_pair"]["median"] - out["pair_batch_16_ms_per_pair"]["median"]
                                                            > out["loop_ms_per_pair"]["max"] - out["loop_ms_per_pair"]["min"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--points", type=int, default=52000)
    ap.add_argument("--dropout", type=float, default=0.925, help="share of the visible points a view does not detect")
    ap.add_argument("--distract", type=int, default=200, help="unmatched keypoints per view")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--match-pairs", type=int, default=32, help="image pairs of the scan the matching stage is timed on (0: skip)")
    ap.add_argument("--match-passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_bench.json"))
    a = ap.parse_args(argv)
    scene = synthetic.make_map_scene(n_points=a.points, n_views=a.views, hw=(480, 640), seed=0, noise_px=0.3, wrong_frac=0.05,
                                     n_distract=a.distract, pairs_per_view=a.neighbours, dropout=a.dropout)
    feats, pm = scene["features"], scene["pair_matches"]
    tail = mapping.MapTail("cuda:0")
    dev = tail.device
    n_kpts = [len(f["keypoints"]) for f in feats]
    kpt_offsets = np.concatenate([[0], np.cumsum(n_kpts)]).astype(np.int32)
    kpts = torch.from_numpy(np.concatenate([f["keypoints"] for f in feats])).to(dev)
    cams_h = mapping.make_cams(scene["Ks"], scene["poses"])
    cams = torch.from_numpy(cams_h).to(dev)
    pair_images = torch.tensor([(i, j) for i, j, _ in pm], dtype=torch.int32, device=dev)
    match_offsets_h = np.concatenate([[0], np.cumsum([len(m) for _, _, m in pm])]).astype(np.int32)
    match_offsets = torch.from_numpy(match_offsets_h).to(dev)
    matches0 = torch.from_numpy(np.concatenate([m for _, _, m in pm])).to(dev)
    res = {"views": a.views, "pairs": len(pm), "keypoints": int(kpt_offsets[-1]), "max_keypoints_per_view": int(max(n_kpts)), "device": torch.cuda.get_device_name(0), "stages": {}}

    (out, counts), res["stages"]["verify"] = timed(lambda: tail.verify(kpts, kpt_offsets, cams, pair_images, match_offsets, matches0), a.passes)
    out_h, counts_h = out.cpu().numpy(), counts.cpu().numpy()
    survivors = [out_h[match_offsets_h[p]:match_offsets_h[p] + counts_h[p]] for p in range(len(pm))]
    (track_offsets, obs_image, obs_kpt), res["stages"]["build_tracks_host"] = timed(
        lambda: mapping.build_tracks(n_kpts, pair_images.cpu().numpy(), survivors), 3, warmup=0)
    T = len(track_offsets) - 1
    res.update(tracks=T, observations=int(len(obs_image)), verified_matches=int(counts_h.sum()))
    obs_xy = kpts[torch.from_numpy(kpt_offsets[obs_image].astype(np.int64) + obs_kpt).to(dev)]
    to, oi = torch.from_numpy(track_offsets).to(dev), torch.from_numpy(obs_image).to(dev)
    max_len = int(np.diff(track_offsets).max())
    (xyz, mask, info, lengths), res["stages"]["triangulate"] = timed(lambda: tail.triangulate(to, oi, obs_xy, cams, max_len), a.passes)
    thr, res["stages"]["track_length_threshold"] = timed(lambda: tail.track_length_threshold(lengths, 2500), a.passes)
    (ids, kept), res["stages"]["filter_points"] = timed(lambda: tail.filter_points(xyz, lengths, thr, scene["box"]), a.passes)
    (merged, moffs, members), res["stages"]["merge_points"] = timed(lambda: tail.merge_points(kept), a.passes)
    po, gi, gk = mapping.point_observations(track_offsets, obs_image, obs_kpt, mask.cpu().numpy(), ids.cpu().numpy(), moffs.cpu().numpy(),
                                            members.cpu().numpy())
    descs = [torch.from_numpy(f["descriptors"]).to(dev) for f in feats]
    scores = [torch.from_numpy(f["scores"]).to(dev) for f in feats]
    _, res["stages"]["gather_descriptors"] = timed(lambda: tail.gather(descs, scores, po, gi, gk), a.passes)
    res.update(points_ok=int(info[:, 0].sum()), threshold=int(thr), kept=int(ids.shape[0]), merged=int(merged.shape[0]), collected=int(len(gi)),
               max_track_length=max_len)

    # the numpy yardstick on the host
    y = {}
    _, y["verify_ms"] = host_ms(lambda: [mo.verify_pair(feats[i]["keypoints"], feats[j]["keypoints"], cams_h[i], cams_h[j], m) for i, j, m in pm])
    sub = range(0, T, 25)
    xy_h = obs_xy.cpu().numpy()
    _, t_sub = host_ms(lambda: [mo.triangulate_track(cams_h[obs_image[track_offsets[t]:track_offsets[t + 1]]], xy_h[track_offsets[t]:track_offsets[t + 1]])
                                for t in sub])
    y["triangulate_ms_scaled_from_every_25th_track"] = round(t_sub * T / max(1, len(sub)), 1)
    xyz_h, len_h = xyz.cpu().numpy(), lengths.cpu().numpy()
    t_ref, y["track_length_threshold_ms"] = host_ms(lambda: mo.track_length_threshold(len_h, 2500))
    (ids_ref, kept_ref), y["filter_points_ms"] = host_ms(lambda: mo.filter_points(xyz_h, len_h, t_ref, scene["box"]))
    _, y["merge_points_ms"] = host_ms(lambda: mo.merge_points(kept_ref))
    _, y["gather_descriptors_ms"] = host_ms(lambda: mo.gather_descriptors(feats, po, gi, gk))
    res["numpy_yardstick_host"] = y
    res["tail_median_ms_total"] = round(sum(v["median_ms"] for k, v in res["stages"].items()), 3)
    if a.match_pairs:
        res["matching"] = matching_stage(feats, [(i, j) for i, j, _ in pm[:a.match_pairs]], dev, a.match_passes)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
