"""Placement tests of the object database builder and the bundle adjustment (include/mapping/mapping.h, bundle_adjust.h):
map_verify_matches, map_triangulate_tracks, map_filter_points, map_merge_points, map_gather_descriptors and ba_solve with every
device argument an exact piece of a guarded arena (tests/arena.py) under the fills 0xFF and 0x00; the workspaces are exactly
map_workspace_bytes / ba_workspace_bytes.  Where the header calls rows "undefined" or says nothing is written past a count, the rows
it says are written are compared across the two fills.  Also map_track_length_threshold and the stage entries ba_linearize ->
ba_normal_blocks -> ba_step.  Every case runs a second time with each call captured and replayed (arena.run_captured).  Bitwise
comparisons only; the oracle comparisons stay in
tests/test_map_hip.py and tests/test_ba_hip.py."""
import ctypes

import numpy as np
import pytest
import torch

import ba_cases as bc
import map_cases as mc
import mapping_oracle as mo
from arena import captured_twin, run_placement
from onepose_amd import _native_map

BINDING = _native_map
ROLES = {
    "map_verify_matches": dict(kpts="in", kpt_offsets="in", cams="in", pair_images="in", match_offsets="in", matches0="in",
                               out_matches="out", counts="out"),
    "map_triangulate_tracks": dict(track_offsets="in", obs_image="in", obs_xy="in", cams="in", xyz="out", inlier_mask="out", info="out",
                                   lengths="out"),
    "map_filter_points": dict(xyz="in", lengths="in", threshold="in", kept_ids="out", kept_xyz="out", count="out"),
    "map_merge_points": dict(xyz32="in", merged_xyz="out", member_offsets="out", members="out", count="out", workspace="scratch"),
    "map_gather_descriptors": dict(desc_table="in", score_table="in", n_kpts="in", point_offsets="in", obs_image="in", obs_kpt="in",
                                   collect_desc="out", collect_scores="out", idxs="out", mean_desc="out", mean_scores="out"),
    # cams and points are updated in place: ``double*`` in the header, placed with their start values
    "ba_solve": dict(cams="out", intr="in", points="out", obs_cam="in", obs_pt="in", obs_xy="in", cam_fixed="in", pt_fixed="in",
                     trace="out", summary="out", workspace="scratch"),
    "ba_linearize": dict(cams="in", intr="in", points="in", obs_cam="in", obs_pt="in", obs_xy="in", r="out", Jc="out", Jp="out"),
    "ba_normal_blocks": dict(r="in", Jc="in", Jp="in", obs_cam="in", obs_pt="in", cam_fixed="in", pt_fixed="in", U="out", V="out", g_c="out",
                             g_p="out", cost_cam="out", workspace="scratch"),
    "ba_step": dict(U="in", V="in", g_c="in", g_p="in", r="in", Jc="in", Jp="in", obs_cam="in", obs_pt="in", cam_fixed="in", pt_fixed="in",
                    delta_c="out", delta_p="out", model_decrease="out", workspace="scratch"),
    "map_track_length_threshold": dict(lengths="in", threshold="out"),
}
T = dict(max_epipolar_error=4.0, min_pair_inliers=15, max_reproj_error=4.0, min_tri_angle=1.5, max_hypotheses=120,
         refine_iterations=10, dist_threshold=1e-3, seed=0)       # onepose_amd.mapping.THRESHOLDS
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64


def tensor(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def outputs(mem, spec):
    return {nm: mem.place(torch.empty(s, dtype=t), "out", nm) for nm, s, t in spec}


@pytest.mark.parametrize("P", [mc.VERIFY_PAIRS[0], mc.VERIFY_PAIRS[-1]])
def test_verify_matches(P, run=run_placement):
    b = mc.verify_batch(P)
    V, total = len(b["cams"]), int(b["match_offsets"][-1])

    def body(mem):
        ins = [mem.place(tensor(b[k], t), "in", k) for k, t in (("kpts", F32), ("kpt_offsets", I32), ("cams", F64))]
        more = [mem.place(tensor(b[k], t), "in", k) for k, t in (("pair_images", I32), ("match_offsets", I32), ("matches0", I64))]
        out = outputs(mem, (("out_matches", (max(1, total), 2), I32), ("counts", (P,), I32)))
        mem.call(BINDING, "map_verify_matches", *ins, V, *more, P, T["max_epipolar_error"], T["min_pair_inliers"], *out.values())
        # the header: the survivors of pair p are compacted from row match_offsets[p]; nothing is said of the rows behind them
        rows = [out["out_matches"][base:base + n] for base, n in zip(b["match_offsets"][:-1].tolist(), out["counts"].tolist())]
        return out, {"out_matches": torch.cat(rows)}

    got = run(body, DEV, ROLES)
    assert got["counts"].tolist() == [c["count"] for c in b["pairs"]]


@pytest.mark.parametrize("m", [63, 64, 65, 200])
def test_triangulate_tracks(m, run=run_placement):
    """Every kind of track at the wave edge (63, 64, 65: one wave a track up to 64) and on the workgroup path (65, 200)."""
    cases = [mc.track_case(m, kind, 1) for kind in mc.TRACK_KINDS]
    b = mc.track_batch(cases)
    n_tracks, M, V = len(cases), len(b["obs_image"]), len(b["cams"])

    def body(mem):
        ins = [mem.place(tensor(b[k], t), "in", k) for k, t in (("track_offsets", I32), ("obs_image", I32), ("obs_xy", F32), ("cams", F64))]
        out = outputs(mem, (("xyz", (n_tracks, 3), F64), ("inlier_mask", (M,), I32), ("info", (n_tracks, 4), I32), ("lengths", (n_tracks,), I32)))
        mem.call(BINDING, "map_triangulate_tracks", *ins, n_tracks, V, b["max_len"], T["max_reproj_error"], T["min_tri_angle"], T["max_hypotheses"],
                 T["refine_iterations"], T["seed"], *out.values())
        return out

    got = run(body, DEV, ROLES)
    assert got["info"].tolist() == [list(c["result"]["info"]) for c in cases]


@pytest.mark.parametrize("n", [mc.POINT_COUNTS[0], mc.POINT_COUNTS[-1]])
def test_filter_and_merge_points(n, run=run_placement):
    """map_filter_points at the oracle's threshold, then map_merge_points on the points the oracle keeps (its fp32 coordinates are
    the kernel's bit for bit, tests/test_map_hip.py)."""
    c = mc.points_case(n)
    thr = mo.track_length_threshold(c["lengths"], c["max_num_kp3d"])
    box = (ctypes.c_float * 24)(*np.asarray(c["box"], np.float64).astype(np.float32).reshape(24).tolist())
    ref_ids, ref_xyz = mo.filter_points(c["xyz"], c["lengths"], thr, c["box"])

    def filter_body(mem):
        xyz, lengths, threshold = mem.place(tensor(c["xyz"], F64), "in", "xyz"), mem.place(tensor(c["lengths"], I32), "in", "lengths"), \
            mem.place(torch.tensor([thr], dtype=I32), "in", "threshold")
        out = outputs(mem, (("kept_ids", (n,), I32), ("kept_xyz", (n, 3), F32), ("count", (1,), I32)))
        mem.call(BINDING, "map_filter_points", xyz, lengths, n, threshold, box, *out.values())
        k = int(out["count"])
        return out, {"kept_ids": out["kept_ids"][:k], "kept_xyz": out["kept_xyz"][:k]}          # the kept points; nothing is said of the rest

    got = run(filter_body, DEV, ROLES)
    k = int(got["count"])
    assert got["kept_ids"][:k].tolist() == ref_ids.tolist()
    if k == 0:
        return
    nbytes = BINDING.load().map_workspace_bytes(k)
    assert nbytes > 0

    def merge_body(mem):
        xyz32 = mem.place(tensor(ref_xyz, F32), "in", "xyz32")
        out = outputs(mem, (("merged_xyz", (k, 3), F32), ("member_offsets", (k + 1,), I32), ("members", (k,), I32), ("count", (1,), I32)))
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "map_merge_points", xyz32, k, T["dist_threshold"], *out.values(), ws, nbytes)
        q = int(out["count"])
        # the header: member_offsets "entries past the merged count undefined"; members: ascending positions per merged point
        offs = out["member_offsets"][:q + 1]
        return out, {"merged_xyz": out["merged_xyz"][:q], "member_offsets": offs, "members": out["members"][:int(offs[-1])]}

    merged = run(merge_body, DEV, ROLES)
    assert int(merged["count"]) == len(mo.merge_points(ref_xyz)[1])


@pytest.mark.parametrize("n", [mc.POINT_COUNTS[0], mc.POINT_COUNTS[-1]])
def test_track_length_threshold(n, run=run_placement):
    """the lengths of map_cases.points_case (0 = no point, 2 .. 12) against the oracle's threshold"""
    c = mc.points_case(n)

    def body(mem):
        lengths = mem.place(tensor(c["lengths"], I32), "in", "lengths")
        threshold = mem.place(torch.empty(1, dtype=I32), "out", "threshold")
        mem.call(BINDING, "map_track_length_threshold", lengths, n, c["max_num_kp3d"], threshold)
        return dict(threshold=threshold)

    got = run(body, DEV, ROLES)
    assert got["threshold"].item() == mo.track_length_threshold(c["lengths"], c["max_num_kp3d"])


def test_gather_descriptors(run=run_placement):
    """map_cases.gather_case(): every image's descriptors and scores are pieces of their own, reached through the two pointer tables."""
    c = mc.gather_case()
    dim, V = c["features"][0]["descriptors"].shape[0], len(c["features"])
    N, K = len(c["point_offsets"]) - 1, len(c["obs_image"])

    def body(mem):
        desc = [mem.place(tensor(f["descriptors"], F32), "in", f"descriptors[{v}]") for v, f in enumerate(c["features"])]
        scores = [mem.place(tensor(f["scores"], F32), "in", f"scores[{v}]") for v, f in enumerate(c["features"])]
        dtab = mem.place(torch.tensor([d.data_ptr() for d in desc], dtype=I64), "in", "desc_table")
        stab = mem.place(torch.tensor([s.data_ptr() for s in scores], dtype=I64), "in", "score_table")
        n_kpts = mem.place(torch.tensor([d.shape[1] for d in desc], dtype=I32), "in", "n_kpts")
        ins = [mem.place(tensor(c[k], I32), "in", k) for k in ("point_offsets", "obs_image", "obs_kpt")]
        out = outputs(mem, (("collect_desc", (K, dim), F32), ("collect_scores", (K,), F32), ("idxs", (N,), I64), ("mean_desc", (N, dim), F64),
                            ("mean_scores", (N,), F64)))
        mem.call(BINDING, "map_gather_descriptors", dtab, stab, n_kpts, V, *ins, N, dim, *out.values())
        return out

    got = run(body, DEV, ROLES)
    assert got["idxs"].tolist() == mc.GATHER_COUNTS + [3, 3]


def ba_problems():
    return {"blocks_257": lambda: (bc.blocks_case(bc.CAMERA_CHUNK + 1), 5), "wide_32x48": lambda: (bc.wide_case(32, 48, tuple(range(48)), 51)[0], 3)}


@pytest.mark.parametrize("name", sorted(ba_problems()))
def test_ba_solve(name, run=run_placement):
    """One observation over a pass of the per-camera kernels (camera 0 has BA_CAMERA_CHUNK + 1), nothing fixed, the reference's 5 / 5
    iterations; and the 32-camera limit with its gauge fixed, 3 / 3 iterations as tests/test_ba_hip.py runs it."""
    pb, iterations = ba_problems()[name]()
    nbytes = BINDING.load().ba_workspace_bytes(pb.C, pb.P, pb.M)
    assert nbytes > 0

    def body(mem):
        cams = mem.place(tensor(pb.cams, F64), "out", "cams", copy=True)
        intr = mem.place(tensor(pb.intr, F64), "in", "intr")
        points = mem.place(tensor(pb.points, F64), "out", "points", copy=True)
        obs = [mem.place(tensor(a, t), "in", nm) for a, t, nm in ((pb.obs_cam, I32, "obs_cam"), (pb.obs_pt, I32, "obs_pt"), (pb.obs_xy, F64, "obs_xy"))]
        fixed = [None if a is None else mem.place(tensor(a, I32), "in", nm) for a, nm in ((pb.cam_fixed, "cam_fixed"), (pb.pt_fixed, "pt_fixed"))]
        out = outputs(mem, (("trace", (iterations, _native_map.BA_TRACE_COLUMNS), F64), ("summary", (_native_map.BA_SUMMARY_ENTRIES,), F64)))
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "ba_solve", cams, intr, points, *obs, *fixed, pb.C, pb.P, pb.M, iterations, iterations, *out.values(), ws, nbytes)
        return dict(out, cams=cams, points=points)

    got = run(body, DEV, ROLES)
    assert got["summary"][5] == _native_map.BA_STATUS_OK and got["summary"][1] <= got["summary"][0]


def test_ba_stage_entries(run=run_placement):
    """ba_linearize, then ba_normal_blocks on its r, Jc, Jp, then ba_step at mu = 1e4 (where ba_solve starts) on the blocks of that:
    the outputs of one stage are the ``const`` inputs of the next, and protected there.  blocks_case(BA_CAMERA_CHUNK + 1): camera 0
    has one observation over a pass of the per-camera kernels, camera 2 and point 0 have none; nothing fixed (NULL masks)."""
    pb = bc.blocks_case(bc.CAMERA_CHUNK + 1)
    C, P, M = pb.C, pb.P, pb.M
    nbytes = BINDING.load().ba_workspace_bytes(C, P, M)
    assert nbytes > 0

    def body(mem):
        cams, intr, points = (mem.place(tensor(a, F64), "in", nm) for a, nm in ((pb.cams, "cams"), (pb.intr, "intr"), (pb.points, "points")))
        obs_cam, obs_pt = mem.place(tensor(pb.obs_cam, I32), "in", "obs_cam"), mem.place(tensor(pb.obs_pt, I32), "in", "obs_pt")
        obs_xy = mem.place(tensor(pb.obs_xy, F64), "in", "obs_xy")
        lin = outputs(mem, (("r", (M, 2), F64), ("Jc", (M, 2, 6), F64), ("Jp", (M, 2, 3), F64)))
        blocks = outputs(mem, (("U", (C, 6, 6), F64), ("V", (P, 3, 3), F64), ("g_c", (C, 6), F64), ("g_p", (P, 3), F64), ("cost_cam", (C,), F64)))
        step = outputs(mem, (("delta_c", (C, 6), F64), ("delta_p", (P, 3), F64), ("model_decrease", (1,), F64)))
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "ba_linearize", cams, intr, points, obs_cam, obs_pt, obs_xy, C, P, M, *lin.values())
        mem.call(BINDING, "ba_normal_blocks", *lin.values(), obs_cam, obs_pt, None, None, C, P, M, *blocks.values(), ws, nbytes)
        U, V, g_c, g_p, _ = blocks.values()
        mem.call(BINDING, "ba_step", U, V, g_c, g_p, *lin.values(), obs_cam, obs_pt, None, None, C, P, M, 1e4, *step.values(), ws, nbytes)
        return {**lin, **blocks, **step}

    got = run(body, DEV, ROLES)
    assert not any(torch.isnan(v).any() for v in got.values()) and got["model_decrease"].item() > 0
    # the header: zeros for an unobserved variable, exactly 0 in the step
    assert not got["U"][2].any() and not got["V"][0].any() and not got["delta_c"][2].any() and not got["delta_p"][0].any()


# every case again with each library call captured in a graph and replayed (arena.run_captured): the stream contract
test_verify_matches_captured = captured_twin(test_verify_matches)
test_triangulate_tracks_captured = captured_twin(test_triangulate_tracks)
test_filter_and_merge_points_captured = captured_twin(test_filter_and_merge_points)
test_gather_descriptors_captured = captured_twin(test_gather_descriptors)
test_ba_solve_captured = captured_twin(test_ba_solve)
test_track_length_threshold_captured = captured_twin(test_track_length_threshold)
test_ba_stage_entries_captured = captured_twin(test_ba_stage_entries)
