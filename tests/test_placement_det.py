"""Placement tests of the detector tail and the flow step (include/detector/detector.h, flow.h): det_affine_partial_from_matches,
det_bbox_vote, det_crop_resize, flow_build_pyramid, flow_track and flow_reproj_mean with every device argument an exact piece of a
guarded arena (tests/arena.py) under the fills 0xFF and 0x00; the workspaces are exactly det_workspace_bytes / flow_workspace_bytes,
the pyramids exactly flow_pyramid_bytes; det_affine_partial_ransac, the points form, view by view.  Every case runs a second time with
each call captured and replayed (arena.run_captured).  Bitwise comparisons only; the oracle comparisons stay in tests/test_det_hip.py and
tests/test_flow_hip.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import det_cases as dc
import detector_oracle as do
import flow_cases as fc
import flow_oracle as fo
from arena import captured_twin, run_placement
from onepose_amd import _native_det

BINDING = _native_det
ROLES = {
    "det_affine_partial_ransac": dict(src="in", dst="in", affine="out", inlier_mask="out", info="out", workspace="scratch"),
    "det_affine_partial_from_matches": dict(kpts0="in", n0="in", matches0="in", kpts1="in", affine="out", inlier_mask="out", info="out",
                                            workspace="scratch"),
    "det_bbox_vote": dict(affine="in", info="in", hw0="in", boxes="out", bbox="out", best_view="out"),
    "det_crop_resize": dict(image_u8="in", bbox="in", out="out", K_crop="out", info="out"),
    "flow_build_pyramid": dict(image_u8="in", pyramid="out"),
    "flow_track": dict(pyramid_i="in", pyramid_j="in", pts="in", init="in", next_pts="out", status="out", matches0="out", trace="out",
                       workspace="scratch"),
    "flow_reproj_mean": dict(pose="in", pts3d="in", pts2d="in", status="in", out="out"),
}
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
U8, I32, I64, F32, F64 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64
CROP_BOXES = {"left": (-60, 50, 200, 300), "larger": (-100, -50, 800, 600), "outside": (700, 500, 900, 640)}     # of tests/test_det_hip.py


def tensor(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def outputs(mem, spec):
    return {nm: mem.place(torch.empty(s, dtype=t), "out", nm) for nm, s, t in spec}


@functools.lru_cache(maxsize=None)
def sixteen_views():
    """V = 16 with every size of det_cases.N_MATCHES in one launch: the batch of tests/test_det_hip.py"""
    V = 16
    ns = [dc.N_MATCHES[(3 * V + 4 * i) % len(dc.N_MATCHES)] for i in range(V)]
    ns[:11] = dc.N_MATCHES
    views = [dc.planted_view(n, 100 * V + i) for i, n in enumerate(ns)]
    return views, dc.embed(views, V)


def test_affine_from_matches_and_bbox_vote(run=run_placement):
    """det_affine_partial_from_matches on the 16 views, then det_bbox_vote on the affines and infos it wrote (``const`` there)."""
    views, emb = sixteen_views()
    V, cap0, n1 = len(views), emb["cap0"], len(emb["kpts1"])
    nbytes = BINDING.load().det_workspace_bytes(V, cap0, do.ITERATIONS)
    assert nbytes > 0
    hw0 = np.array([dc.HW0] * V, np.int32)

    def body(mem):
        ins = [mem.place(tensor(emb[k]), "in", k) for k in ("kpts0", "n0", "matches0", "kpts1")]
        fit = outputs(mem, (("affine", (V, 2, 3), F64), ("inlier_mask", (V, cap0), I32), ("info", (V, 4), I32)))
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "det_affine_partial_from_matches", *ins, V, cap0, n1, do.REPROJ_THRESHOLD, do.ITERATIONS, 0, *fit.values(), ws, nbytes)
        hw = mem.place(tensor(hw0), "in", "hw0")
        vote = outputs(mem, (("boxes", (V, 4), I32), ("bbox", (4,), I32), ("best_view", (1,), I32)))
        mem.call(BINDING, "det_bbox_vote", fit["affine"], fit["info"], hw, V, 480, 640, _native_det.RANK_BY["matches"], *vote.values())
        return {**fit, **vote}

    got = run(body, DEV, ROLES)
    assert got["info"].tolist() == [[int(v["ok"]), len(v["src"]), v["best"], v["count"]] for v in views]
    assert got["best_view"].item() == dc.N_MATCHES.index(4096)


@pytest.mark.parametrize("V", [1, 16])
def test_affine_partial_ransac(V, run=run_placement):
    """The points form, one call per view of the batches of V = 1 and V = 16 of tests/test_det_hip.py (16: every size of
    det_cases.N_MATCHES), on the source and destination points det_affine_partial_from_matches selects on the device.  The views of
    0 matches are left out: the body places no empty piece.  Workspace: det_workspace_bytes(1, n, iterations), as the header says."""
    ns = [dc.N_MATCHES[(3 * V + 4 * i) % len(dc.N_MATCHES)] for i in range(V)]
    if V == 16:
        ns[:11] = dc.N_MATCHES
    views = [v for v in (dc.planted_view(n, 100 * V + i) for i, n in enumerate(ns)) if len(v["src"])]
    assert views
    lib = BINDING.load()

    def body(mem):
        out = {}
        for i, v in enumerate(views):
            n = len(v["src"])
            nbytes = lib.det_workspace_bytes(1, n, do.ITERATIONS)
            assert nbytes > 0
            src, dst = mem.place(tensor(v["src"], F32), "in", f"src[{i}]"), mem.place(tensor(v["dst"], F32), "in", f"dst[{i}]")
            fit = outputs(mem, ((f"affine[{i}]", (2, 3), F64), (f"inlier_mask[{i}]", (n,), I32), (f"info[{i}]", (4,), I32)))
            ws = mem.place(nbytes, "scratch", f"workspace[{i}]")
            mem.call(BINDING, "det_affine_partial_ransac", src, dst, n, do.REPROJ_THRESHOLD, do.ITERATIONS, 0, *fit.values(), ws, nbytes)
            out.update(fit)
        return out

    got = run(body, DEV, ROLES)
    for i, v in enumerate(views):
        n = len(v["src"])
        ok, count, best, inliers = got[f"info[{i}]"].tolist()          # the header: {ok, n, index of the best hypothesis, its inlier count}
        assert ok == 1 and count == n and 0 <= best < do.ITERATIONS and int(got[f"inlier_mask[{i}]"].sum()) == inliers >= 2


@pytest.mark.parametrize("name", sorted(CROP_BOXES))
def test_crop_resize(name, run=run_placement):
    img = np.random.RandomState(11).randint(0, 256, size=(480, 640)).astype(np.uint8)
    K9 = (ctypes.c_double * 9)(1063.2, 0.0, 318.7, 0.0, 1071.9, 243.1, 0.0, 0.0, 1.0)
    box, crop = CROP_BOXES[name], 256

    def body(mem):
        image, bbox = mem.place(tensor(img), "in", "image_u8"), mem.place(torch.tensor(box, dtype=I32), "in", "bbox")
        out = outputs(mem, (("out", (crop, crop), F32), ("K_crop", (9,), F64), ("info", (4,), I32)))
        mem.call(BINDING, "det_crop_resize", image, 480, 640, bbox, K9, crop, *out.values())
        return out

    got = run(body, DEV, ROLES)
    assert got["info"].tolist() == [1, box[2] - box[0], box[3] - box[1], 0] and (name != "outside" or not got["out"].any())


@pytest.mark.parametrize("H,W,levels", [(29, 37, 4), (2, 2, 3)])
def test_build_pyramid(H, W, levels, run=run_placement):
    img = np.random.RandomState(H + W).randint(0, 256, (H, W)).astype(np.uint8)
    nbytes = BINDING.load().flow_pyramid_bytes(H, W, levels - 1)
    assert nbytes == sum(h * w for h, w in fo.level_sizes(H, W, levels))

    def body(mem):
        image, pyr = mem.place(tensor(img), "in", "image_u8"), mem.place(nbytes, "out", "pyramid")
        mem.call(BINDING, "flow_build_pyramid", image, H, W, levels, pyr)
        return dict(pyramid=pyr)

    got = run(body, DEV, ROLES)
    assert torch.equal(got["pyramid"][:H * W].cpu(), tensor(img).reshape(-1))


def track_body(first, second, pts, win, levels, max_iter=10, eps=0.03):
    """both pyramids built in place (flow_build_pyramid), then flow_track on them (``const`` there), with a trace, no initial guess"""
    H, W = first.shape
    n = len(pts)
    lib = BINDING.load()
    pyr_bytes, ws_bytes = lib.flow_pyramid_bytes(H, W, levels - 1), lib.flow_workspace_bytes(n, *win)
    assert pyr_bytes > 0 and ws_bytes > 0

    def body(mem):
        pyrs = []
        for img, nm in ((first, "pyramid_i"), (second, "pyramid_j")):
            image, pyr = mem.place(tensor(img), "in", "image of " + nm), mem.place(pyr_bytes, "out", nm)
            mem.call(BINDING, "flow_build_pyramid", image, H, W, levels, pyr)
            pyrs.append(pyr)
        p = mem.place(tensor(pts, F32), "in", "pts")
        out = outputs(mem, (("next_pts", (n, 2), F32), ("status", (n,), I32), ("matches0", (n,), I64), ("trace", (n, levels, 2), I32)))
        ws = mem.place(ws_bytes, "scratch", "workspace")
        mem.call(BINDING, "flow_track", *pyrs, H, W, levels, p, None, n, win[0], win[1], max_iter, eps, fo.MIN_EIG_THRESHOLD, *out.values(), ws, ws_bytes)
        return out
    return body


@pytest.mark.parametrize("n", [5, 257])
def test_track_noisy_case(n, run=run_placement):
    """flow_cases.noisy_case() cut to 5 points and extended to 257 as tests/test_flow_hip.py extends it (15 x 15: patches in registers)."""
    case = fc.noisy_case()
    pts = np.concatenate([case.pts, case.pts[:55] + np.float32(0.375)])[:n]
    got = run(track_body(case.first, case.second, pts, case.win, case.levels, case.max_iter, case.eps), DEV, ROLES)
    assert got["status"].any() and got["matches0"].tolist() == [i if s else -1 for i, s in enumerate(got["status"].tolist())]


def test_track_31x31_window(run=run_placement):
    """The 31 x 31 case of tests/test_flow_hip.py: above FLOW_REGISTER_SAMPLES the patches live in the workspace."""
    a, b = fc.image_pair(150, 170, (3, 2), sigma=0.06, seed=5, noise_sd=4.0)
    pts = np.concatenate([fc.interior_points(150, 170, 30, 5, 6), np.array([[0, 0], [169, 149], [-40, 3]], np.float32)])
    levels = fo.pyramid_levels(150, 170, (31, 31), 2)
    assert levels == 3 and 31 * 31 > _native_det.FLOW_REGISTER_SAMPLES
    got = run(track_body(a, b, pts, (31, 31), levels), DEV, ROLES)
    assert got["status"][:-1].any() and not got["status"][-1]


@pytest.mark.parametrize("n", [5, 257])
def test_reproj_mean(n, run=run_placement):
    """the inputs of tests/test_flow_hip.py at the point counts of the tracking cases above (257: one over FLOW_REPROJ_THREADS)"""
    rs = np.random.RandomState(n)
    X = rs.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
    pose = np.concatenate([np.eye(3) + rs.normal(0, 0.01, (3, 3)), [[0.01], [-0.02], [0.6]]], axis=1)
    K = np.array([[500.0, 0, 64], [0, 510.0, 60], [0, 0, 1]])
    h = (X.astype(np.float64) @ pose[:, :3].T + pose[:, 3]) @ K.T
    x = (h[:, :2] / h[:, 2:] + rs.normal(0, 1.5, (n, 2))).astype(np.float32)
    status = (rs.uniform(size=n) < 0.8).astype(np.int32)
    K9 = (ctypes.c_double * 9)(*K.reshape(9).tolist())

    def body(mem):
        ins = [mem.place(tensor(a), "in", nm) for a, nm in ((pose, "pose"), (X, "pts3d"), (x, "pts2d"), (status, "status"))]
        out = mem.place(torch.empty(2, dtype=F64), "out", "out")
        mem.call(BINDING, "flow_reproj_mean", ins[0], K9, *ins[1:], n, out)
        return dict(out=out)

    got = run(body, DEV, ROLES)
    assert got["out"][1] == status.sum() and got["out"][0] > 0


# every case again with each library call captured in a graph and replayed (arena.run_captured): the stream contract
test_affine_from_matches_and_bbox_vote_captured = captured_twin(test_affine_from_matches_and_bbox_vote)
test_crop_resize_captured = captured_twin(test_crop_resize)
test_build_pyramid_captured = captured_twin(test_build_pyramid)
test_track_noisy_case_captured = captured_twin(test_track_noisy_case)
test_track_31x31_window_captured = captured_twin(test_track_31x31_window)
test_reproj_mean_captured = captured_twin(test_reproj_mean)
test_affine_partial_ransac_captured = captured_twin(test_affine_partial_ransac)
