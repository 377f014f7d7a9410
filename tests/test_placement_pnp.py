"""Placement tests of the pose solver (include/pnp.h, include/pnp_batch.h): pnp_ransac_epnp_matches at the wave-edge counts of
tests/pnp_cases.py, pnp_ransac_epnp_matches_batch on three frames of unequal counts and the points forms pnp_ransac_epnp /
pnp_ransac_epnp_batch at the smallest count and one past a workgroup, every device argument an exact piece of a
guarded arena (tests/arena.py) under the fills 0xFF and 0x00; the workspace is exactly pnp_workspace_bytes /
pnp_batch_workspace_bytes.  Every case runs a second time with each call captured and replayed (arena.run_captured).  Bitwise
comparisons only; the oracle comparisons stay in tests/test_pnp*.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pnp_cases as pc
from arena import captured_twin, run_placement
from onepose_amd import _native_pnp, synthetic

BINDING = _native_pnp
_OUT = dict(pose="out", inlier_mask="out", info="out", workspace="scratch")
ROLES = {
    "pnp_ransac_epnp": dict(pts_3d="in", pts_2d="in", **_OUT),
    "pnp_ransac_epnp_batch": dict(pts_3d="in", pts_2d="in", **_OUT),
    "pnp_ransac_epnp_matches": dict(kpts2d="in", kpts3d="in", matches0="in", **_OUT),
    "pnp_ransac_epnp_matches_batch": dict(kpts2d="in", kpts3d="in", matches0="in", **_OUT),
}
# the 64-lane pass of the scoring kernel (pnp_cases.SCORE_N: below, at, above one and two waves) and the 1024-thread pass of the
# selection (pnp_cases.BEST_N: one over)
COUNTS = [5, 63, 64, 65, 127, 128, 129, 1025]
assert set(COUNTS[:-1]) <= set(pc.SCORE_N) and COUNTS[-1] in pc.BEST_N
ITERATIONS = 257                                 # one over four workgroups of 64 hypotheses (pnp_cases.HYP_ITERATIONS, SCORE_ITERATIONS)
N3 = 1200
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@functools.lru_cache(maxsize=None)
def frame(n1, seed):
    """n1 query keypoints, all matched but one (all where n1 <= 5) to database points that project through a planted pose
    (0.5 px noise, 30 % of the matches wrong): the recipe of tests/test_pnp_batch.py::match_frames."""
    rs = np.random.RandomState(seed)
    db = rs.uniform(-0.1, 0.1, (N3, 3)).astype(np.float32)
    p = synthetic.make_pnp_problem(5, 0.0, 0.0, 300 + seed)                        # its K and pose
    d = rs.choice(N3, n1, replace=False)
    pcam = db[d].astype(np.float64) @ p["pose_gt"][:, :3].T + p["pose_gt"][:, 3]
    uv = np.stack([p["K"][0, 2] + p["K"][0, 0] * pcam[:, 0] / pcam[:, 2], p["K"][1, 2] + p["K"][1, 1] * pcam[:, 1] / pcam[:, 2]], axis=1)
    uv += rs.standard_normal(uv.shape) * 0.5
    wrong = rs.rand(n1) < (0.3 if n1 > 5 else 0.0)
    uv[wrong] = rs.uniform(0, 512, (int(wrong.sum()), 2))
    matches = d.astype(np.int64)
    if n1 > 5:
        matches[n1 // 2] = -1
    return dict(n1=n1, K=np.ascontiguousarray(p["K"], dtype=np.float64), kp2=uv.astype(np.float32), db=db, matches=matches, seed=7 + seed)


def host(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


@pytest.mark.parametrize("n1", COUNTS)
def test_ransac_epnp_matches(n1, run=run_placement):
    f = frame(n1, n1)
    K = f["K"].reshape(9)
    nbytes = BINDING.load().pnp_workspace_bytes(n1, ITERATIONS)
    assert nbytes > 0

    def body(mem):
        kp2, db, m0 = (mem.place(torch.from_numpy(f[k]), "in", nm) for k, nm in (("kp2", "kpts2d"), ("db", "kpts3d"), ("matches", "matches0")))
        pose, mask, info = (mem.place(torch.empty(s, dtype=t), "out", nm) for s, t, nm in
                            (((3, 4), torch.float64, "pose"), ((n1,), torch.int32, "inlier_mask"), ((4,), torch.int32, "info")))
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "pnp_ransac_epnp_matches", kp2, db, m0, n1, host(K, ctypes.c_double), pc.SCALE, pc.THR, ITERATIONS, f["seed"], pose, mask,
                 info, ws, ws.numel())
        return dict(pose=pose, inlier_mask=mask, info=info)

    got = run(body, DEV, ROLES)
    info = got["info"].tolist()
    assert info[0] in (0, 1) and int(got["inlier_mask"].sum()) == info[1] and (n1 < 63 or info[0] == 1)


@pytest.mark.parametrize("shared3d", [1, 0])
def test_ransac_epnp_matches_batch(shared3d, run=run_placement):
    """Three frames of 65, 5 and 129 keypoints at a capacity of 129: the padding of the inputs holds plausible keypoints and
    in-range match indices, as in tests/test_pnp_batch.py."""
    frames = [frame(n1, 40 + (0 if shared3d else i)) for i, n1 in enumerate((65, 5, 129))]
    b, cap1 = len(frames), 129
    rs = np.random.RandomState(3)
    kp2 = rs.uniform(0, 512, (b, cap1, 2)).astype(np.float32)
    m0 = rs.randint(-1, N3, (b, cap1)).astype(np.int64)
    for j, f in enumerate(frames):
        kp2[j, :f["n1"]], m0[j, :f["n1"]] = f["kp2"], f["matches"]
    db = frames[0]["db"] if shared3d else np.stack([f["db"] for f in frames])
    K = np.ascontiguousarray(np.stack([f["K"].reshape(9) for f in frames]))
    counts, seeds = np.array([f["n1"] for f in frames], np.int32), np.array([f["seed"] for f in frames], np.uint64)
    nbytes = BINDING.load().pnp_batch_workspace_bytes(b, cap1, ITERATIONS)
    assert nbytes > 0

    def body(mem):
        k2, k3, m = mem.place(torch.from_numpy(kp2), "in", "kpts2d"), mem.place(torch.from_numpy(db), "in", "kpts3d"), mem.place(torch.from_numpy(m0), "in", "matches0")
        pose, mask, info = (mem.place(torch.empty(s, dtype=t), "out", nm) for s, t, nm in
                            (((b, 3, 4), torch.float64, "pose"), ((b, cap1), torch.int32, "inlier_mask"), ((b, 4), torch.int32, "info")))
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "pnp_ransac_epnp_matches_batch", k2, k3, m, host(K, ctypes.c_double), host(counts, ctypes.c_int32), host(seeds, ctypes.c_uint64),
                 b, cap1, N3, shared3d, pc.SCALE, pc.THR, ITERATIONS, pose, mask, info, ws, ws.numel())
        return dict(pose=pose, inlier_mask=mask, info=info)

    got = run(body, DEV, ROLES)
    assert got["info"][0, 0] == 1 and got["info"][2, 0] == 1        # (the frame of 5 has one minimal set: it may find a model or not)
    for j, f in enumerate(frames):
        assert not got["inlier_mask"][j, f["n1"]:].any()            # "inlier_mask entries past the count are written as 0"


@functools.lru_cache(maxsize=None)
def points(n):
    """n correspondences, 30 % of them wrong, 0.5 px noise: the recipe of tests/test_pnp_batch.py::frame"""
    p = synthetic.make_pnp_problem(max(n, 5), 0.3, 0.5, 500 + n)
    return dict(n=n, K=np.ascontiguousarray(p["K"], dtype=np.float64), pts_2d=p["pts_2d"][:n], pts_3d=p["pts_3d"][:n], seed=11 + n)


@pytest.mark.parametrize("n", [5, 1025])
def test_ransac_epnp(n, run=run_placement):
    """The points form the flow step hands its tracked points to.  5: the smallest count the entry point takes (4 is refused before
    anything is enqueued; the batch below has a frame of 4); 1025: one over the selection's 1024-thread pass (pnp_cases.BEST_N)."""
    assert n == 5 or n in pc.BEST_N
    f = points(n)
    nbytes = BINDING.load().pnp_workspace_bytes(n, ITERATIONS)
    assert nbytes > 0

    def body(mem):
        p3, p2 = mem.place(torch.from_numpy(f["pts_3d"]), "in", "pts_3d"), mem.place(torch.from_numpy(f["pts_2d"]), "in", "pts_2d")
        pose, mask, info = (mem.place(torch.empty(s, dtype=t), "out", nm) for s, t, nm in
                            (((3, 4), torch.float64, "pose"), ((n,), torch.int32, "inlier_mask"), ((4,), torch.int32, "info")))
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "pnp_ransac_epnp", p3, p2, host(f["K"].reshape(9), ctypes.c_double), pc.SCALE, n, pc.THR, ITERATIONS, f["seed"], pose, mask,
                 info, ws, ws.numel())
        return dict(pose=pose, inlier_mask=mask, info=info)

    got = run(body, DEV, ROLES)
    info = got["info"].tolist()
    assert info[0] in (0, 1) and int(got["inlier_mask"].sum()) == info[1] and (n < 63 or info[0] == 1)


def test_ransac_epnp_batch(run=run_placement):
    """Frames of 4 (short: identity, no model), 1025 and 65 correspondences at a capacity of 1025; the padding holds plausible
    correspondences, as in tests/test_pnp_batch.py."""
    frames = [points(n) for n in (4, 1025, 65)]
    b, cap = len(frames), 1025
    rs = np.random.RandomState(4)
    p2, p3 = rs.uniform(0, 512, (b, cap, 2)).astype(np.float32), rs.uniform(-0.1, 0.1, (b, cap, 3)).astype(np.float32)
    for j, f in enumerate(frames):
        p2[j, :f["n"]], p3[j, :f["n"]] = f["pts_2d"], f["pts_3d"]
    K = np.ascontiguousarray(np.stack([f["K"].reshape(9) for f in frames]))
    counts, seeds = np.array([f["n"] for f in frames], np.int32), np.array([f["seed"] for f in frames], np.uint64)
    nbytes = BINDING.load().pnp_batch_workspace_bytes(b, cap, ITERATIONS)
    assert nbytes > 0

    def body(mem):
        x3, x2 = mem.place(torch.from_numpy(p3), "in", "pts_3d"), mem.place(torch.from_numpy(p2), "in", "pts_2d")
        pose, mask, info = (mem.place(torch.empty(s, dtype=t), "out", nm) for s, t, nm in
                            (((b, 3, 4), torch.float64, "pose"), ((b, cap), torch.int32, "inlier_mask"), ((b, 4), torch.int32, "info")))
        ws = mem.place(nbytes, "scratch", "workspace")
        mem.call(BINDING, "pnp_ransac_epnp_batch", x3, x2, host(K, ctypes.c_double), host(counts, ctypes.c_int32), host(seeds, ctypes.c_uint64), b, cap,
                 pc.SCALE, pc.THR, ITERATIONS, pose, mask, info, ws, ws.numel())
        return dict(pose=pose, inlier_mask=mask, info=info)

    got = run(body, DEV, ROLES)
    assert got["info"][0].tolist() == [0, 0, -1, 0] and got["info"][1, 0] == 1 and got["info"][2, 0] == 1
    assert torch.equal(got["pose"][0].cpu(), torch.eye(3, 4, dtype=torch.float64))
    for j, f in enumerate(frames):
        assert not got["inlier_mask"][j, f["n"]:].any()             # "inlier_mask entries past the count are written as 0"


# every case again with each library call captured in a graph and replayed (arena.run_captured): the stream contract
test_ransac_epnp_matches_captured = captured_twin(test_ransac_epnp_matches)
test_ransac_epnp_matches_batch_captured = captured_twin(test_ransac_epnp_matches_batch)
test_ransac_epnp_captured = captured_twin(test_ransac_epnp)
test_ransac_epnp_batch_captured = captured_twin(test_ransac_epnp_batch)
