"""The batched pose solver (pnp_ransac_epnp_batch, pnp_ransac_epnp_matches_batch) against the single-frame entry points, by EQUALITY:
every frame's pose (as int64 bits), mask and info are those of the frame solved alone.  No tolerance anywhere -- the single-frame solve
is pinned stage by stage in tests/test_pnp_stages.py, and these tests tie the batch to it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pnp_cases as pc
from onepose_amd import _native_pnp, pnp, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the edges of the model size (5), of score_kernel's 64-lane pass and of best_kernel's 1024-thread pass (2049: three passes)
FRAME_N = [0, 4, 5, 6, 63, 64, 65, 1023, 1024, 1025, 2049]
FRAME_SEEDS = [0, 1, 5, 2 ** 24 + 3, 7, 2 ** 63 + 1, 11, 2 ** 24 + 3, 2 ** 63 + 1, 13, 5]       # two of them wrap seed << 40
CAP = 2049
ITERATIONS = [1, 64, 257, 1025]           # hyp_kernel: 64 per workgroup; score_kernel: 4 per workgroup; best_kernel: 1024 per pass
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
FAILED = [0, 0, -1, 0]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64).cpu().numpy()


@functools.lru_cache(maxsize=None)
def frame(i):
    """Frame i of the ragged batch: n = FRAME_N[i] correspondences of a problem of its own (own K, own pose), padded to CAP."""
    n = FRAME_N[i]
    p = synthetic.make_pnp_problem(max(n, 5), 0.3, 0.5, 100 + i)
    return dict(n=n, K=p["K"], seed=FRAME_SEEDS[i], pts_2d=p["pts_2d"][:n], pts_3d=p["pts_3d"][:n])


@functools.lru_cache(maxsize=None)
def alone(i, iterations):
    """Frame i solved by pnp_ransac_epnp alone -> (pose bits [12], mask [n], info [4]) as numpy; None for a frame the call refuses."""
    f = frame(i)
    if f["n"] < 5:
        return None
    pose, mask, info = pnp.ransac_pnp_device(f["K"], gpu(f["pts_2d"]), gpu(f["pts_3d"]), scale=pc.SCALE, reproj_error=pc.THR,
                                             iterations=iterations, seed=f["seed"])
    return bits(pose).reshape(12), mask.cpu().numpy(), info.cpu().numpy()


def padded(frames, cap, pad_seed=None):
    """-> pts_2d [b, cap, 2], pts_3d [b, cap, 3]; the entries past a frame's count are zero, or (pad_seed) finite values of the same
    ranges as real correspondences: wrong if read, never a fault."""
    b = len(frames)
    if pad_seed is None:
        p2, p3 = np.zeros((b, cap, 2), np.float32), np.zeros((b, cap, 3), np.float32)
    else:
        rs = np.random.RandomState(pad_seed)
        p2, p3 = rs.uniform(0, 512, (b, cap, 2)).astype(np.float32), rs.uniform(-0.1, 0.1, (b, cap, 3)).astype(np.float32)
    for j, f in enumerate(frames):
        p2[j, :f["n"]], p3[j, :f["n"]] = f["pts_2d"], f["pts_3d"]
    return p2, p3


def check_frame(what, pose, mask, info, n, want):
    """One frame of a batch (numpy: pose bits [12], mask [cap], info [4]) against the single-frame answer `want` (None: a short frame)."""
    if want is None:
        np.testing.assert_array_equal(pose, IDENTITY.reshape(12).view(np.int64), err_msg=what)
        np.testing.assert_array_equal(info, FAILED, err_msg=what)
        assert not mask.any(), what
        return
    np.testing.assert_array_equal(pose, want[0], err_msg=what)
    np.testing.assert_array_equal(mask[:n], want[1], err_msg=what)
    np.testing.assert_array_equal(info, want[2], err_msg=what)
    assert not mask[n:].any(), what


def batch_orders():
    """The eleven frames as they are; then b = 1, 2, 31, 32 with the frames repeated cyclically -- for b = 1 and 2 also starting from
    the far end, so that the long frames are seen at position 0 of a small batch as well."""
    k = len(FRAME_N)
    orders = [list(range(k))] + [[j % k for j in range(b)] for b in (1, 2, 31, 32)]
    return orders + [[k - 1], [k - 1, k - 2]]


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_every_frame_of_a_batch_is_the_frame_solved_alone(iterations):
    """Ragged counts at the edges of every pass, own K and seed per frame, through the public wrapper; each frame is compared with the
    SAME single-frame answer wherever it sits and whatever the batch size, so a frame also equals itself in every other batch."""
    for order in batch_orders():
        frames = [frame(i) for i in order]
        p2, p3 = padded(frames, CAP)
        pose, mask, info = pnp.ransac_pnp_batch(np.stack([f["K"] for f in frames]), gpu(p2), gpu(p3), counts=[f["n"] for f in frames],
                                                scale=pc.SCALE, reproj_error=pc.THR, iterations=iterations, seeds=[f["seed"] for f in frames])
        assert pose.shape == (len(order), 3, 4) and mask.shape == (len(order), CAP) and info.shape == (len(order), 4)
        pose, mask, info = bits(pose).reshape(-1, 12), mask.cpu().numpy(), info.cpu().numpy()
        for j, i in enumerate(order):
            check_frame(f"iterations = {iterations}, b = {len(order)}, position {j}, n = {FRAME_N[i]}", pose[j], mask[j], info[j], FRAME_N[i],
                        alone(i, iterations))
    if iterations >= 64:         # not vacuous: at 30 % outliers a sample of 5 is clean with p = 0.17, so 64 draws miss with p < 1e-5 --
        #                          the seven frames of 63 correspondences and more have a model (the frames of 5 and 6 need not)
        assert sum(alone(i, iterations)[2][0] == 1 for i in range(len(FRAME_N)) if FRAME_N[i] >= 63) >= 6


def garbage(nbytes, seed):
    return torch.randint(0, 256, (nbytes,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).to(DEV)


def raw_batch(frames, cap, iterations, pad_seed, garbage_seed):
    """pnp_ransac_epnp_batch on buffers of the test's own: the workspace and all three outputs start out as random bytes."""
    b = len(frames)
    p2, p3 = (gpu(a) for a in padded(frames, cap, pad_seed))
    lib = _native_pnp.load()
    ws = garbage(lib.pnp_batch_workspace_bytes(b, cap, iterations), garbage_seed)
    pose = garbage(b * 12 * 8, garbage_seed + 1).view(torch.float64).view(b, 3, 4)
    mask = garbage(b * cap * 4, garbage_seed + 2).view(torch.int32).view(b, cap)
    info = garbage(b * 4 * 4, garbage_seed + 3).view(torch.int32).view(b, 4)
    k = np.ascontiguousarray(np.stack([f["K"] for f in frames]).reshape(b, 9))
    n = np.array([f["n"] for f in frames], np.int32)
    s = np.array([f["seed"] for f in frames], np.uint64)
    _native_pnp.call("pnp_ransac_epnp_batch", DEV, p3, p2, k.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                     n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), s.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), b, cap, pc.SCALE,
                     pc.THR, iterations, pose, mask, info, ws, ws.numel())
    return bits(pose).reshape(b, 12), mask.cpu().numpy(), info.cpu().numpy()


def test_dirty_buffers_and_wrong_padding_change_nothing():
    """Workspace and outputs pre-filled with random bytes, the padding of the inputs filled with plausible wrong correspondences: the
    answers are those of the clean run (i.e. of the frames alone), the mask's padding is ZERO, and a second run over other garbage is
    bitwise the first."""
    iterations = 257
    frames = [frame(i) for i in range(len(FRAME_N))]
    first = raw_batch(frames, CAP, iterations, pad_seed=1, garbage_seed=10)
    second = raw_batch(frames, CAP, iterations, pad_seed=2, garbage_seed=20)
    for a, c in zip(first, second):
        np.testing.assert_array_equal(a, c)
    for j in range(len(frames)):
        check_frame(f"frame {j}, n = {FRAME_N[j]}", first[0][j], first[1][j], first[2][j], FRAME_N[j], alone(j, iterations))


# ---- the matches variant ----------------------------------------------------------------------------------------------
MATCH_N1 = [1, 5, 5, 1000, 1025]           # the second frame of 5 has one unmatched keypoint: 4 valid matches, no model
CAP1, N3 = 1025, 1200


@functools.lru_cache(maxsize=None)
def match_frames(shared3d):
    """Frames of n1 query keypoints, about 60 % of them matched (all of them where n1 <= 5, but for one keypoint of the second frame
    of 5) to points of a database that project through the frame's planted pose (0.5 px noise, 30 % of the matches wrong).  shared3d:
    one database for all frames; otherwise each frame has its own."""
    frames = []
    for i, n1 in enumerate(MATCH_N1):
        rs = np.random.RandomState(50 + i)
        db = np.random.RandomState(7 if shared3d else 70 + i).uniform(-0.1, 0.1, (N3, 3)).astype(np.float32)
        p = synthetic.make_pnp_problem(5, 0.0, 0.0, 200 + i)                        # its K and pose
        m = n1 if n1 <= 5 else int(0.6 * n1)
        q = np.sort(rs.choice(n1, m, replace=False))
        d = rs.choice(N3, m, replace=False)
        pcam = db[d].astype(np.float64) @ p["pose_gt"][:, :3].T + p["pose_gt"][:, 3]
        uv = np.stack([p["K"][0, 2] + p["K"][0, 0] * pcam[:, 0] / pcam[:, 2], p["K"][1, 2] + p["K"][1, 1] * pcam[:, 1] / pcam[:, 2]], axis=1)
        uv += rs.standard_normal(uv.shape) * 0.5
        wrong = rs.rand(m) < (0.3 if n1 > 5 else 0.0)
        uv[wrong] = rs.uniform(0, 512, (int(wrong.sum()), 2))
        kp2 = rs.uniform(0, 512, (n1, 2)).astype(np.float32)
        matches = -np.ones(n1, np.int64)
        kp2[q], matches[q] = uv.astype(np.float32), d
        if i == 2:
            matches[3] = -1
        frames.append(dict(n1=n1, K=p["K"], seed=FRAME_SEEDS[3 + i], kp2=kp2, db=db, matches=matches, valid=int((matches > -1).sum())))
    return frames


@pytest.mark.parametrize("shared3d", [1, 0])
def test_matches_batch_is_the_single_frame_matches_call(shared3d):
    iterations = 257
    frames = match_frames(shared3d)
    b = len(frames)
    rs = np.random.RandomState(3)
    kp2 = rs.uniform(0, 512, (b, CAP1, 2)).astype(np.float32)               # padding: plausible keypoints and IN-RANGE match indices
    m0 = rs.randint(-1, N3, (b, CAP1)).astype(np.int64)
    for j, f in enumerate(frames):
        kp2[j, :f["n1"]], m0[j, :f["n1"]] = f["kp2"], f["matches"]
    db = gpu(frames[0]["db"]) if shared3d else gpu(np.stack([f["db"] for f in frames]))
    if not shared3d:
        assert all((frames[0]["db"] != f["db"]).any() for f in frames[1:])
    pose, mask, info = pnp.ransac_pnp_from_matches_batch([f["K"] for f in frames], gpu(kp2), db, gpu(m0), counts=[f["n1"] for f in frames],
                                                         scale=pc.SCALE, reproj_error=pc.THR, iterations=iterations, seeds=[f["seed"] for f in frames])
    pose, mask, info = bits(pose).reshape(b, 12), mask.cpu().numpy(), info.cpu().numpy()
    for j, f in enumerate(frames):
        one = pnp.ransac_pnp_from_matches(f["K"], gpu(f["kp2"]), gpu(f["db"]), gpu(f["matches"]), scale=pc.SCALE, reproj_error=pc.THR,
                                          iterations=iterations, seed=f["seed"])
        check_frame(f"shared3d = {shared3d}, frame {j}, n1 = {f['n1']}", pose[j], mask[j], info[j], f["n1"],
                    (bits(one[0]).reshape(12), one[1].cpu().numpy(), one[2].cpu().numpy()))
        if f["valid"] < 5:                                                  # fails cleanly, beside frames that succeed
            check_frame(f"short frame {j}", pose[j], mask[j], info[j], f["n1"], None)
    assert [f["valid"] < 5 for f in frames] == [True, False, True, False, False]
    assert info[3][0] == 1 and info[4][0] == 1                            # ... that succeed


# ---- the default workload ---------------------------------------------------------------------------------------------
def test_eight_frames_at_the_default_iterations():
    """b = 8, the two CHAIN_CASES problems cycled (300 and 2049 correspondences in one batch of capacity 2049), 10000 hypotheses, a seed
    per frame: bitwise the single-frame solve, which test_the_solve_is_its_stages ties to the stages; like that test it asks for a
    model with at least 5 inliers, and the pose is within 0.3 degrees and 0.2 cm of the planted one -- the bound the suite already
    accepts for 0.5 px noise (tests/test_pnp.py: the oracle at 300 correspondences with MORE outliers, the solver at 400)."""
    names = list(pc.CHAIN_CASES)
    cases = [pc.chain_case(names[j % len(names)]) for j in range(8)]
    frames = [dict(n=len(c["pts_3d"]), K=c["K"], seed=pc.CHAIN_SEED + j, pts_2d=c["pts_2d"], pts_3d=c["pts_3d"]) for j, c in enumerate(cases)]
    cap = max(f["n"] for f in frames)
    p2, p3 = padded(frames, cap, pad_seed=4)
    pose, mask, info = pnp.ransac_pnp_batch(np.stack([f["K"] for f in frames]), gpu(p2), gpu(p3), counts=[f["n"] for f in frames],
                                            scale=pc.SCALE, reproj_error=pc.THR, iterations=pc.CHAIN_ITERATIONS, seeds=[f["seed"] for f in frames])
    pose_bits, mask, info = bits(pose).reshape(8, 12), mask.cpu().numpy(), info.cpu().numpy()
    pose = pose.cpu().numpy()
    for j, (f, c) in enumerate(zip(frames, cases)):
        one = pnp.ransac_pnp_device(f["K"], gpu(f["pts_2d"]), gpu(f["pts_3d"]), scale=pc.SCALE, reproj_error=pc.THR,
                                    iterations=pc.CHAIN_ITERATIONS, seed=f["seed"])
        check_frame(f"frame {j}", pose_bits[j], mask[j], info[j], f["n"], (bits(one[0]).reshape(12), one[1].cpu().numpy(), one[2].cpu().numpy()))
        r_err, t_err = pnp.query_pose_error(pose[j], c["pose_gt"])
        print(f"frame {j} ({names[j % len(names)]}): {info[j][1]} inliers, {r_err:.4f} deg, {t_err:.4f} cm")
        assert info[j][0] == 1 and info[j][1] >= 5
        assert r_err < 0.3 and t_err < 0.2


def test_thirty_three_frames_go_in_two_calls():
    """More than PNP_MAX_ITEMS frames through the wrapper: the 33rd frame, alone in the second call, is still the frame solved alone."""
    order = [4 + j % 7 for j in range(33)]                                # n = 63 .. 2049
    frames = [frame(i) for i in order]
    p2, p3 = padded(frames, CAP)
    pose, mask, info = pnp.ransac_pnp_batch(np.stack([f["K"] for f in frames]), gpu(p2), gpu(p3), counts=[f["n"] for f in frames],
                                            scale=pc.SCALE, reproj_error=pc.THR, iterations=64, seeds=[f["seed"] for f in frames])
    pose, mask, info = bits(pose).reshape(-1, 12), mask.cpu().numpy(), info.cpu().numpy()
    for j, i in enumerate(order):
        check_frame(f"position {j}", pose[j], mask[j], info[j], FRAME_N[i], alone(i, 64))


# ---- FrameMatcher -----------------------------------------------------------------------------------------------------
def test_solve_poses_device_is_solve_pose_device_per_frame():
    """Three synthetic crops of different sizes (so their keypoint counts differ) through extractor, matcher and ONE batched solve:
    per frame bitwise what solve_pose_device answers with that frame's K and seed."""
    from onepose_amd import FrameMatcher, GATsSuperGlue, SuperPoint
    ext = SuperPoint({"nms_radius": 3, "max_keypoints": 1000})
    ext.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_spp_state_dict(0).items()}, strict=True)
    hp = {"descriptor_dim": 256, "keypoints_encoder": [32, 64, 128], "match_type": "softmax", "scale_factor": 0.07,
          "match_threshold": 0.0, "include_self": True, "additional": False, "with_linear_transform": False}
    m = GATsSuperGlue(hp)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict(0).items()}, strict=True)
    dbn = synthetic.make_inputs(b=1, n1=4, n2=300, num_leaf=8, seed=3)
    db = {k: torch.from_numpy(dbn[k]).to(DEV) for k in ("keypoints3d", "descriptors3d_db", "descriptors2d_db")}
    fm = FrameMatcher(ext.to(DEV).eval(), m.to(DEV).eval(), db)
    images = [torch.from_numpy(synthetic.make_image(1, s, s, 4 + j)).to(DEV) for j, s in enumerate((96, 160, 256))]
    Ks = [np.array([[600.0 + 10 * j, 0, s / 2], [0, 590.0 + 10 * j, s / 2], [0, 0, 1]]) for j, s in enumerate((96, 160, 256))]
    seeds = [3, 2 ** 24 + 3, 9]
    poses, masks, infos, dets = fm.solve_poses_device(images, Ks, seeds=seeds)
    counts = [d["keypoints"][0].shape[0] for d in dets]
    assert len(set(counts)) == 3 and min(counts) >= 5, counts
    assert poses.shape == (3, 3, 4) and masks.shape == (3, max(counts)) and infos.shape == (3, 4)
    for j in range(3):
        pose, mask, info, det = fm.solve_pose_device(images[j], Ks[j], seed=seeds[j])
        assert torch.equal(det["keypoints"][0], dets[j]["keypoints"][0])
        check_frame(f"crop {j}, {counts[j]} keypoints", bits(poses[j]).reshape(12), masks[j].cpu().numpy(), infos[j].cpu().numpy(), counts[j],
                    (bits(pose).reshape(12), mask.cpu().numpy(), info.cpu().numpy()))
