"""onepose_amd.flow: the numpy drop-in and the device chain track -> RANSAC-EPnP -> reprojection distance against the oracle, on a
planted scene; float and uint8 images give one pyramid; host tensors are refused."""
import numpy as np
import pytest
import torch

import flow_cases as fc
import flow_oracle as fo
import onepose_amd
from onepose_amd import FlowTracker, ImagePyramid, kpt_flow_track, pnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def tracker():
    return FlowTracker()


def test_exports():
    assert {"FlowTracker", "ImagePyramid", "kpt_flow_track"} <= set(onepose_amd.__all__)


def test_kpt_flow_track_equals_the_oracle_on_a_planted_pair():
    case = fc.planted_cases()[3]
    kpt_new, valid = kpt_flow_track(case.first, case.second, case.pts)
    r_nxt, r_status = case.result[:2]
    assert kpt_new.dtype == np.float32 and kpt_new.shape == (40, 2) and isinstance(valid, tuple) and len(valid) == 1
    assert kpt_new.tobytes() == r_nxt.tobytes() and np.array_equal(valid[0], np.where(r_status == 1)[0])
    assert np.abs(kpt_new - (case.pts + np.array(case.planted, np.float32))).max() <= 0.03


def planted_scene(n=300, size=128, shift=(5, -3), seed=4):
    """n 3D points seen by a known pose in a textured size x size keyframe; the query is the same texture shifted by whole
    pixels, i.e. the same pose under an intrinsic matrix whose principal point moved by the shift."""
    rs = np.random.RandomState(seed)
    first, second = fc.image_pair(size, size, shift, sigma=0.08, seed=seed)
    K = np.array([[420.0, 0, size / 2], [0, 420.0, size / 2], [0, 0, 1]])
    ang = np.array([0.3, -0.2, 0.1])
    cx, cy, cz = np.cos(ang)
    sx, sy, sz = np.sin(ang)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t = np.array([0.02, -0.01, 0.6])
    uv = rs.uniform(12, size - 13, (n, 2))
    z = rs.uniform(0.5, 0.7, n)
    cam = np.concatenate([(uv - K[:2, 2]) / 420.0, np.ones((n, 1))], axis=1) * z[:, None]
    X = ((cam - t) @ R).astype(np.float32)                       # R^T (cam - t)
    c = X.astype(np.float64) @ R.T + t
    kpts = ((c @ K.T)[:, :2] / c[:, 2:]).astype(np.float32)
    K_query = K.copy()
    K_query[0, 2] += shift[0]
    K_query[1, 2] += shift[1]
    return first, second, kpts, X, K_query, np.concatenate([R, t[:, None]], axis=1)


def test_flow_track_device_on_a_planted_scene(tracker):
    first, second, kpts, X, K_query, pose_true = planted_scene()
    pyr_kf, pyr_query = tracker.pyramid(gpu(first)), tracker.pyramid(gpu(second))
    assert isinstance(pyr_kf, ImagePyramid) and pyr_kf.levels == 3
    pose, mask, info, next_pts, status, kpt_dist = tracker.flow_track_device(pyr_kf, pyr_query, gpu(kpts), gpu(X), K_query, seed=3)
    torch.cuda.synchronize()
    pi, pj = fo.Pyramid(first, 3), fo.Pyramid(second, 3)
    r_nxt, r_status, r_m0, _, margins = fo.track(pi, pj, kpts)
    assert margins["min_eig"] > 1e-9 and margins["det"] > 1e-9 and margins["eps"] > 1e-9 and margins["oscillation"] > 1e-12
    assert next_pts.cpu().numpy().tobytes() == r_nxt.tobytes() and np.array_equal(status.cpu().numpy(), r_status)
    assert int(info[0]) == 1 and int(r_status.sum()) >= 290
    ref_pose, ref_mask, ref_info = pnp.ransac_pnp_from_matches(K_query, gpu(r_nxt), gpu(X), gpu(r_m0), seed=3)
    assert pose.cpu().numpy().tobytes() == ref_pose.cpu().numpy().tobytes()
    assert torch.equal(mask, ref_mask) and torch.equal(info, ref_info)
    P = pose.cpu().numpy()
    assert np.abs(P - pose_true).max() < 1e-2
    ref, count = fo.reproj_mean(P, K_query, X, r_nxt, r_status)
    ld, _ = fo.reproj_mean(P, K_query, X, r_nxt, r_status, np.longdouble)
    own = abs(float(ref - ld))
    bound = 4 * own + 4 * np.finfo(np.float64).eps * abs(float(ld))
    got = kpt_dist.cpu().numpy()
    print(f"kpt_dist {got[0]:.6f} px over {int(got[1])} points; |HIP - oracle| {abs(got[0] - ref):.3e}, bound {bound:.3e}")
    assert got[1] == count and abs(got[0] - ref) <= bound and got[0] < 0.1


def test_float_and_uint8_images_give_the_same_pyramid(tracker):
    img = fc.texture(70, 90, 0.08, 12)
    as_u8 = tracker.pyramid(gpu(img))
    crop = (gpu(img).to(torch.float32) / 255.0)[None, None]                       # as the detector returns it
    as_float = tracker.pyramid(crop)
    assert (as_u8.H, as_u8.W, as_u8.levels) == (70, 90, 3) == (as_float.H, as_float.W, as_float.levels)
    expect = (crop[0, 0] * 255).to(torch.uint8)                                    # inference_demo.py:251: truncation
    assert torch.equal(as_float.level(0), expect)
    assert np.array_equal(as_float.data.cpu().numpy(), fo.Pyramid(expect.cpu().numpy(), 3).packed())
    assert np.array_equal(as_u8.data.cpu().numpy(), fo.Pyramid(img, 3).packed())
    if torch.equal(expect, gpu(img)):
        assert torch.equal(as_u8.data, as_float.data)
    assert as_u8.level(2).shape == (18, 23)


def test_track_returns_the_trace_on_request_and_takes_a_guess(tracker):
    case = fc.guess_case()
    pyr_kf, pyr_query = tracker.pyramid(gpu(case.first)), tracker.pyramid(gpu(case.second))
    nxt, status, m0, trace = tracker.track(pyr_kf, pyr_query, gpu(case.pts), init=gpu(case.init), trace=True)
    r = case.result
    assert nxt.cpu().numpy().tobytes() == r[0].tobytes() and np.array_equal(trace.cpu().numpy(), r[3]) and np.array_equal(m0.cpu().numpy(), r[2])
    assert len(tracker.track(pyr_kf, pyr_query, gpu(case.pts))) == 3
    allocated = tracker._workspaces.allocations
    tracker.track(pyr_kf, pyr_query, gpu(case.pts))
    assert tracker._workspaces.allocations == allocated                            # the workspace is cached per shape


def test_host_tensors_are_refused_with_the_modules_message(tracker):
    case = fc.planted_cases()[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tracker.pyramid(torch.from_numpy(case.first))
    pyr = tracker.pyramid(gpu(case.first))
    with pytest.raises(RuntimeError, match=r"onepose_amd.FlowTracker runs only on a ROCm GPU \(the points are on cpu\); there is no CPU fallback"):
        tracker.track(pyr, pyr, torch.from_numpy(case.pts))
    with pytest.raises(ValueError):
        tracker.track(pyr, tracker.pyramid(gpu(fc.planted_cases()[3].first)), gpu(case.pts))
    with pytest.raises(ValueError):
        FlowTracker(win_size=(16, 15))
