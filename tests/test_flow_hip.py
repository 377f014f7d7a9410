"""The flow step's HIP kernels (include/detector/flow.h) through the C ABI against the numpy oracle (tests/flow_oracle.py).
Everything that touches pixels is integer arithmetic and the per-point algebra is individually rounded fp64 that the oracle
restates in the kernel's order, so pyramids, sums, patches, status, matches0, trace are compared for equality and next_pts bit for
bit; only the reprojection mean has a bound.  Every case satisfies the exactness conditions asserted in
tests/test_flow_oracle.py.  Outputs are poisoned before every call."""
import ctypes

import numpy as np
import pytest
import torch

import flow_cases as fc
import flow_oracle as fo
from onepose_amd import _native_det
from onepose_amd._binding import stream_handle
from onepose_amd._native_det import FLOW_REGISTER_SAMPLES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    return _native_det.load()


def _stream():
    return stream_handle(torch.device(DEV))


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def build_pyramid(lib, img, levels):
    H, W = img.shape
    nbytes = lib.flow_pyramid_bytes(H, W, levels - 1)
    assert nbytes == sum(h * w for h, w in fo.level_sizes(H, W, levels))
    pyr = torch.full((nbytes,), 0xA5, device=DEV, dtype=torch.uint8)
    image = gpu(img)
    _native_det.check(lib.flow_build_pyramid(image.data_ptr(), H, W, levels, pyr.data_ptr(), _stream()), "flow_build_pyramid")
    return pyr


@pytest.mark.parametrize("H,W,levels", [(48, 64, 3), (29, 37, 4), (2, 2, 3), (512, 512, 5), (33, 20, 6)])
def test_pyramid_bytes_equal_the_oracle(lib, H, W, levels):
    img = np.random.RandomState(H + W).randint(0, 256, (H, W)).astype(np.uint8)
    pyr = build_pyramid(lib, img, levels)
    torch.cuda.synchronize()
    assert np.array_equal(pyr.cpu().numpy(), fo.Pyramid(img, levels).packed())


# fractional offsets {0, 0.5, 1 - 2^-20} on both axes around an interior pixel, and windows over each border and a corner
FRACTIONS = [0.0, 0.5, 1.0 - 2.0 ** -20]


def stage_positions(H, W, win):
    hx, hy = (win[0] - 1) / 2, (win[1] - 1) / 2
    pos = [(W // 2 + a, H // 2 + b) for a in FRACTIONS for b in FRACTIONS]
    pos += [(hx - win[0] + 0.25, H / 2), (W - 1 + hx - 0.75, H / 2 + 0.5), (W / 2, hy - win[1] + 0.5), (W / 2 + 0.25, H - 1 + hy - 0.125),
            (hx - 3.0, hy - 2.5), (W - 1 + hx, H - 1 + hy), (1.5, 2.25)]
    pos += [(hx - win[0] - 1.0, H / 2), (W + hx + 0.5, 3.0)]                      # both fail the range test: zeros
    return np.array(pos, np.float64)


@pytest.mark.parametrize("win", [(3, 3), (15, 15), (31, 31), (15, 7)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_patch_and_mismatch_sums_equal_the_oracle(lib, win):
    H, W, level = 75, 90, 1
    a, b = fc.image_pair(H, W, (2, -1), sigma=0.1, seed=win[0] + win[1], noise_sd=6.0)
    pi, pj = fo.Pyramid(a, 2), fo.Pyramid(b, 2)
    gi, gj = build_pyramid(lib, a, 2), build_pyramid(lib, b, 2)
    Hl, Wl = pi.levels[level].shape
    prev = stage_positions(Hl, Wl, win)
    nxt = prev + np.random.RandomState(3).uniform(-1.5, 1.5, prev.shape)
    n, ns = len(prev), win[0] * win[1]
    sums = torch.full((n, 3), -77, device=DEV, dtype=torch.int64)
    patches = torch.full((n, 3, ns), -31000, device=DEV, dtype=torch.int16)
    bsums = torch.full((n, 2), -77, device=DEV, dtype=torch.int64)
    gp, gn = gpu(prev), gpu(nxt)
    _native_det.check(lib.flow_patch_sums(gi.data_ptr(), H, W, level, gp.data_ptr(), n, win[0], win[1], sums.data_ptr(), patches.data_ptr(),
                                          _stream()), "flow_patch_sums")
    _native_det.check(lib.flow_mismatch_sums(gi.data_ptr(), gj.data_ptr(), H, W, level, gp.data_ptr(), gn.data_ptr(), n, win[0], win[1],
                                             bsums.data_ptr(), _stream()), "flow_mismatch_sums")
    torch.cuda.synchronize()
    sums, patches, bsums = sums.cpu().numpy(), patches.cpu().numpy(), bsums.cpu().numpy()
    refused = 0
    for i in range(n):
        ref = fo.patch_sums(pi, level, prev[i], win)
        if ref is None:
            refused += 1
            assert not sums[i].any() and not patches[i].any() and not bsums[i].any(), i
            continue
        A, ival, ix, iy = ref
        assert sums[i].tolist() == list(A), (i, prev[i])
        assert np.array_equal(patches[i], np.stack([ival, ix, iy]).reshape(3, ns)), (i, prev[i])
        B = fo.mismatch_sums(pi, pj, level, prev[i], nxt[i], win, ref)
        assert bsums[i].tolist() == (list(B) if B is not None else [0, 0]), (i, prev[i], nxt[i])
    assert refused == 2


def run_track(lib, case, pyr_i, pyr_j, pts, init=None, ws=None, want_trace=True):
    H, W = case.first.shape
    n = len(pts)
    nbytes = lib.flow_workspace_bytes(n, *case.win)
    assert nbytes > 0
    if ws is None:
        ws = torch.full((nbytes,), 0x5A, device=DEV, dtype=torch.uint8)
    nxt = torch.full((max(n, 1), 2), float("nan"), device=DEV, dtype=torch.float32)
    status = torch.full((max(n, 1),), 7, device=DEV, dtype=torch.int32)
    m0 = torch.full((max(n, 1),), -9, device=DEV, dtype=torch.int64)
    trace = torch.full((max(n, 1), case.levels, 2), -9, device=DEV, dtype=torch.int32)
    gp = gpu(np.asarray(pts, np.float32).reshape(-1, 2)) if n else None
    gi = gpu(np.asarray(init, np.float32)) if init is not None else None
    _native_det.check(lib.flow_track(pyr_i.data_ptr(), pyr_j.data_ptr(), H, W, case.levels, gp.data_ptr() if n else None,
                                     gi.data_ptr() if gi is not None else None, n, case.win[0], case.win[1], case.max_iter, case.eps,
                                     fo.MIN_EIG_THRESHOLD, nxt.data_ptr(), status.data_ptr(), m0.data_ptr(),
                                     trace.data_ptr() if want_trace else None, ws.data_ptr(), nbytes, _stream()), "flow_track")
    torch.cuda.synchronize()
    return nxt.cpu().numpy(), status.cpu().numpy(), m0.cpu().numpy(), trace.cpu().numpy(), ws


def assert_equal_to_oracle(got, ref, n, what):
    nxt, status, m0, trace = got[:4]
    r_nxt, r_status, r_m0, r_trace = ref[:4]
    assert np.array_equal(status[:n], r_status), what
    assert np.array_equal(m0[:n], r_m0), what
    assert np.array_equal(trace[:n], r_trace), what
    bad = np.nonzero((nxt[:n].view(np.uint32) != r_nxt.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:5], nxt[bad[:5]], r_nxt[bad[:5]])


@pytest.mark.parametrize("case", fc.all_cases(), ids=lambda c: c.name)
def test_track_equals_the_oracle_bit_for_bit(lib, case):
    pyr_i, pyr_j = build_pyramid(lib, case.first, case.levels), build_pyramid(lib, case.second, case.levels)
    got = run_track(lib, case, pyr_i, pyr_j, case.pts, case.init)
    assert_equal_to_oracle(got, case.result, len(case.pts), case.name)
    again = run_track(lib, case, pyr_i, pyr_j, case.pts, case.init, want_trace=False)       # no trace asked for: none written
    assert again[0].tobytes() == got[0].tobytes() and np.array_equal(again[1], got[1]) and (again[3] == -9).all()


@pytest.mark.parametrize("n", [0, 1, 4, 5, 257])
def test_track_point_counts(lib, n):
    case = fc.noisy_case()
    pyr_i, pyr_j = build_pyramid(lib, case.first, case.levels), build_pyramid(lib, case.second, case.levels)
    pts = np.concatenate([case.pts, case.pts[:55] + np.float32(0.375)])[:n]
    got = run_track(lib, case, pyr_i, pyr_j, pts)
    if n == 0:
        assert np.isnan(got[0]).all() and got[1][0] == 7 and got[2][0] == -9                # nothing enqueued, nothing written
        return
    r202 = case.result
    if n <= 202:
        ref = [r[:n] for r in r202[:4]]
    else:
        extra = fo.track(*case.pyramids, pts[202:], None, case.win, case.max_iter, case.eps)
        ref = [np.concatenate([a, b]) for a, b in zip(r202[:4], extra[:4])]
        ref[2] = np.where(ref[1] == 1, np.arange(n), -1).astype(np.int64)
    assert_equal_to_oracle(got, ref, n, f"n={n}")


def test_large_window_keeps_its_patches_in_the_workspace_and_a_dirty_rerun_is_bitwise_equal(lib):
    """31 x 31 is the strided form (patches in the workspace); the second and third runs start from the workspace the run
    before left behind, and from a poisoned one."""
    a, b = fc.image_pair(150, 170, (3, 2), sigma=0.06, seed=5, noise_sd=4.0)
    pts = np.concatenate([fc.interior_points(150, 170, 30, 5, 6), np.array([[0, 0], [169, 149], [-40, 3]], np.float32)])
    case = fc.Case("win31", a, b, pts, win=(31, 31), max_level=2)
    assert 15 * 15 <= FLOW_REGISTER_SAMPLES < 31 * 31
    assert case.levels == 3 and all(m > 1e-9 for k, m in case.result[4].items() if k != "oscillation") and case.result[4]["oscillation"] > 1e-12
    pyr_i, pyr_j = build_pyramid(lib, a, case.levels), build_pyramid(lib, b, case.levels)
    first = run_track(lib, case, pyr_i, pyr_j, pts)
    assert_equal_to_oracle(first, case.result, len(pts), "win31")
    assert first[1][:-1].any() and not first[1][-1]
    second = run_track(lib, case, pyr_i, pyr_j, pts, ws=first[4])
    third = run_track(lib, case, pyr_i, pyr_j, pts, ws=torch.full_like(first[4], 0xFF))
    for other in (second, third):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first[:4], other[:4]))
    small = fc.planted_cases()[0]                                                            # and the register form
    pi, pj = build_pyramid(lib, small.first, small.levels), build_pyramid(lib, small.second, small.levels)
    one = run_track(lib, small, pi, pj, small.pts)
    two = run_track(lib, small, pi, pj, small.pts, ws=torch.full_like(one[4], 0xFF))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one[:4], two[:4]))


def test_rectangular_and_small_windows_equal_the_oracle(lib):
    a, b = fc.image_pair(61, 75, (1, -1), sigma=0.1, seed=9)
    for win in [(15, 7), (3, 3), (21, 5)]:
        case = fc.Case(f"win{win}", a, b, fc.interior_points(61, 75, 24, 2, 11), win=win, max_level=1)
        pyr_i, pyr_j = build_pyramid(lib, a, case.levels), build_pyramid(lib, b, case.levels)
        assert_equal_to_oracle(run_track(lib, case, pyr_i, pyr_j, case.pts), case.result, 24, case.name)


def reproj_bound(pose, K, X, x, status):
    """4 x the oracle's own fp64 error against a longdouble evaluation, plus 4 ulps of the result."""
    ref, _ = fo.reproj_mean(pose, K, X, x, status)
    ld, _ = fo.reproj_mean(pose, K, X, x, status, np.longdouble)
    own = abs(float(ref - ld))
    return ref, 4 * own + 4 * np.finfo(np.float64).eps * abs(float(ld)), own


@pytest.mark.parametrize("n", [1, 255, 300, 1000])
def test_reproj_mean_against_the_oracle(lib, n):
    rs = np.random.RandomState(n)
    X = rs.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
    pose = np.concatenate([np.eye(3) + rs.normal(0, 0.01, (3, 3)), [[0.01], [-0.02], [0.6]]], axis=1)
    K = np.array([[500.0, 0, 64], [0, 510.0, 60], [0, 0, 1]])
    h = (X.astype(np.float64) @ pose[:, :3].T + pose[:, 3]) @ K.T
    x = (h[:, :2] / h[:, 2:] + rs.normal(0, 1.5, (n, 2))).astype(np.float32)
    status = (rs.uniform(size=n) < 0.8).astype(np.int32) if n > 1 else np.ones(1, np.int32)
    ref, bound, own = reproj_bound(pose, K, X, x, status)
    g_pose, g_X, g_x, g_status, g_none = gpu(pose), gpu(X), gpu(x), gpu(status), gpu(np.zeros(n, np.int32))
    K9 = (ctypes.c_double * 9)(*K.reshape(9).tolist())
    outs = []
    for _ in range(2):
        out = torch.full((2,), float("nan"), device=DEV, dtype=torch.float64)
        _native_det.check(lib.flow_reproj_mean(g_pose.data_ptr(), K9, g_X.data_ptr(), g_x.data_ptr(), g_status.data_ptr(), n, out.data_ptr(),
                                               _stream()), "flow_reproj_mean")
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    err = abs(float(outs[0][0] - ref))
    print(f"n={n}: reproj mean |HIP - oracle| {err:.3e}, oracle's own error {own:.3e}, bound {bound:.3e}")
    assert outs[0][1] == status.sum() and err <= bound
    assert outs[0].tobytes() == outs[1].tobytes()
    none = torch.full((2,), 5.0, device=DEV, dtype=torch.float64)
    _native_det.check(lib.flow_reproj_mean(g_pose.data_ptr(), K9, g_X.data_ptr(), g_x.data_ptr(), g_none.data_ptr(), n, none.data_ptr(),
                                           _stream()), "flow_reproj_mean")
    torch.cuda.synchronize()
    assert np.isnan(float(none[0])) and float(none[1]) == 0.0
