"""The detector tail's HIP library (include/detector/detector.h) stage by stage through its C ABI against the numpy fp64 oracle
(tests/detector_oracle.py).  The oracle restates every expression in the kernels' order and numpy never fuses a multiply
with an add, so best hypothesis, inlier mask, boxes and crop bits are compared exactly; the refit is held to the bound
below.  Every planted case satisfies the exactness conditions of detector_oracle.exactness_conditions (asserted here)."""
import ctypes

import numpy as np
import pytest
import torch

import det_cases as dc
import detector_oracle as do
from onepose_amd import _native_det
from onepose_amd._binding import stream_handle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    return _native_det.load()


def _stream():
    return stream_handle(torch.device(DEV))


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_from_matches(lib, emb, iterations=do.ITERATIONS, seed=0, views=None):
    sel = slice(None) if views is None else views
    kpts0, n0, m0 = gpu(emb["kpts0"][sel]), gpu(emb["n0"][sel]), gpu(emb["matches0"][sel])
    kpts1 = gpu(emb["kpts1"])
    V, cap0 = kpts0.shape[0], kpts0.shape[1]
    nbytes = lib.det_workspace_bytes(V, cap0, iterations)
    assert nbytes > 0
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    aff = torch.full((V, 2, 3), float("nan"), device=DEV, dtype=torch.float64)
    mask = torch.full((V, cap0), 7, device=DEV, dtype=torch.int32)
    info = torch.full((V, 4), -9, device=DEV, dtype=torch.int32)
    _native_det.check(lib.det_affine_partial_from_matches(kpts0.data_ptr(), n0.data_ptr(), m0.data_ptr(), kpts1.data_ptr(), V, cap0,
                                                          kpts1.shape[0], do.REPROJ_THRESHOLD, iterations, seed, aff.data_ptr(),
                                                          mask.data_ptr(), info.data_ptr(), ws.data_ptr(), nbytes, _stream()),
                      "det_affine_partial_from_matches")
    torch.cuda.synchronize()
    return aff, mask, info


def refit_bound(view):
    """4 x the oracle's own fp64 error against a longdouble evaluation of the same inliers, plus 4 ulps of the output scale
    (the rule of the SuperGlue stage tests)."""
    ld = do.refit(view["src"], view["dst"], view["mask"], np.longdouble)
    own = float(np.abs(view["affine"] - ld).max())
    return 4 * own + 4 * np.finfo(np.float64).eps * float(np.abs(ld).max()), own


def check_views(views, emb, aff, mask, info):
    worst = 0.0
    for i, v in enumerate(views):
        assert all(v["conditions"]), (i, v["conditions"])
        n = len(v["src"])
        assert info[i].tolist() == [int(v["ok"]), n, v["best"], v["count"]], (i, n, info[i].tolist())
        full = np.zeros(emb["cap0"], np.int32)
        full[emb["positions"][i][v["mask"]]] = 1
        assert np.array_equal(mask[i], full), (i, n)
        if v["ok"]:
            bound, own = refit_bound(v)
            err = float(np.abs(aff[i] - v["affine"]).max())
            worst = max(worst, err / bound)
            print(f"n={n}: refit |HIP - oracle| {err:.3e}, oracle's own error {own:.3e}, bound {bound:.3e}")
            assert err <= bound, (i, n, err, bound)
        else:
            assert (aff[i] == 0).all()
    return worst


@pytest.mark.parametrize("V", [1, 2, 15, 16])
def test_ransac_batched_matches_the_oracle_and_each_view_alone(lib, V):
    ns = [dc.N_MATCHES[(3 * V + 4 * i) % len(dc.N_MATCHES)] for i in range(V)]
    if V == 16:
        ns[:11] = dc.N_MATCHES                 # every size of the list in one launch
    views = [dc.planted_view(n, 100 * V + i) for i, n in enumerate(ns)]
    emb = dc.embed(views, V)
    aff, mask, info = (t.cpu().numpy() for t in run_from_matches(lib, emb))
    check_views(views, emb, aff, mask, info)
    aff2, mask2, info2 = (t.cpu().numpy() for t in run_from_matches(lib, emb))        # two runs: bitwise equal
    assert aff.tobytes() == aff2.tobytes() and np.array_equal(mask, mask2) and np.array_equal(info, info2)
    for i in sorted({0, V // 2, V - 1}):                                                # each view alone: bitwise equal
        a1, m1, i1 = (t.cpu().numpy() for t in run_from_matches(lib, emb, views=slice(i, i + 1)))
        assert a1[0].tobytes() == aff[i].tobytes() and np.array_equal(m1[0], mask[i]) and np.array_equal(i1[0], info[i]), i


@pytest.mark.parametrize("n", dc.N_MATCHES + [4100])
def test_ransac_single_view_sizes(lib, n):
    """Wave (64) and LDS-chunk (4096) edges, one view per launch; 4100 crosses into a second chunk."""
    views = [dc.planted_view(n, 7)]
    emb = dc.embed(views, n)
    aff, mask, info = (t.cpu().numpy() for t in run_from_matches(lib, emb))
    check_views(views, emb, aff, mask, info)


@pytest.mark.parametrize("n,iterations,seed", [(2, 50, 0), (3, 200, 1), (64, 2000, 5), (300, 777, 2)])
def test_points_entry_matches_the_oracle(lib, n, iterations, seed):
    rs = np.random.RandomState(n)
    src, dst, _, _ = do.planted_matches(rs, n, 0.3 if n > 3 else 0.0, noise=2.0)
    ok, A, m, best, cnt, dbg = do.estimate_affine_partial(src, dst, iterations=iterations, seed=seed, return_debug=True)
    assert np.all(np.abs(dbg["residuals"] - dbg["thr2"]) > 1e-6)
    s, d = gpu(src), gpu(dst)
    nbytes = lib.det_workspace_bytes(1, n, iterations)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    aff = torch.empty(2, 3, device=DEV, dtype=torch.float64)
    mask = torch.empty(n, device=DEV, dtype=torch.int32)
    info = torch.empty(4, device=DEV, dtype=torch.int32)
    _native_det.check(lib.det_affine_partial_ransac(s.data_ptr(), d.data_ptr(), n, 6.0, iterations, seed, aff.data_ptr(), mask.data_ptr(),
                                                    info.data_ptr(), ws.data_ptr(), nbytes, _stream()), "det_affine_partial_ransac")
    torch.cuda.synchronize()
    assert int(info[0]) == 1 and int(info[1]) == n
    # the winner's count is exact; its index too whenever no other pair ties (small n: the same pair is drawn many times)
    assert int(info[3]) == cnt and np.array_equal(mask.cpu().numpy().astype(bool), m)
    assert int(info[2]) == best
    bound, _ = refit_bound(dict(src=src, dst=dst, mask=m, affine=A))
    assert float(np.abs(aff.cpu().numpy() - A).max()) <= bound


def test_degenerate_and_failed_views(lib):
    """All source points coincide (no valid sample), fewer than 6 matches, no keypoints at all, matches pointing past n1."""
    rs = np.random.RandomState(0)
    cap0, n1 = 40, 30
    kpts1 = rs.uniform(0, 500, (n1, 2)).astype(np.float32)
    kpts0 = rs.uniform(0, 500, (4, cap0, 2)).astype(np.float32)
    kpts0[0, :] = 5.0
    m0 = np.full((4, cap0), -1, np.int64)
    m0[0, :20] = np.arange(20)
    m0[1, :5] = np.arange(5)
    m0[3, :10] = np.arange(10) + n1 - 4          # six of them >= n1: unmatched, leaves 4 matches
    emb = dict(kpts0=kpts0, n0=np.array([cap0, cap0, 0, cap0], np.int32), matches0=m0, kpts1=kpts1)
    aff, mask, info = (t.cpu().numpy() for t in run_from_matches(lib, emb))
    assert info.tolist() == [[0, 20, -1, 0], [0, 5, -1, 0], [0, 0, -1, 0], [0, 4, -1, 0]]
    assert (aff == 0).all() and (mask == 0).all()


def vote_gpu(lib, aff, info, hw0, qh, qw, rank_by):
    V = len(info)
    a, i, h = gpu(np.asarray(aff, np.float64)), gpu(np.asarray(info, np.int32)), gpu(np.asarray(hw0, np.int32))
    boxes = torch.empty(V, 4, device=DEV, dtype=torch.int32)
    bbox = torch.empty(4, device=DEV, dtype=torch.int32)
    bv = torch.empty(1, device=DEV, dtype=torch.int32)
    _native_det.check(lib.det_bbox_vote(a.data_ptr(), i.data_ptr(), h.data_ptr(), V, qh, qw, _native_det.RANK_BY[rank_by],
                                        boxes.data_ptr(), bbox.data_ptr(), bv.data_ptr(), _stream()), "det_bbox_vote")
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), bbox.cpu().numpy(), int(bv)


@pytest.mark.parametrize("rank_by", ["matches", "inliers"])
def test_box_and_vote_are_integer_equal_to_the_oracle(lib, rank_by):
    ns = [0, 64, 5, 1024, 64, 1024, 65, 7]
    views = [dc.planted_view(n, 40 + i) for i, n in enumerate(ns)]
    hw0 = [(480, 640), (480, 640), (300, 400), (480, 640), (512, 512), (480, 640), (200, 333), (480, 640)]
    aff = np.stack([v["affine"] for v in views])
    info = np.array([[int(v["ok"]), len(v["src"]), v["best"], v["count"]] for v in views], np.int32)
    for v, hw in zip(views, hw0):
        if v["ok"]:
            c = do.projected_corners(v["affine"], hw)
            assert np.all(np.abs(c - np.rint(c)) > 1e-6)
    boxes, bbox, bv = vote_gpu(lib, aff, info, hw0, 480, 640, rank_by)
    ref_boxes = np.stack([do.view_box(v["affine"], v["ok"], hw, (480, 640)) for v, hw in zip(views, hw0)])
    ref_bv = do.vote(info[:, 0], info[:, 1], info[:, 3], rank_by)
    assert np.array_equal(boxes, ref_boxes) and bv == ref_bv and np.array_equal(bbox, ref_boxes[ref_bv])
    assert bv == (3 if rank_by == "matches" else ref_bv)          # 1024 matches twice: the first of the two
    assert boxes[0].tolist() == [0, 0, 480, 640] and boxes[2].tolist() == [0, 0, 480, 640]
    # all views failed: the first view's [0, 0, H, W]
    boxes, bbox, bv = vote_gpu(lib, np.zeros((3, 2, 3)), np.array([[0, 5, -1, 0], [0, 0, -1, 0], [0, 3, -1, 0]]), [(9, 9)] * 3, 480, 640,
                               rank_by)
    assert bv == 0 and bbox.tolist() == [0, 0, 480, 640]
    # negative coordinates truncate toward zero, like .astype(np.int32)
    A = np.array([[[0.5, -0.25, -10.7], [0.25, 0.5, -3.2]]])
    boxes, bbox, bv = vote_gpu(lib, A, np.array([[1, 10, 0, 8]]), [(100, 37)], 480, 640, rank_by)
    assert np.array_equal(bbox, do.view_box(A[0], True, (100, 37), (480, 640))) and bbox[0] == -35


def crop_gpu(lib, img_u8, bbox, K, crop):
    H, W = img_u8.shape
    im, bb = gpu(img_u8), gpu(np.asarray(bbox, np.int32))
    out = torch.full((crop, crop), float("nan"), device=DEV, dtype=torch.float32)
    Kc = torch.empty(9, device=DEV, dtype=torch.float64)
    info = torch.empty(4, device=DEV, dtype=torch.int32)
    rc = lib.det_crop_resize(im.data_ptr(), H, W, bb.data_ptr(), (ctypes.c_double * 9)(*np.asarray(K, np.float64).reshape(9)), crop,
                             out.data_ptr(), Kc.data_ptr(), info.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), Kc.cpu().numpy().reshape(3, 3), info.cpu().numpy()


CROP_BOXES = {"inside": (100, 80, 400, 330), "left": (-60, 50, 200, 300), "top": (50, -70, 300, 200), "right": (500, 100, 700, 300),
              "bottom": (100, 400, 300, 560), "larger": (-100, -50, 800, 600), "one_px_wide": (300, 10, 301, 470),
              "one_px_high": (10, 200, 630, 201), "wide": (20, 200, 620, 300), "tall": (300, 5, 380, 475), "outside": (700, 500, 900, 640)}


@pytest.mark.parametrize("crop", [256, 512])
@pytest.mark.parametrize("name", list(CROP_BOXES))
def test_crop_is_bitwise_equal_to_the_oracle(lib, name, crop):
    rs = np.random.RandomState(11)
    img = rs.randint(0, 256, size=(480, 640)).astype(np.uint8)
    K = np.array([[1063.2, 0.0, 318.7], [0.0, 1071.9, 243.1], [0.0, 0.0, 1.0]])
    box = CROP_BOXES[name]
    rc, out, Kc, info = crop_gpu(lib, img, box, K, crop)
    assert rc == 0 and info.tolist() == [1, box[2] - box[0], box[3] - box[1], 0]
    ref = do.crop_resize(img, box, crop)
    assert out.tobytes() == ref.tobytes(), int((out != ref).sum())
    assert Kc.tobytes() == do.k_crop(box, K, crop).tobytes()
    if name == "outside":
        assert (out == 0).all()


def test_crop_refuses_bad_sizes_and_empty_boxes(lib):
    img = np.zeros((48, 64), np.uint8) + 9
    K = np.eye(3)
    for bad in (300, 96, 1000):
        rc, _, _, _ = crop_gpu(lib, img, (0, 0, 10, 10), K, bad)
        assert rc != 0 and b"power of two" in lib.det_last_error(), bad
    for box in [(10, 10, 10, 30), (10, 10, 30, 10), (30, 30, 10, 50)]:
        rc, out, Kc, info = crop_gpu(lib, img, box, K, 64)
        assert rc == 0 and info[0] == 0 and (out == 0).all() and (Kc == 0).all()
