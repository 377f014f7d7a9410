"""onepose_amd.bundle_adjust: ``apply_ba`` (the drop-in for the reference's BATracker.apply_ba) against ``BundleAdjuster.solve``
on the compacted window problem, and the module's refusals."""
import numpy as np
import pytest
import torch

import ba_cases as bc

pytestmark = pytest.mark.gpu
WIN = 4


@pytest.fixture(scope="module")
def sequence():
    """A tracker state in the reference's form: 9 keyframes (BAL cameras [9,9]), 70 points, observations of every frame, some
    without a 3D point (-1); with win_size = 4 only the frames 5 .. 8 enter."""
    rng, cams6, intr, points = bc._scene(9, 70, 61)
    kpt2ds, ids, fids = [], [], []
    for f in range(9):
        seen = np.sort(rng.choice(60, size=25, replace=False))          # points 60 .. 69 are never observed
        xy = bc._project(cams6, intr, points, np.full(25, f), seen) + rng.normal(scale=0.5, size=(25, 2))
        kpt2ds.append(xy)
        ids.append(np.where(rng.uniform(size=25) < 0.2, -1, seen))
        fids.append(np.full(25, f))
    order = rng.permutation(9 * 25)
    cams = np.concatenate([cams6 + rng.normal(scale=0.003, size=cams6.shape), intr[:, [0, 2, 3]]], axis=1)
    return (np.concatenate(kpt2ds)[order], np.concatenate(ids)[order].astype(np.int64), np.concatenate(fids)[order].astype(np.int64),
            points + rng.normal(scale=0.002, size=points.shape), cams)


def test_apply_ba_is_the_solve_on_the_compacted_window(sequence):
    from onepose_amd import BundleAdjuster
    from onepose_amd.bundle_adjust import apply_ba, compact_problem
    kpt2ds, ids, fids, kpt3ds, cams = sequence
    points_opt, cam_opt = apply_ba(kpt2ds, ids, fids, kpt3ds, cams, WIN)
    assert points_opt.shape == kpt3ds.shape and points_opt.dtype == np.float64
    assert cam_opt.shape == cams.shape == (9, 9) and cam_opt.dtype == np.float64
    cam_ids, pt_ids, cams6, intr, points, obs_cam, obs_pt, obs_xy = compact_problem(kpt2ds, ids, fids, kpt3ds, cams, WIN)
    assert list(cam_ids) == [5, 6, 7, 8] and obs_cam.dtype == np.int32 and len(obs_cam) == int(((ids != -1) & (fids > 8 - WIN)).sum())
    assert np.array_equal(intr[:, 0], intr[:, 1]) and np.array_equal(intr[:, 0], cams[cam_ids, 6])
    to = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    cams_new, points_new, trace, summary = BundleAdjuster().solve(to(cams6), to(intr), to(points), to(obs_cam), to(obs_pt), to(obs_xy))
    assert cams_new.is_cuda and points_new.is_cuda and trace.is_cuda and summary.is_cuda and trace.shape == (5, 6)
    assert np.array_equal(cam_opt[cam_ids, :6], cams_new.cpu().numpy()) and np.array_equal(points_opt[pt_ids], points_new.cpu().numpy())
    assert summary[1].item() < summary[0].item() and summary[2].item() >= 1
    # outside the window: unchanged, bit for bit; the intrinsics columns are put back
    outside = np.setdiff1d(np.arange(9), cam_ids)
    assert np.array_equal(cam_opt[outside], cams[outside]) and np.array_equal(cam_opt[:, 6:], cams[:, 6:])
    untouched = np.setdiff1d(np.arange(len(kpt3ds)), pt_ids)
    assert len(untouched) >= 10 and np.array_equal(points_opt[untouched], kpt3ds[untouched])
    assert not np.array_equal(cam_opt[cam_ids, :6], cams[cam_ids, :6])


def test_short_sequences_use_every_frame(sequence):
    from onepose_amd.bundle_adjust import window_observations
    kpt2ds, ids, fids, kpt3ds, cams = sequence
    assert len(window_observations(ids, fids, 8)) == int((ids != -1).sum())          # max fid 8 is not > 8: no window yet
    assert len(window_observations(ids, fids, 7)) == int(((ids != -1) & (fids > 1)).sum())


def test_refusals():
    import onepose_amd
    from onepose_amd import BundleAdjuster, _binding, _native_map
    assert "BundleAdjuster" in onepose_amd.__all__ and onepose_amd.__all__[-1] == "BundleAdjuster" and issubclass(BundleAdjuster, _binding.Engine)
    ba = BundleAdjuster()
    pb = bc.tiny_case()
    cpu = [torch.from_numpy(a) for a in pb.args()]
    with pytest.raises(RuntimeError, match="only on a ROCm GPU"):
        ba.solve(*cpu)
    dev = [t.cuda() for t in cpu]
    with pytest.raises(ValueError):
        ba.solve(dev[0][:, :5], *dev[1:])
    many = torch.zeros(_native_map.BA_MAX_CAMERAS + 1, 6, dtype=torch.float64, device="cuda")
    with pytest.raises(_binding.NativeError, match="ba_workspace_bytes"):
        ba.solve(many, torch.ones(len(many), 4, dtype=torch.float64, device="cuda"), *dev[2:])
    saved, _native_map._lib = (_native_map.LIB_PATH, _native_map._lib), None
    try:
        _native_map.LIB_PATH = saved[0] + ".missing"
        with pytest.raises(_binding.NativeError, match="has not been built"):
            BundleAdjuster()
    finally:
        _native_map.LIB_PATH, _native_map._lib = saved
