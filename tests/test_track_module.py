"""onepose_amd.MapUpdater, apply_triangulation and BATracker on the GPU.

BATracker is compared with the state machine of tests/track_oracle.py driven by the SAME public HIP cores as callables
(NearestNeighbour, FlowTracker.flow_track_device, MapUpdater.update, bundle_adjust.apply_ba): every core is deterministic, so
the whole state after each of 12 frames is equal -- integer arrays exactly, float arrays bit for bit.  Two sequences: motion
prediction (auto_mode=True) and the flow step on real pixels.  The pose errors are printed (pytest -s) for DESIGN section 19."""
import numpy as np
import pytest
import torch

import onepose_amd
import track_cases as tc
import track_oracle as orc
from onepose_amd import BATracker, BundleAdjuster, FlowTracker, MapUpdater, NearestNeighbour, apply_triangulation, bundle_adjust

pytestmark = pytest.mark.gpu


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def cores():
    return dict(matcher=NearestNeighbour(), flow=FlowTracker(), adjuster=BundleAdjuster(), updater=MapUpdater())


def test_exports():
    assert {"BATracker", "MapUpdater", "apply_triangulation"} <= set(onepose_amd.__all__) and onepose_amd.__all__[-1] == "BundleAdjuster"


def test_map_updater_equals_the_oracle(cores):
    c = tc.shape_cases()["63x65"]
    out = cores["updater"].update(*(gpu(c[k]) for k in tc.INPUTS))
    u = orc.update(**c)
    kept = int(u.summary[4])
    for name in ("pair_kf", "pair_q", "q_pt_ids", "unmatched_q", "summary"):
        assert np.array_equal(getattr(out, name).cpu().numpy(), getattr(u, name)), name
    assert out.pair_dist.cpu().numpy().tobytes() == u.pair_dist.tobytes() and out.median.cpu().numpy().tobytes() == u.median.tobytes()
    assert out.new_points[:kept].cpu().numpy().tobytes() == u.new_points.tobytes() and all(t.is_cuda for t in out)
    # [3, 4] poses and int64 matches are taken as they are
    again = cores["updater"].update(gpu(c["matches0"].astype(np.int64)), *(gpu(c[k]) for k in tc.INPUTS[1:7]), gpu(c["pose_kf"][:3]),
                                    gpu(c["pose_q"][:3]))
    for name, x, y in zip(out._fields, out, again):
        rows = kept if name == "new_points" else None
        assert x[:rows].cpu().numpy().tobytes() == y[:rows].cpu().numpy().tobytes(), name


def test_host_tensors_are_refused(cores):
    c = tc.shape_cases()["5x7"]
    args = [gpu(c[k]) for k in tc.INPUTS]
    for k in range(len(args)):
        bad = list(args)
        bad[k] = bad[k].cpu()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cores["updater"].update(*bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cores["updater"].gate_median(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cores["updater"].triangulate(torch.zeros(3, 4, dtype=torch.float64), gpu(np.zeros((3, 4))), gpu(np.zeros((2, 2), np.float32)),
                                     gpu(np.zeros((2, 2), np.float32)))
    with pytest.raises(TypeError):
        cores["updater"].update(c["matches0"], *args[1:])


def test_apply_triangulation_equals_the_oracle(cores):
    rs = np.random.RandomState(11)
    X = rs.uniform(-tc.BOX, tc.BOX, (70, 3))
    a = (tc.project(X, tc.K, tc.POSE_KF) + 0.3 * rs.standard_normal((70, 2))).astype(np.float32)
    b = (tc.project(X, tc.K, tc.POSE_Q) + 0.3 * rs.standard_normal((70, 2))).astype(np.float32)
    Tcw1, Tcw2 = np.linalg.inv(tc.POSE_KF), np.linalg.inv(tc.POSE_Q)
    got = apply_triangulation(tc.K, tc.K, Tcw1, Tcw2, a, b, updater=cores["updater"])
    ref = orc.triangulate_pairs(orc.projection_matrix(tc.K, np.linalg.inv(Tcw1)[:3]), orc.projection_matrix(tc.K, np.linalg.inv(Tcw2)[:3]), a, b)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.tobytes() == ref.tobytes()
    assert np.abs(got - X).max() < 5e-3
    assert apply_triangulation(tc.K, tc.K, Tcw1, Tcw2, a[:0], b[:0], updater=cores["updater"]).shape == (0, 3)


# ---- BATracker against the oracle's state machine on the same cores ------------------------------------------------------------

def oracle_tracker(cores, **kw):
    def match(desc_kf, desc_q):
        out = cores["matcher"]({"descriptors0": gpu(desc_kf.astype(np.float32))[None], "descriptors1": gpu(desc_q.astype(np.float32))[None]})
        return out["matches0"][0].cpu().numpy()

    def flow_pnp(kf_info, frame):
        flow = cores["flow"]
        pyr_kf, pyr_q = flow.pyramid(gpu(kf_info['im_path'])), flow.pyramid(gpu(frame['im_path']))
        pose, _, _, next_pts, status, kpt_dist = flow.flow_track_device(pyr_kf, pyr_q, gpu(np.asarray(kf_info['mkpts2d'], np.float32)),
                                                                      gpu(np.asarray(kf_info['mkpts3d'], np.float32)), frame['K_crop'])
        homo = np.eye(4)
        homo[:3] = pose.cpu().numpy()
        dist = kpt_dist.cpu().numpy()
        return homo, (dist[0] if dist[1] > 0 else 1000086.0), next_pts.cpu().numpy(), np.where(status.cpu().numpy() == 1)[0]

    def update(matches0, kf_xy, q_xy, kf_pt_ids, points, K_kf, K_q, pose_kf, pose_q):
        out = cores["updater"].update(gpu(np.asarray(matches0)), gpu(np.asarray(kf_xy, np.float32)), gpu(np.asarray(q_xy, np.float32)),
                                      gpu(np.asarray(kf_pt_ids, np.int32)), gpu(np.asarray(points, np.float64)), gpu(np.asarray(K_kf, np.float64)),
                                      gpu(np.asarray(K_q, np.float64)), gpu(pose_kf), gpu(pose_q))
        return orc.Update(*(t.cpu().numpy() for t in out))

    def ba(kpt2ds, ids, fids, pts, cams, win_size):
        return bundle_adjust.apply_ba(kpt2ds, ids, fids, pts, cams, win_size, adjuster=cores["adjuster"])

    return orc.Tracker(match, flow_pnp, update, ba, **kw)


def assert_same_state(a, b, where):
    sa, sb = orc.state_of(a), orc.state_of(b)
    assert sa.keys() == sb.keys()
    for key in sa:
        x, y = sa[key], sb[key]
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype.kind == y.dtype.kind and x.tobytes() == y.tobytes(), (where, key)
        else:
            assert x == y, (where, key)


def pose_error(pose, truth):
    return float(np.linalg.norm(np.asarray(pose, np.float64)[:3] - truth[:3]))


@pytest.mark.parametrize("which", ["auto", "flow"])
def test_batracker_equals_the_oracle_state_machine(cores, which):
    seq = tc.auto_sequence() if which == "auto" else tc.flow_sequence()
    ours, ref = BATracker(**cores), oracle_tracker(cores)
    s_ours, s_ref = seq.copy(), seq.copy()
    for t, s in ((ours, s_ours), (ref, s_ref)):
        assert t.update_kf(s.kf)
        t.add_kf(s.kf)
    assert_same_state(ours, ref, "keyframe")
    tracked = 0
    for k, (f_ours, f_ref) in enumerate(zip(s_ours.frames, s_ref.frames)):
        init_a, opt_a, log_a = ours.track(f_ours, auto_mode=seq.auto_mode)
        init_b, opt_b, log_b = ref.track(f_ref, auto_mode=seq.auto_mode)
        assert np.asarray(init_a).tobytes() == np.asarray(init_b).tobytes() and opt_a.tobytes() == opt_b.tobytes() and log_a == log_b
        assert_same_state(ours, ref, f"frame {k}")
        assert ("mkpts2d" in f_ours) == ("mkpts2d" in f_ref) and (ours.last_kf_info is f_ours) == (ref.last_kf_info is f_ref)
        e_init, e_opt = pose_error(init_a, seq.truth[k + 1]), pose_error(opt_a, seq.truth[k + 1])
        print(f"{which} frame {k}: |pose_init - truth| {e_init:.3e}, |pose_opt - truth| {e_opt:.3e}, {log_a}")
        if e_init > 1e-6:
            tracked += 1
            assert e_opt < e_init, (k, e_init, e_opt)
    assert tracked >= 8 and len(ours.pose_list) == 13 and ours.frame_id == 12 and ours.init_cnt == 0
    if which == "flow":
        assert ours.use_motion_cnt == 0 and ours.last_kf_info is s_ours.frames[-1]       # every frame took the flow step's pose


def test_reset_restores_the_second_defaults(cores):
    t = BATracker(**cores)
    assert (t.win_size, t.frame_interval, t.init_cnt) == (10, 5, 3)
    s = tc.auto_sequence().copy()
    t.add_kf(s.kf)
    t.track(s.frames[0], auto_mode=True)
    t.reset()
    assert (t.win_size, t.frame_interval, t.init_cnt, t.id, t.last_kf_id, t.frame_id, t.use_motion_cnt) == (20, 3, 3, 0, -1, 0, 0)
    assert t.pose_list == [] and t.kf_frames == {} and len(t.kpt2ds) == 0 and t.last_kf_info is None and t._kf_dev is None
    s = tc.auto_sequence().copy()
    t.add_kf(s.kf)                                   # usable again
    assert t.track(s.frames[0], auto_mode=True)[1].shape == (4, 4)
