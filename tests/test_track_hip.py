"""The HIP map update step against tests/track_oracle.py, bit for bit: trk_update as a whole at every shape of
track_cases.SHAPES (1 item, below / at / above one wave, several items a thread, the 8192 limit), with the known pairs
running over none, 1, 2, odd, even and all, on every hand case, from a dirty and from a poisoned workspace; the two stage
entries alone.  Outputs are poisoned before every call."""
import numpy as np
import pytest
import torch

import track_cases as tc
import track_oracle as orc

pytestmark = pytest.mark.gpu
POISON_I, POISON_F = -777, -12345.678


@pytest.fixture(scope="module")
def lib():
    from onepose_amd import _native_trk
    return _native_trk.load()


@pytest.fixture(scope="module")
def updater():
    from onepose_amd import MapUpdater
    return MapUpdater()


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def raw_update(lib, c, workspace=None, gate=tc.GATE, max_reproj=tc.MAX_REPROJ, max_z=tc.MAX_Z):
    """trk_update through the raw library on poisoned outputs -> (outputs as numpy, inputs as they are afterwards, workspace)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    n_kf, n_q, n_points = len(c["matches0"]), len(c["q_xy"]), len(c["points"])
    ins = [gpu(c[k]) for k in tc.INPUTS]
    i32 = lambda *s: torch.full(s, POISON_I, device=dev, dtype=torch.int32)  # noqa: E731
    f64 = lambda *s: torch.full(s, POISON_F, device=dev, dtype=torch.float64)  # noqa: E731
    outs = [i32(n_kf), i32(n_kf), i32(n_kf), f64(n_kf, 2), f64(n_kf, 3), i32(n_q), f64(1), i32(8)]
    if workspace is None:
        workspace = torch.empty(lib.trk_workspace_bytes(n_kf, n_q), device=dev, dtype=torch.uint8)
    args = [t if t.numel() else None for t in ins]
    lib.call("trk_update", dev, *args, n_kf, n_q, n_points, gate, max_reproj, max_z, *outs, workspace, workspace.numel())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs], [t.cpu().numpy() for t in ins], workspace


def assert_equals_oracle(out, c, poisoned=True, **kw):
    u = orc.update(**c, **kw)
    pair_kf, pair_q, q_pt_ids, pair_dist, new_points, unmatched_q, median, summary = out
    assert summary.tolist() == u.summary.tolist()
    m, kept, n_unmatched = int(u.summary[0]), int(u.summary[4]), int(u.summary[7])
    assert np.array_equal(pair_kf, u.pair_kf) and np.array_equal(pair_q, u.pair_q) and np.array_equal(q_pt_ids, u.q_pt_ids)
    assert np.array_equal(bits(pair_dist), bits(u.pair_dist)) and np.array_equal(bits(median), bits(u.median))
    assert np.array_equal(bits(new_points[:kept]), bits(u.new_points))
    assert np.array_equal(unmatched_q, u.unmatched_q)
    # rows beyond the counts
    assert (pair_kf[m:] == -1).all() and (pair_q[m:] == -1).all() and (q_pt_ids[m:] == -1).all()
    assert (bits(pair_dist[m:]) == 0x7ff8000000000000).all()
    assert not poisoned or (new_points[kept:] == POISON_F).all()       # not written
    assert (unmatched_q[n_unmatched:] == -1).all() and (np.diff(unmatched_q[:n_unmatched]) > 0).all()
    return u


@pytest.mark.parametrize("name", sorted(tc.shape_cases()))
def test_update_equals_the_oracle(lib, name):
    c = tc.shape_cases()[name]
    out, ins, _ = raw_update(lib, c)
    u = assert_equals_oracle(out, c)
    for k, after in zip(tc.INPUTS, ins):
        assert after.tobytes() == np.ascontiguousarray(c[k]).tobytes(), k       # inputs unchanged
    m, known, known_kept, cand, cand_kept = u.summary[:5].tolist()
    if name.endswith("known_none") or name.endswith("none_known"):
        assert known == 0 and cand == m and np.isnan(out[6][0])
    if name.endswith("known_all") or name.endswith("all_known"):
        assert cand == 0 and known == m
    for count in (1, 2, 51, 52):
        if name.endswith(f"known_{count}"):
            assert known == count
    if known >= 20:                       # the gate cuts: about 0.6 of the distances lie below 1.2 x their median
        assert 0 < known_kept < known
    if cand >= 90:                        # a tenth of the pairs are gross outliers
        assert 0 < cand_kept < cand


@pytest.mark.parametrize("name", sorted(tc.hand_cases()))
def test_update_hand_cases(lib, name):
    c = tc.hand_cases()[name]
    out, _, _ = raw_update(lib, c)
    assert_equals_oracle(out, c)


def test_other_thresholds(lib):
    c = tc.shape_cases()["257x300"]
    kw = dict(gate_factor=0.9, max_reproj=1.0, max_z=0.02)
    out, _, _ = raw_update(lib, c, gate=0.9, max_reproj=1.0, max_z=0.02)
    u = assert_equals_oracle(out, c, **kw)
    ref = orc.update(**c)
    assert u.summary[2] < ref.summary[2] and u.summary[4] < ref.summary[4]


@pytest.mark.parametrize("name", ["5x7", "257x300", "1025x1000", "8192x8192"])
def test_dirty_and_poisoned_workspace(lib, name):
    c = tc.shape_cases()[name]
    first, _, ws = raw_update(lib, c)
    other = tc.shape_cases()["8192x8192_none_known" if name != "8192x8192" else "8192x8192_all_known"]
    big = torch.empty(lib.trk_workspace_bytes(8192, 8192), device="cuda", dtype=torch.uint8)
    raw_update(lib, other, workspace=big)                      # leaves another problem's state behind
    dirty, _, _ = raw_update(lib, c, workspace=big)
    ws.fill_(0xA5)
    poisoned, _, _ = raw_update(lib, c, workspace=ws)
    for a, b, p in zip(first, dirty, poisoned):
        assert a.tobytes() == b.tobytes() == p.tobytes()


def test_updater_equals_the_oracle_and_leaves_inputs(updater):
    c = tc.shape_cases()["255x257"]
    ins = [gpu(c[k]) for k in tc.INPUTS]
    keep = [t.clone() for t in ins]
    out = updater.update(*ins)
    assert_equals_oracle([t.cpu().numpy() for t in out], c, poisoned=False)
    assert all(torch.equal(a, b) for a, b in zip(ins, keep))


@pytest.mark.parametrize("n", [1, 64, 65, 4097])
def test_triangulate_pairs_is_bitwise(updater, n):
    rs = np.random.RandomState(n)
    X = rs.uniform(-tc.BOX, tc.BOX, (n, 3))
    a = (tc.project(X, tc.K, tc.POSE_KF) + 0.4 * rs.standard_normal((n, 2))).astype(np.float32)
    b = (tc.project(X, tc.K, tc.POSE_Q) + 0.4 * rs.standard_normal((n, 2))).astype(np.float32)
    if n > 1:
        b[n // 2] = a[n // 2] = [256, 256]
    P1, P2 = orc.projection_matrix(tc.K, tc.POSE_KF), orc.projection_matrix(tc.K, tc.POSE_Q)
    got = updater.triangulate(gpu(P1), gpu(P2), gpu(a), gpu(b)).cpu().numpy()
    ref = orc.triangulate_pairs(P1, P2, a, b)
    assert np.array_equal(bits(got), bits(ref))
    assert np.abs(got - X)[np.arange(n) != (n // 2 if n > 1 else -1)].max() < 5e-3


def gate_inputs(n, kind):
    rs = np.random.RandomState(1000 + n)
    d = rs.uniform(0, 40, n) ** 2 / 40
    if kind == "equal":
        d[:] = 3.25
    if kind == "nan":
        d[n // 2] = np.nan
    if kind == "ties":
        d = np.round(d)                  # many equal values around the median
    if kind == "signed":
        d = d - 15.0                     # the stage entry orders negative values too
    return d


@pytest.mark.parametrize("kind", ["random", "equal", "nan", "ties", "signed"])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1024, 1025, 8192])
def test_gate_median_is_numpys(updater, n, kind):
    d = gate_inputs(n, kind)
    median, keep = updater.gate_median(gpu(d), 1.2)
    median, keep = median.cpu().numpy(), keep.cpu().numpy()
    with np.errstate(all="ignore"):
        want = np.median(d) * 1.2
    assert np.array_equal(bits(median), bits(orc.canonical(np.array([want]))))
    assert np.array_equal(keep, (d < want).astype(np.int32))
    ref_med, ref_keep = orc.gate_median(d, 1.2)
    assert np.array_equal(bits(np.array([ref_med])), bits(median)) and np.array_equal(ref_keep, keep)
