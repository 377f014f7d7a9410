"""GPU tests of the ragged frame batch (gatsspg_forward_frames): b frames with their own query counts against ONE database and one
b = 1 cache.  Everything is compared with the project's own single-frame cached forward, which the reference-run goldens pin, so no
tolerance appears anywhere: frame i of the batch is BITWISE that frame alone (torch.equal throughout).

Shapes are the smallest that cross every granule: the column padding CP = 128, the 64-column tiles, the 128-row score tile, the
16-row conf strip, the 4-point GATs tile (n2 = 130: a last tile of 2 points, and the non-vector conf path; n2 = 256: the vector one).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gatsspg_oracle as orc
from onepose_amd import FrameMatcher, GATsSuperGlue, SuperPoint, synthetic
from onepose_amd.gats_superglue import pack_frames

pytestmark = pytest.mark.gpu

HP = dict(orc.DEFAULT_HPARAMS, match_threshold=0.0)      # threshold 0: the matches of random weights are not all -1
PRECISIONS = ["fp32", "bf16x3", "bf16x6", "fp16x3", "fp16x4"]
COUNTS = [2, 16, 17, 63, 64, 65, 127, 128, 129, 200]
CAP1 = 200
KEYS = ("conf", "matches0", "matching_scores0", "matches1", "matching_scores1")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


_models, _dbs, _queries, _alone = {}, {}, {}, {}


def model_of(precision, **hp):
    key = (precision, tuple(sorted(hp.items())))
    if key not in _models:
        m = GATsSuperGlue(dict(HP, **hp), precision=precision).eval()
        sd = synthetic.make_state_dict(0)
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
        _models[key] = m.to(dev())
    return _models[key]


def database_tensors(n2, num_leaf=8):
    if (n2, num_leaf) not in _dbs:
        d = synthetic.make_inputs(1, 4, n2, num_leaf, seed=70 + num_leaf)
        _dbs[(n2, num_leaf)] = {k: torch.from_numpy(d[k]).to(dev()) for k in ("descriptors3d_db", "descriptors2d_db")}
    return _dbs[(n2, num_leaf)]


def query(n, n2=130):
    """The one query of n points that every test uses (so that the frames' references are computed once and shared)."""
    if n not in _queries:
        _queries[n] = torch.from_numpy(synthetic.make_inputs(1, n, 8, 1, seed=1000 + n)["descriptors2d_query"][0]).to(dev()).contiguous()
    return _queries[n]


def alone(model, db, q, share=None):
    """The frame alone through the existing b = 1 cached forward; `share`: a key under which the result is kept (never modified)."""
    if share is not None and share in _alone:
        return _alone[share]
    n, n2 = q.shape[1], db.n2
    data = {"keypoints2d": torch.zeros(1, n, 2, device=dev()), "keypoints3d": torch.zeros(1, n2, 3, device=dev()),
            "descriptors2d_query": q[None]}
    conf, m0, m1, s0, s1 = model.forward_batched(data, database=db)
    out = dict(zip(KEYS, (conf[0], m0[0], s0[0], m1[0], s1[0])))
    if share is not None:
        _alone[share] = out
    return out


def setup(precision, n2, num_leaf=8, **hp):
    model = model_of(precision, **hp)
    key = ("db", precision, n2, num_leaf, tuple(sorted(hp.items())))
    if key not in _alone:
        _alone[key] = model.prepare_database(database_tensors(n2, num_leaf))
    return model, _alone[key]


def same(got, ref, what):
    for k in KEYS:
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), f"{what}: {k} differs from the frame alone"


def check_frames(model, db, counts, tag, share=True):
    qs = [query(n) for n in counts]
    res = model.match_frames(qs, db)
    assert len(res) == len(counts)
    hits = 0
    for i, (n, r) in enumerate(zip(counts, res)):
        ref = alone(model, db, qs[i], share=(tag, n) if share else None)
        same(r, ref, f"{tag} frame {i} (n1 = {n})")
        hits += int((ref["matches0"] > -1).sum())
    assert hits > 0, "the case never matched anything"
    return res


@pytest.mark.parametrize("n2", [130, 256])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_frame_is_bitwise_the_frame_alone(precision, n2):
    model, db = setup(precision, n2)
    dq, counts = pack_frames([query(n) for n in COUNTS])
    assert dq.shape == (10, 256, CAP1)
    out = model.engine.forward_frames(dq, counts, db, HP["scale_factor"], HP["match_threshold"])
    conf, m0, m1, s0, s1 = out
    for i, n in enumerate(COUNTS):
        ref = alone(model, db, query(n), share=(precision, n2, n))
        got = dict(zip(KEYS, (conf[i, :n], m0[i, :n], s0[i, :n], m1[i], s1[i])))
        same(got, ref, f"{precision} n2={n2} frame {i} (n1 = {n})")
        assert bool((m0[i, n:] == -1).all()) and bool((s0[i, n:] == 0).all()), "past the count: matches0 = -1, mscores0 = 0"
    assert int((m0 > -1).sum()) > 0


@pytest.mark.parametrize("n2", [130, 256])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_poisoned_padding_workspace_and_outputs(precision, n2):
    """NaN in the padded query columns, the whole workspace and the output buffers: the results do not move, and the conf rows past a
    count still hold the poison (they are not written)."""
    model, db = setup(precision, n2)
    eng = model.engine
    nan = float("nan")
    dq = torch.full((len(COUNTS), 256, CAP1), nan, device=dev())
    pack_frames([query(n) for n in COUNTS], out=dq)
    ws = eng.workspace(len(COUNTS), CAP1, n2, 8, dev())
    ws.view(torch.float32).fill_(nan)
    out = eng._outputs(len(COUNTS), CAP1, n2, dev())
    out[0].fill_(nan); out[3].fill_(nan); out[4].fill_(nan)
    out[1].fill_(-7); out[2].fill_(-7)
    conf, m0, m1, s0, s1 = eng.forward_frames(dq, COUNTS, db, HP["scale_factor"], HP["match_threshold"], out=out)
    assert conf.data_ptr() == out[0].data_ptr()
    for i, n in enumerate(COUNTS):
        ref = alone(model, db, query(n), share=(precision, n2, n))
        got = dict(zip(KEYS, (conf[i, :n], m0[i, :n], s0[i, :n], m1[i], s1[i])))
        same(got, ref, f"poisoned {precision} n2={n2} frame {i} (n1 = {n})")
        assert bool(torch.isnan(conf[i, n:]).all()), "conf rows past the count are not written"
        assert bool((m0[i, n:] == -1).all()) and bool((s0[i, n:] == 0).all())


FLAG_CASES = {"no_self": dict(include_self=False), "additional": dict(additional=True), "wlt": dict(with_linear_transform=True),
              "wlt_additional": dict(with_linear_transform=True, additional=True)}


@pytest.mark.parametrize("precision", ["fp32", "fp16x4"])
@pytest.mark.parametrize("case", sorted(FLAG_CASES) + ["leaf3"])
def test_gats_flags_and_generic_leaf_count(case, precision):
    hp = FLAG_CASES.get(case, {})
    model, db = setup(precision, 130, 3 if case == "leaf3" else 8, **hp)
    check_frames(model, db, [2, 65, 129], ("flags", case, precision))


@pytest.mark.parametrize("precision", ["fp32", "fp16x4"])
def test_shifted_softmax_path(precision):
    """1 / scale_factor = 100 > 80: raw scores, the two softmax statistics kernels, the max-subtracting finalisation."""
    model, db = setup(precision, 130, scale_factor=0.01)
    check_frames(model, db, [17, 129], ("shifted", precision))


@pytest.mark.parametrize("precision", ["fp32", "fp16x4"])
def test_capacity_across_the_looped_prologue_of_conf_finalize(precision):
    """cap1 = 2100 is past the 2048 rows of the straight-line prologue: the 300-point frame takes the straight-line form alone and
    the looped one inside the batch -- the same sums in the same order."""
    model, db = setup(precision, 130)
    check_frames(model, db, [2100, 300], ("cap2100", precision))


@pytest.mark.parametrize("precision,n2,counts", [("fp32", 3840, [200, 300, 128]), ("fp16x4", 5888, [100, 200, 129]), ("fp16x3", 5888, [200, 100])])
def test_frames_of_two_kernel_forms_in_one_batch(precision, n2, counts):
    """A stage whose kernel form goes by the size of the launch runs every frame on the form it takes alone.  fp32: mlp.3 takes the
    K-split 64 x 64 tile up to 64 column tiles per launch -- n2p = 3840 is 60 of them, so a frame of 200 / 128 points (64 / 62 tiles)
    takes it and one of 300 (66) the 128 x 64 tile.  fp16: mlp.0 takes the 128-column tile from 96 tiles on -- n2p = 5888 is 92, so
    200 / 129 points (96) take it and 100 (94) the 64-column one."""
    model, db = setup(precision, n2)
    check_frames(model, db, counts, ("forms", precision))


def test_fp16_mlp3_ring_switch_inside_the_batch():
    """The fp16 mlp.3 takes the two-stage ring from more than 256 column tiles per launch: five frames at n2p = 3328 are 5 x 56 = 280
    tiles in the batch (two-stage) and 54-56 alone (three-stage).  The two rings differ in when an instruction is issued, never in
    the order of additions: the frames still equal themselves alone."""
    model, db = setup("fp16x4", 3300)
    check_frames(model, db, [65, 129, 2, 17, 128], ("ring", "fp16x4"))


@pytest.mark.parametrize("cached", [True, False])
@pytest.mark.parametrize("n2", [130, 256])
def test_shared_leaf_gats_layer_is_the_layer_frame_by_frame(n2, cached):
    """One GATs layer over b = 5 frames (two groups of the shared-leaf kernel: 4 + 1) through gatsspg_gats_layer_frames, against
    gatsspg_gats_layer on every frame alone; with the leaf logits from the database cache and recomputed.  The per-frame kernel at
    database stride 0 (shared_leaf = False) must give the same bits."""
    model, db = setup("fp32", n2)
    eng, t = model.engine, database_tensors(n2)
    g = torch.Generator().manual_seed(17)
    d3 = (torch.rand(5, 256, n2, generator=g) - 0.5).to(dev())
    dq = (torch.rand(5, 256, 6, generator=g) - 0.5).to(dev())
    layer = 2
    ref = []
    for i in range(5):
        dims = eng.load_state(dq[i:i + 1].contiguous(), d3[i:i + 1].contiguous(), 8)
        eng.gats_layer(dims, layer, t["descriptors2d_db"])
        ref.append(eng.store_state(dims)[1][0].clone())
    tiles = (n2 + 3) // 4
    y2_qy_kv = 2 * 256 * n2 + 4 * (64 * 64 + 64 + 8)                       # floats in front of the leaf logits in a b = 1 cache
    ll = db.cache[y2_qy_kv + (layer - 1) * tiles * 32:][:tiles * 32].contiguous() if cached else None
    for shared in (True, False):
        dims = eng.load_state(dq, d3, 8)
        eng.gats_layer_frames(dims, layer, t["descriptors2d_db"], ll, shared_leaf=shared)
        o2, o3 = eng.store_state(dims)
        assert torch.equal(o2, dq), "a GATs layer must not touch the 2D side"
        for i in range(5):
            assert torch.equal(o3[i], ref[i]), f"n2={n2} cached={cached} shared={shared}: frame {i} differs from the layer alone"


def test_one_frame_at_capacity_is_forward_cached():
    model, db = setup("fp32", 130)
    r = model.match_frames([query(200)[None]], db)[0]
    same(r, alone(model, db, query(200), share=("fp32", 130, 200)), "b = 1")


@pytest.mark.parametrize("precision", ["fp32", "fp16x4"])
def test_uniform_counts_equal_the_uniform_batch_on_a_replicated_database(precision):
    """Three 65-point frames: the existing uniform batch over three COPIES of the database, frame by frame.  (At this size the uniform
    batch launches the kernel forms one frame launches alone -- its thresholds go by the size of the whole launch -- so it is bitwise
    the single frames too.)"""
    model, db = setup(precision, 130)
    t = database_tensors(130)
    qs = [torch.roll(query(65), k, dims=1).contiguous() for k in range(3)]
    data = {"keypoints2d": torch.zeros(3, 65, 2, device=dev()), "keypoints3d": torch.zeros(3, 130, 3, device=dev()),
            "descriptors2d_query": torch.stack(qs), "descriptors3d_db": t["descriptors3d_db"].expand(3, -1, -1).contiguous(),
            "descriptors2d_db": t["descriptors2d_db"].expand(3, -1, -1).contiguous()}
    conf, m0, m1, s0, s1 = model.forward_batched(data)
    for i, r in enumerate(model.match_frames(qs, db)):
        same(r, dict(zip(KEYS, (conf[i], m0[i], s0[i], m1[i], s1[i]))), f"uniform frame {i}")


def test_permuting_the_frames_permutes_the_outputs_and_runs_repeat():
    model, db = setup("fp16x4", 130)
    counts = [129, 2, 65, 17, 200]
    a = model.match_frames([query(n) for n in counts], db)
    again = model.match_frames([query(n) for n in counts], db)
    perm = [3, 0, 4, 2, 1]
    b = model.match_frames([query(counts[p]) for p in perm], db)
    for i, p in enumerate(perm):
        same(b[i], a[p], f"permuted frame {i}")
    for i in range(len(counts)):
        same(again[i], a[i], f"second run, frame {i}")


@pytest.mark.parametrize("precision", ["fp32", "fp16x4"])
def test_thirty_two_frames(precision):
    model, db = setup(precision, 130)
    counts = [COUNTS[i % len(COUNTS)] for i in range(32)]
    res = model.match_frames([query(n) for n in counts], db)
    for i, (n, r) in enumerate(zip(counts, res)):
        same(r, alone(model, db, query(n), share=(precision, 130, n)), f"b = 32 frame {i} (n1 = {n})")
    # 33 frames: two chunks
    res = model.match_frames([query(n) for n in counts + [63]], db)
    assert len(res) == 33
    same(res[32], alone(model, db, query(63), share=(precision, 130, 63)), "frame 32 (second chunk)")


def test_forward_frames_is_hip_graph_capturable():
    """Counts by value in the kernel arguments, nothing allocated, copied or synchronised: one linear chain, captured and replayed."""
    model, db = setup("fp32", 130)
    eng, lib = model.engine, model.engine.lib
    counts = [2, 65, 129, 200]
    dq, _ = pack_frames([query(n) for n in counts])
    ref = eng.forward_frames(dq, counts, db, HP["scale_factor"], HP["match_threshold"])
    packed = eng.packed_weights(dev())
    ws = eng.workspace(4, CAP1, 130, 8, dev())
    out = [torch.zeros_like(t) for t in ref]
    n1 = (ctypes.c_int32 * 4)(*counts)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream(dev()).cuda_stream
        rc = lib.gatsspg_forward_frames(packed.data_ptr(), dq.data_ptr(), n1, db.desc2d_db.data_ptr(), db.cache.data_ptr(), db.cache.numel() * 4,
                                        4, CAP1, 130, 8, eng.flags(), HP["scale_factor"], HP["match_threshold"], *[t.data_ptr() for t in out],
                                        ws.data_ptr(), ws.numel(), st)
        assert rc == 0
    for i in range(4):
        n1[i] = 2          # the counts were read at enqueue time: the graph holds them
    out[0].zero_()
    g.replay()
    torch.cuda.synchronize()
    for i, n in enumerate(counts):
        for a, b in zip(out, ref):
            assert torch.equal(a[i, :n] if a.shape[1] == CAP1 else a[i], b[i, :n] if b.shape[1] == CAP1 else b[i])


class ShortFrames:
    """The extractor, with the detections of every image of height `short_h` cut to ONE keypoint (a frame that stays out of the batch)."""

    def __init__(self, extractor, short_h):
        self.extractor, self.short_h = extractor, short_h

    def __call__(self, image):
        det = self.extractor(image)
        keep = {self.short_h: 1, self.short_h + 8: 0}.get(image.shape[-2])     # a second height: NO keypoint at all
        if keep is None:
            return det
        return {"keypoints": [det["keypoints"][0][:keep]], "scores": [det["scores"][0][:keep]], "descriptors": [det["descriptors"][0][:, :keep]]}


SIZES = (96, 160, 256)


@pytest.fixture(scope="module")
def frame_matcher():
    ext = SuperPoint({"nms_radius": 3, "max_keypoints": 1000})
    ext.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_spp_state_dict(0).items()}, strict=True)
    dbn = synthetic.make_inputs(b=1, n1=4, n2=300, num_leaf=8, seed=3)
    db = {k: torch.from_numpy(dbn[k]).to(dev()) for k in ("keypoints3d", "descriptors3d_db", "descriptors2d_db")}
    return FrameMatcher(ShortFrames(ext.to(dev()).eval(), 64), model_of("fp32"), db)


def crops():
    return [torch.from_numpy(synthetic.make_image(1, s, s, 4 + j)).to(dev()) for j, s in enumerate(SIZES)]


def test_frame_matcher_match_frames_is_the_per_frame_call(frame_matcher):
    ims = crops()
    res = frame_matcher.match_frames(ims)
    counts = set()
    for im, r in zip(ims, res):
        ref = frame_matcher(im)
        counts.add(ref["keypoints2d"].shape[0])
        assert sorted(r) == sorted(ref)
        for k in ref:
            assert r[k].shape == ref[k].shape and r[k].dtype == ref[k].dtype and torch.equal(r[k], ref[k]), k
    assert len(counts) == 3 and min(counts) >= 5, counts


def test_solve_poses_device_with_the_batched_matcher_is_the_frame_loop(frame_matcher):
    """Forced on against forced off: the same poses, masks and infos bit for bit.  A frame with fewer than 2 keypoints stays out of
    the batch and is answered as without it: the single-frame path refuses one keypoint (what InstanceNorm1d raises in the
    reference), with the same error either way."""
    ims = crops()
    Ks = [np.array([[600.0 + 10 * j, 0, s / 2], [0, 590.0 + 10 * j, s / 2], [0, 0, 1]]) for j, s in enumerate(SIZES)]
    seeds = [3, 2 ** 24 + 3, 9]
    off = frame_matcher.solve_poses_device(ims, Ks, seeds=seeds, batched_matcher=False)
    on = frame_matcher.solve_poses_device(ims, Ks, seeds=seeds, batched_matcher=True)
    assert int(off[2][:, 1].min()) >= 5, "every frame was meant to be solved"
    for a, b in zip(off[:3], on[:3]):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    for a, b in zip(off[3], on[3]):
        assert torch.equal(a["keypoints"][0], b["keypoints"][0])
    # Frames with fewer than 2 keypoints stay out of the batch and meet the single-frame path, as without the batch.  One keypoint: the
    # matcher refuses it (what InstanceNorm1d raises in the reference).  NO keypoint: the matcher returns the reference's bare dict
    # (:195-203), which the frame loop has never unpacked -- a different error from the one the ragged batch raises for a short query,
    # so this case tells whether such frames really stay out of the batch.
    K4 = Ks + [Ks[0]]
    short = torch.from_numpy(synthetic.make_image(1, 64, 64, 9)).to(dev())
    empty = torch.from_numpy(synthetic.make_image(1, 72, 64, 8)).to(dev())
    for extra, word in ((short, "more than 1 spatial element"), (empty, "unpack")):
        errors = []
        for flag in (False, True):
            with pytest.raises(ValueError, match=word) as e:
                frame_matcher.solve_poses_device(ims + [extra], K4, seeds=seeds + [1], batched_matcher=flag)
            errors.append(str(e.value))
        assert errors[0] == errors[1]
    with pytest.raises(ValueError, match="more than 1 spatial element"):      # the batch itself refuses a short query
        frame_matcher.matcher.match_frames([torch.zeros(256, 0, device=dev())], frame_matcher.db_cache)
