"""SuperGlue HIP kernels against the reference-run goldens and the numpy oracle (fp64 for the stages), on the MI355X."""
import json
import os

import numpy as np
import pytest
import torch

import superglue_oracle as so
from onepose_amd import SuperGlue, StreamRing, synthetic

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")
IN_KEYS = ("keypoints0", "keypoints1", "scores0", "scores1", "descriptors0", "descriptors1")


def meta():
    with open(os.path.join(GOLD, "sg_golden_meta.json")) as f:
        return json.load(f)


def build(sd, cfg):
    m = SuperGlue(cfg).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


def to_dev(inp, stream_data=True):
    d = {k: torch.from_numpy(inp[k]).to(DEV) for k in IN_KEYS}
    b = inp["keypoints0"].shape[0]
    h, w = (int(x) for x in inp["image_size0"])
    d["image0"] = torch.empty(b, 1, h, w, device=DEV)
    h, w = (int(x) for x in inp["image_size1"])
    d["image1"] = torch.empty(b, 1, h, w, device=DEV)
    return d


def case(name):
    spec = meta()["cases"][name]
    cfg = spec["cfg"]
    fn = synthetic.make_superglue_passthrough_state_dict if spec["w"]["kind"] == "passthrough" else synthetic.make_superglue_state_dict
    sd = fn(spec["w"]["seed"], len(cfg["GNN_layers"]), **{k: v for k, v in spec["w"].items() if k not in ("kind", "seed")})
    inp = synthetic.make_superglue_inputs(**spec["inp"])
    return sd, inp, cfg, dict(np.load(os.path.join(GOLD, f"sg_{name}.npz")))


def run_full(model, d):
    b, n0, n1 = d["keypoints0"].shape[0], d["keypoints0"].shape[1], d["keypoints1"].shape[1]
    z = torch.empty(b, n0 + 1, n1 + 1, device=DEV)
    out = model.engine.forward(*(d[k] for k in ("keypoints0", "scores0", "descriptors0", "keypoints1", "scores1", "descriptors1")),
                               d["image0"].shape[-2:], d["image1"].shape[-2:], z_out=z)
    names = ("matches0", "matches1", "matching_scores0", "matching_scores1")
    return {k: v.cpu().numpy() for k, v in zip(names, out)}, z.cpu().numpy()


MAXIMA = {}


@pytest.mark.parametrize("name", ["tiny", "iters0", "iters1", "n1", "planted", "outdoor", "headline", "stress", "peaked", "sizes"])
def test_forward_matches_golden(name):
    sd, inp, cfg, gold = case(name)
    model = build(sd, cfg)
    out, Z = run_full(model, to_dev(inp))
    if "Z" in gold:
        zerr = float(np.abs(Z - gold["Z"]).max())
        stats = so.z_stats(gold["Z"].astype(np.float64))
    else:
        st = so.z_stats(Z)
        zerr = max(float(np.abs(st[k] - gold[k]).max()) for k in ("row_best", "col_best", "dust_row", "dust_col"))
        stats = gold
    c0 = stats["row_best"] - stats["row_second"] > 1e-4
    c1 = stats["col_best"] - stats["col_second"] > 1e-4
    serr = max(float(np.abs(out[k] - gold[k]).max() / max(1.0, float(np.abs(gold[k]).max())))
               for k in ("matching_scores0", "matching_scores1"))
    print(f"\n{name}: max|dZ| {zerr:.3e}  max score err (rel to max(1, |s|)) {serr:.3e}  clear rows {c0.mean():.3f}")
    assert zerr < so.FORWARD_ZTOL
    assert serr < so.FORWARD_STOL
    assert (out["matches0"][c0] == gold["matches0"][c0]).all()
    assert (out["matches1"][c1] == gold["matches1"][c1]).all()
    if name in ("planted", "peaked"):
        m0 = out["matches0"][0]
        assert (m0[inp["planted0"][0]] == inp["planted1"][0]).all() and (m0 >= 0).sum() == inp["planted0"].shape[1]


def _stage_model(n_layers=2):
    sd = synthetic.make_superglue_state_dict(21, n_layers)
    return sd, build(sd, {"GNN_layers": ["self", "cross"][:n_layers] if n_layers <= 2 else ["self", "cross"] * (n_layers // 2)})


def test_stage_keypoint_encoder():
    sd, model = _stage_model()
    inp = synthetic.make_superglue_inputs(2, 37, 53, 480, 640, seed=22)
    d = to_dev(inp)
    o0, o1 = model.engine.keypoint_encode(d["keypoints0"], d["scores0"], d["descriptors0"], d["keypoints1"], d["scores1"],
                                          d["descriptors1"], (480, 640), (480, 640))
    for o, s in ((o0, 0), (o1, 1)):
        ref = so.keypoint_encode(sd, inp[f"keypoints{s}"], inp[f"scores{s}"], inp[f"descriptors{s}"], 480, 640, np.float64)
        assert np.abs(o.cpu().numpy() - ref).max() < 1e-5


@pytest.mark.parametrize("index,kind", [(0, "self"), (1, "cross")])
def test_stage_layer(index, kind):
    sd, model = _stage_model()
    rs = np.random.RandomState(23 + index)
    d0 = rs.normal(0, 0.5, size=(2, 256, 37)).astype(np.float32)
    d1 = rs.normal(0, 0.5, size=(2, 256, 53)).astype(np.float32)
    o0, o1 = model.engine.layer(index, torch.from_numpy(d0).to(DEV), torch.from_numpy(d1).to(DEV))
    r0, r1 = so.layer(sd, index, kind, d0.astype(np.float64), d1.astype(np.float64), np.float64)
    for o, r in ((o0, r0), (o1, r1)):
        err = np.abs(o.cpu().numpy() - r).max() / np.abs(r).max()
        assert err < 1e-5, err


@pytest.mark.parametrize("iters", [0, 1, 100])
def test_stage_sinkhorn(iters):
    _, model = _stage_model()
    rs = np.random.RandomState(30)
    sc = rs.normal(0, 2, size=(2, 45, 61)).astype(np.float32)
    z = model.engine.sinkhorn(torch.from_numpy(sc).to(DEV), 1.3, iters).cpu().numpy()
    ref = so.sinkhorn(sc.astype(np.float64), 1.3, iters, np.float64)
    assert np.abs(z - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())


def test_stage_match_tail_bit_consistent_with_ties():
    _, model = _stage_model()
    rs = np.random.RandomState(31)
    Z = rs.normal(-3, 1, size=(2, 70, 90)).astype(np.float32)
    Z[0, 5, 10] = Z[0, 5, 40] = 2.0          # tie in a row: column 10 wins
    Z[0, 60, 10] = 2.0                       # tie in a column: row 5 wins
    Z[1, :3, :3] = -0.05                     # a block of exact ties
    for th in (0.0, 0.2, 0.7):
        m0, m1, s0, s1 = (t.cpu().numpy() for t in model.engine.match_tail(torch.from_numpy(Z).to(DEV), th))
        ref = so.match_tail(Z, th)
        assert (m0 == ref["matches0"]).all() and (m1 == ref["matches1"]).all()
        np.testing.assert_allclose(s0, ref["matching_scores0"], rtol=1e-6, atol=0)
        np.testing.assert_allclose(s1, ref["matching_scores1"], rtol=1e-6, atol=0)
    assert m0[0, 5] == 10 and m1[0, 10] == 5 and m0[1, 0] == 0


def test_deterministic_and_four_in_flight():
    sd, inp, cfg, _ = case("tiny")
    model = build(sd, cfg)
    d = to_dev(inp)
    a = model(d)
    b = model(d)
    for k in a:
        assert torch.equal(a[k], b[k])
    ring = StreamRing(DEV)
    outs = []
    for _ in range(8):
        with ring.next():
            outs.append(model(d))
    ring.synchronize()
    for o in outs:
        for k in a:
            assert torch.equal(o[k], a[k])


@pytest.mark.parametrize("th", [0.0, 0.2, 0.7])
def test_thresholds_against_oracle(th):
    sd, inp, cfg, _ = case("tiny")
    cfg = dict(cfg, match_threshold=th)
    model = build(sd, cfg)
    out, Z = run_full(model, to_dev(inp))
    ref = so.match_tail(Z, th)        # the tail on the kernels' own Z is exact
    for k in ("matches0", "matches1"):
        assert (out[k] == ref[k]).all()
    if th == 0.0:
        assert (out["matches0"] >= 0).sum() > 0


def test_custom_layers_batch_and_side_stream():
    names = ["cross", "self", "cross"]
    sd = synthetic.make_superglue_state_dict(40, 3)
    cfg = {**SuperGlue.default_config, "GNN_layers": names, "sinkhorn_iterations": 20, "match_threshold": 0.0}
    model = build(sd, cfg)
    inp = synthetic.make_superglue_inputs(2, 64, 33, 300, 400, seed=41)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        d = to_dev(inp)
        out, Z = run_full(model, d)
    ref, rZ = so.forward(sd, inp, cfg, np.float64)
    assert np.abs(Z - rZ).max() < 2e-4
    c0 = (so.z_stats(rZ)["row_best"] - so.z_stats(rZ)["row_second"]) > 1e-4
    assert (out["matches0"][c0] == ref["matches0"][c0]).all()


def test_one_point_side():
    sd = synthetic.make_superglue_state_dict(42, 2)
    cfg = {**SuperGlue.default_config, "GNN_layers": ["self", "cross"], "match_threshold": 0.0}
    model = build(sd, cfg)
    inp = synthetic.make_superglue_inputs(1, 30, 1, 200, 200, seed=43)
    out, Z = run_full(model, to_dev(inp))
    ref, rZ = so.forward(sd, inp, cfg, np.float64)
    assert np.abs(Z - rZ).max() < 2e-4
    assert (out["matches1"] == ref["matches1"]).all()
