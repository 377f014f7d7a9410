"""The ragged batch of the HIP SuperGlue matcher on the MI355X: every item of a ragged launch is BITWISE the same pair run alone
through the uniform entry points (forward and the three stages), whatever the other items, the capacities, the padding (NaN)
and the workspace contents (NaN) are; plus one fp64-oracle check so the feature is pinned against something else than the
old path.  Shapes straddle the 64-source K/V tile, the 128-query block, the 4-row Sinkhorn block and the 256-row column chunk."""
import numpy as np
import pytest
import torch

import superglue_oracle as so
from onepose_amd import SuperGlue, synthetic
from test_sg_hip_edges import C_REL, attention_inputs, build, check_rel, dev, sk_scores

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")

SHAPES = [(1, 1), (64, 65), (129, 63), (257, 130), (63, 130)]         # caps 257 / 130; item 3 sits at both
SIZES = [(480, 640), (640, 480), (700, 300), (1, 1)]
IN_KEYS = ("keypoints0", "scores0", "descriptors0", "keypoints1", "scores1", "descriptors1")


@pytest.fixture(scope="module")
def models():
    cfg = {"GNN_layers": ["self", "cross"]}
    out = {}
    for name, gain in (("default", 1.0), ("peaked", 30.0)):
        sd = synthetic.make_superglue_state_dict(60, 2, attn_gain=gain)
        out[name] = (sd, build(sd, cfg))
    return out


def make_items(shapes, seed):
    """Per item: numpy inputs of synthetic.make_superglue_inputs at its own counts and image sizes."""
    items = []
    for k, (n0, n1) in enumerate(shapes):
        (h0, w0), (h1, w1) = SIZES[k % 4], SIZES[(k + 1) % 4]
        items.append(synthetic.make_superglue_inputs(b=1, n0=n0, n1=n1, h=h0, w=w0, h1=h1, w1=w1, seed=seed + k, planted=min(n0, n1) // 2))
    return items


def pad(items, fill=NAN):
    """Padded device tensors with `fill` past every item's counts, and the host lists."""
    b, cap0, cap1 = len(items), max(i["keypoints0"].shape[1] for i in items), max(i["keypoints1"].shape[1] for i in items)
    shapes = {"keypoints0": (b, cap0, 2), "scores0": (b, cap0), "descriptors0": (b, 256, cap0), "keypoints1": (b, cap1, 2),
              "scores1": (b, cap1), "descriptors1": (b, 256, cap1)}
    out = {}
    for key, shape in shapes.items():
        t = np.full(shape, fill, np.float32)
        for i, it in enumerate(items):
            n = it[key].shape[2 if key.startswith("desc") else 1]
            if key.startswith("desc"):
                t[i, :, :n] = it[key][0]
            else:
                t[i, :n] = it[key][0]
        out[key] = dev(t)
    n0, n1 = [i["keypoints0"].shape[1] for i in items], [i["keypoints1"].shape[1] for i in items]
    hw0, hw1 = [tuple(int(x) for x in i["image_size0"]) for i in items], [tuple(int(x) for x in i["image_size1"]) for i in items]
    return out, n0, n1, hw0, hw1


def run_ragged(model, items, poison=True):
    p, n0, n1, hw0, hw1 = pad(items)
    b, cap0, cap1 = len(items), max(n0), max(n1)
    if poison:
        model.engine.ragged_workspace(b, cap0, cap1, DEV).fill_(0xFF)       # every float of the workspace is a NaN
    z = torch.full((b, cap0 + 1, cap1 + 1), NAN, device=DEV)
    out = model.engine.forward_ragged(*(p[k] for k in IN_KEYS), n0, n1, hw0, hw1, z_out=z)
    return [o.clone() for o in out], z


def run_alone(model, it):
    n0, n1 = it["keypoints0"].shape[1], it["keypoints1"].shape[1]
    z = torch.empty(1, n0 + 1, n1 + 1, device=DEV)
    out = model.engine.forward(*(dev(it[k]) for k in IN_KEYS), tuple(int(x) for x in it["image_size0"]),
                               tuple(int(x) for x in it["image_size1"]), z_out=z)
    return [o.clone() for o in out], z


def assert_items_equal_alone(model, items, out, z):
    for i, it in enumerate(items):
        n0, n1 = it["keypoints0"].shape[1], it["keypoints1"].shape[1]
        ref, zr = run_alone(model, it)
        for got, want, n in zip(out, ref, (n0, n1, n0, n1)):
            assert torch.equal(got[i, :n], want[0]), (i, n0, n1)
            assert bool((got[i, n:] == (-1 if got.dtype == torch.int64 else 0)).all()), (i, "past the count")
        assert torch.equal(z[i, :n0 + 1, :n1 + 1], zr[0]), (i, n0, n1)
        assert bool(torch.isfinite(zr).all())


@pytest.mark.parametrize("iters", [0, 1, 100])
@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("weights", ["default", "peaked"])
def test_forward_ragged_items_are_bitwise_the_item_alone(models, weights, order, iters):
    _, model = models[weights]
    items = make_items(SHAPES, 300)
    if order == "reversed":
        items = items[::-1]
    model.config["sinkhorn_iterations"] = iters
    try:
        out, z = run_ragged(model, items)
        assert_items_equal_alone(model, items, out, z)
    finally:
        model.config["sinkhorn_iterations"] = 100


def test_forward_ragged_eighteen_peaked_layers():
    sd = synthetic.make_superglue_state_dict(61, 18, attn_gain=30.0)
    model = build(sd, {"sinkhorn_iterations": 100})
    items = make_items([(300, 517), (37, 53), (129, 65)], 400)
    out, z = run_ragged(model, items)
    assert_items_equal_alone(model, items, out, z)


def test_forward_ragged_isolation_and_repeatability(models):
    _, model = models["peaked"]
    items = make_items(SHAPES, 300)
    out, z = run_ragged(model, items)
    # two runs, and two runs on two streams (each stream has its own workspace)
    out2, z2 = run_ragged(model, items, poison=False)
    assert all(torch.equal(a, c) for a, c in zip(out, out2)) and z.cpu().numpy().tobytes() == z2.cpu().numpy().tobytes()
    res = []
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    torch.cuda.synchronize()
    for s in streams:
        with torch.cuda.stream(s):
            res.append(run_ragged(model, items, poison=False))
    torch.cuda.synchronize()
    for o, zz in res:
        assert all(torch.equal(a, c) for a, c in zip(out, o)) and z.cpu().numpy().tobytes() == zz.cpu().numpy().tobytes()
    # another item j (other data, same counts) leaves every other item's outputs unchanged
    j = 3
    other = list(items)
    other[j] = make_items(SHAPES, 900)[j]
    out3, z3 = run_ragged(model, other)
    changed = False
    for i, (n0, n1) in enumerate(SHAPES):
        same = all(torch.equal(a[i], c[i]) for a, c in zip(out, out3)) and torch.equal(z[i, :n0 + 1, :n1 + 1], z3[i, :n0 + 1, :n1 + 1])
        if i == j:
            changed = not same
        else:
            assert same, i
    assert changed


def test_forward_ragged_against_the_fp64_oracle(models):
    """Z of every item within C_REL times the fp32 oracle's own error plus 4 ulps of the output scale."""
    sd, model = models["default"]
    items = make_items(SHAPES, 300)
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 100, "match_threshold": 0.2}
    out, z = run_ragged(model, items)
    for i, it in enumerate(items):
        n0, n1 = SHAPES[i]
        _, z64 = so.forward(sd, it, cfg, np.float64)
        _, z32 = so.forward(sd, it, cfg, np.float32)
        check_rel(f"ragged item {i} {n0}/{n1} Z", z[i:i + 1, :n0 + 1, :n1 + 1].cpu().numpy(), z64, z32, scale=max(1.0, float(np.abs(z64).max())))
    assert C_REL == 4.0


# ---------------------------------------------------------------------------------------------------------------------
# stages
# ---------------------------------------------------------------------------------------------------------------------
ATTN_NM = [(1, 1), (1, 200), (65, 127), (128, 129), (257, 700)]


@pytest.mark.parametrize("spread", [12.0, 80.0])
def test_attention_ragged_is_bitwise_the_item_alone(models, spread):
    """Mixed N / M in one batch; every item's row maximum is planted in its last source, i.e. in the masked partial last K/V
    tile wherever M is not a multiple of 64."""
    eng = models["default"][1].engine
    capn, capm = max(n for n, _ in ATTN_NM), max(m for _, m in ATTN_NM)
    q = np.full((len(ATTN_NM), 256, capn), NAN, np.float32)
    kv = np.full((len(ATTN_NM), 512, capm), NAN, np.float32)
    alone = []
    for i, (n, m) in enumerate(ATTN_NM):
        qi, kvi = attention_inputs(1, n, m, spread, seed=1500 + i, peak="last")
        q[i, :, :n], kv[i, :, :m] = qi[0], kvi[0]
        alone.append(eng.attention(dev(qi), dev(kvi)))
    got = eng.attention_ragged(dev(q), dev(kv), [n for n, _ in ATTN_NM], [m for _, m in ATTN_NM])
    for i, (n, m) in enumerate(ATTN_NM):
        assert torch.equal(got[i, :, :n], alone[i][0]), (n, m)
        assert bool(torch.isfinite(alone[i]).all())
        assert bool((got[i, :, n:] == 0).all())                 # columns past the count are not written


SK_NM = [(1, 1), (1, 300), (300, 1), (63, 64), (129, 257)]


@pytest.mark.parametrize("bin_score", [-5.0, 8.0])
@pytest.mark.parametrize("iters", [0, 3, 100])
def test_sinkhorn_ragged_is_bitwise_the_item_alone(models, bin_score, iters):
    eng = models["default"][1].engine
    cap0, cap1 = max(a for a, _ in SK_NM), max(c for _, c in SK_NM)
    sc = np.full((len(SK_NM), cap0, cap1), NAN, np.float32)
    alone = []
    for i, (n0, n1) in enumerate(SK_NM):
        s = sk_scores("pm60", 1, n0, n1, seed=5500 + i)
        sc[i, :n0, :n1] = s[0]
        alone.append(eng.sinkhorn(dev(s), bin_score, iters))
    eng.ragged_workspace(len(SK_NM), cap0, cap1, DEV).fill_(0xFF)
    z = eng.sinkhorn_ragged(dev(sc), bin_score, [a for a, _ in SK_NM], [c for _, c in SK_NM], iters)
    for i, (n0, n1) in enumerate(SK_NM):
        assert torch.equal(z[i, :n0 + 1, :n1 + 1], alone[i][0]), (n0, n1)
        assert bool(torch.isfinite(alone[i]).all())


def test_match_tail_ragged_ties_in_items_that_are_not_the_largest(models):
    """Row ties 64 columns apart and column ties across rows 63/64 and 255/256 (the quarter and chunk edges of the column
    kernel), in items smaller than the capacities; one item has a row of -inf only."""
    eng = models["default"][1].engine
    shapes = [(300, 150), (257, 130), (600, 200), (65, 70)]
    cap0, cap1 = 600, 200
    rs = np.random.RandomState(7100)
    Z = np.full((len(shapes), cap0 + 1, cap1 + 1), NAN, np.float32)
    alone = []
    for i, (n0, n1) in enumerate(shapes):
        z = rs.normal(-3, 1, size=(1, n0 + 1, n1 + 1)).astype(np.float32)
        v = np.float32(2.0 + i)
        r, j = n0 // 3, 1 + i
        z[0, r, j] = z[0, r, j + 64] = v                               # one lane meets both: the first index wins
        for k, (ra, rb) in enumerate(((63, 64), (255, 256))):
            if rb < n0:
                z[0, ra, 5 + 7 * k] = z[0, rb, 5 + 7 * k] = np.float32(v + 1 + k)
        if i == 1:
            z[0, 1, :n1] = -np.inf
        Z[i, :n0 + 1, :n1 + 1] = z[0]
        alone.append((eng.match_tail(dev(z), 0.0), so.match_tail(z, 0.0), (r, j)))
    eng.ragged_workspace(len(shapes), cap0, cap1, DEV).fill_(0xFF)
    got = eng.match_tail_ragged(dev(Z), [a for a, _ in shapes], [c for _, c in shapes], 0.0)
    for i, (n0, n1) in enumerate(shapes):
        one, ref, (r, j) = alone[i]
        for g, w, n in zip(got, one, (n0, n1, n0, n1)):
            assert torch.equal(g[i, :n], w[0]), (i, n0, n1)
            assert bool((g[i, n:] == (-1 if g.dtype == torch.int64 else 0)).all())
        assert (got[0][i, :n0].cpu().numpy() == ref["matches0"][0]).all() and (got[1][i, :n1].cpu().numpy() == ref["matches1"][0]).all()
        assert int(got[0][i, r]) in (j, -1) and int(got[0][i, r]) != j + 64
        if n0 > 256:
            assert int(got[1][i, 5]) == 63 and int(got[1][i, 12]) == 255


# ---------------------------------------------------------------------------------------------------------------------
# module: match_pairs
# ---------------------------------------------------------------------------------------------------------------------
def data_of(it):
    d = {k: dev(it[k]) for k in IN_KEYS}
    d["image0"] = torch.empty(1, 1, *(int(x) for x in it["image_size0"]), device="meta")
    d["image1"] = torch.empty(1, 1, *(int(x) for x in it["image_size1"]), device="meta")
    return d


@pytest.mark.parametrize("max_items", [2, 16])
def test_match_pairs_with_an_empty_side_in_the_middle(models, max_items):
    _, model = models["peaked"]
    datas = [data_of(it) for it in make_items([(64, 65), (129, 63), (5, 9), (63, 130)], 300)]
    empty = data_of(make_items([(7, 3)], 1)[0])
    empty["keypoints1"], empty["scores1"], empty["descriptors1"] = empty["keypoints1"][:, :0], empty["scores1"][:, :0], empty["descriptors1"][:, :, :0]
    datas.insert(2, empty)
    got = model.match_pairs(datas, max_items=max_items)
    assert len(got) == 5
    for i, (d, g) in enumerate(zip(datas, got)):
        want = model(d)
        assert set(g) == set(want) == {"matches0", "matches1", "matching_scores0", "matching_scores1"}
        for k in want:
            assert g[k].shape == want[k].shape and g[k].dtype == want[k].dtype and torch.equal(g[k], want[k]), (i, k)
    assert got[2]["matches0"].tolist() == [[-1] * 7] and got[2]["matches1"].shape == (1, 0) and got[2]["matches0"].dtype == torch.int
