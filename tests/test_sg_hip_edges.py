"""SuperGlue HIP stages at the edges where tiled kernels go wrong, against the fp64 numpy oracle, on the MI355X.

Float bounds are relative to the fp32 oracle's own error on the same inputs: a kernel error may be at most C_REL times that of
the fp32 restatement, plus a floor of a few ulps of the output scale.  The shapes straddle every tile edge of the kernels:
the 64-source K/V tiles and 128-query blocks of sg_attn_kernel, the 64-lane row loop of sg_sk_rows_kernel, and the
64-row quarters and 256-row chunks of sg_col_partial_kernel.
"""
import json
import os

import numpy as np
import pytest
import torch

import superglue_oracle as so
from onepose_amd import SuperGlue, synthetic

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")
C_REL = 4.0          # kernel error <= C_REL * fp32-oracle error + floor (measured on the MI355X: at most 2.4)
ULP = 2.0 ** -23

ATTN_SHAPES = [(1, 1), (1, 200), (64, 64), (65, 127), (128, 129), (129, 65), (257, 700)]


def build(sd, cfg):
    m = SuperGlue(cfg).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def models():
    """Two-layer modules (self, cross): default weights and peaked attention (attn_gain 30)."""
    cfg = {"GNN_layers": ["self", "cross"]}
    out = {}
    for name, gain in (("default", 1.0), ("peaked", 30.0)):
        sd = synthetic.make_superglue_state_dict(60, 2, attn_gain=gain)
        out[name] = (sd, build(sd, cfg))
    return out


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def check_rel(name, got, ref64, ref32, scale=None):
    """max |got - ref64| <= C_REL * max |ref32 - ref64| + floor; prints both."""
    scale = float(np.abs(ref64).max()) if scale is None else scale
    ek = float(np.abs(got.astype(np.float64) - ref64).max())
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    floor = 4 * ULP * max(scale, 1e-30)
    print(f"\n{name}: kernel {ek:.3e}  fp32 oracle {e32:.3e}  scale {scale:.3e}  ratio {ek / max(e32, floor):.2f}")
    assert np.isfinite(got).all()
    assert ek <= C_REL * e32 + floor, (ek, e32, floor)
    return ek, e32


# ---------------------------------------------------------------------------------------------------------------------
# attention stage (sg_attention: the kernel of every layer, same launch shape)
# ---------------------------------------------------------------------------------------------------------------------
def attention_ref(q, kv, dt):
    """Head-contiguous q [b,256,N], kv [b,512,M] -> [b,256,N] (so._softmax, logits / 8)."""
    b, _, n = q.shape
    q, kv = q.astype(dt), kv.astype(dt)
    qh = q.reshape(b, 4, 64, n)
    kh = kv[:, :256].reshape(b, 4, 64, -1)
    vh = kv[:, 256:].reshape(b, 4, 64, -1)
    s = np.einsum("bhdn,bhdm->bhnm", qh, kh, optimize=True) / dt(8)
    return np.einsum("bhnm,bhdm->bhdn", so._softmax(s, -1), vh, optimize=True).reshape(b, 256, n)


def attention_inputs(b, n, m, spread, seed, peak=None):
    """q, kv with a median row logit spread of about `spread`.  peak = "last" / "first": one source (the last one, in the
    masked partial last tile when m % 64 != 0; or source 0, in the first tile) gets about 2 * spread added to its logit in
    every row and head, so that the row max lies there (in more than 99 % of the rows, checked)."""
    rs = np.random.RandomState(seed)
    q = rs.normal(size=(b, 256, n))
    kv = rs.normal(size=(b, 512, m))
    s = np.einsum("bhdn,bhdm->bhnm", q.reshape(b, 4, 64, n), kv[:, :256].reshape(b, 4, 64, m)) / 8
    med = float(np.median(s.max(-1) - s.min(-1))) if m > 1 else 1.0
    q *= np.sqrt(spread / med)
    kv[:, :256] *= np.sqrt(spread / med)
    if peak is not None:
        j = m - 1 if peak == "last" else 0
        # a shared direction u in every head's q and in k[:, j] only: the logit of source j rises by about 2 * spread
        u = rs.normal(size=(64,))
        u /= np.linalg.norm(u)
        for h in range(4):
            q[:, h * 64:(h + 1) * 64] += 4.0 * u[None, :, None] * np.sqrt(spread)
            kv[:, h * 64:(h + 1) * 64, j] += 4.0 * u[None, :] * np.sqrt(spread)
    return q.astype(np.float32), kv.astype(np.float32)


def _attention_case(models, b, n, m, spread, seed, peak=None):
    q, kv = attention_inputs(b, n, m, spread, seed, peak)
    got = models["default"][1].engine.attention(dev(q), dev(kv)).cpu().numpy()
    ref64 = attention_ref(q, kv, np.float64)
    ref32 = attention_ref(q, kv, np.float32)
    if peak is not None and m > 1:
        s = np.einsum("bhdn,bhdm->bhnm", q.astype(np.float64).reshape(b, 4, 64, n), kv[:, :256].astype(np.float64).reshape(b, 4, 64, m))
        want = m - 1 if peak == "last" else 0
        assert (s.argmax(-1) == want).mean() > 0.99
    check_rel(f"attention b={b} N={n} M={m} spread {spread} peak {peak}", got, ref64, ref32)


@pytest.mark.parametrize("spread", [0.5, 12.0, 80.0])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n,m", ATTN_SHAPES)
def test_attention_stage(models, n, m, b, spread):
    _attention_case(models, b, n, m, spread, seed=1000 + n + 7 * m + b)


@pytest.mark.parametrize("peak", ["last", "first"])
@pytest.mark.parametrize("n,m", [(65, 127), (129, 65), (257, 700), (128, 129), (1, 200)])
def test_attention_stage_row_max_position(models, n, m, peak):
    """Row max in the masked partial last tile (every earlier tile rescaled once more at the end) or in the first tile only."""
    _attention_case(models, 3, n, m, 12.0, seed=2000 + n + m, peak=peak)


def test_attention_stage_single_source_second_tile(models):
    """M = 65: the second K/V tile holds one source, 63 masked lanes; a large logit there must still win."""
    _attention_case(models, 3, 130, 65, 12.0, seed=3001, peak="last")
    _attention_case(models, 3, 130, 65, 80.0, seed=3002)


def test_attention_stage_rejects_bad_shapes(models):
    eng = models["default"][1].engine
    with pytest.raises(ValueError):
        eng.attention(torch.zeros(1, 256, 4, device=DEV), torch.zeros(1, 256, 4, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------
# layer stage: assert on the delta (out - in), where the residual cannot hide an attention error
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["default", "peaked"])
@pytest.mark.parametrize("index,kind", [(0, "self"), (1, "cross")])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n0,n1", ATTN_SHAPES)
def test_layer_stage_delta(models, n0, n1, b, index, kind, weights):
    sd, model = models[weights]
    rs = np.random.RandomState(4000 + n0 + 3 * n1 + b + 11 * index)
    sigma = 0.5 if weights == "default" else 0.08     # median row logit spread ~0.5 (default) / ~12 (peaked)
    d0 = rs.normal(0, sigma, size=(b, 256, n0)).astype(np.float32)
    d1 = rs.normal(0, sigma, size=(b, 256, n1)).astype(np.float32)
    o0, o1 = (o.cpu().numpy() for o in model.engine.layer(index, dev(d0), dev(d1)))
    r0, r1 = so.layer(sd, index, kind, d0.astype(np.float64), d1.astype(np.float64), np.float64)
    f0, f1 = so.layer(sd, index, kind, d0, d1, np.float32)
    for s, (o, r, f, d) in enumerate(((o0, r0, f0, d0), (o1, r1, f1, d1))):
        dref = r - d
        check_rel(f"layer {kind} {weights} b={b} {n0}/{n1} side {s} delta", o.astype(np.float64) - d, dref,
                  f.astype(np.float64) - d, scale=float(np.abs(dref).max()))


# ---------------------------------------------------------------------------------------------------------------------
# Sinkhorn
# ---------------------------------------------------------------------------------------------------------------------
SK_SHAPES = [(1, 1), (1, 300), (300, 1), (63, 64), (64, 65), (129, 257), (1000, 1500), (2048, 130)]
BINS = [-5.0, 0.0, 1.3, 8.0]


def sk_scores(kind, b, n0, n1, seed):
    rs = np.random.RandomState(seed)
    if kind == "normal2":
        sc = rs.normal(0, 2, size=(b, n0, n1))
    elif kind == "planted16":
        sc = rs.normal(0, 1, size=(b, n0, n1))
        k = min(n0, n1)
        for i in range(b):
            sc[i, rs.permutation(n0)[:k], rs.permutation(n1)[:k]] += 16.0
    else:   # +-60 magnitudes
        sc = rs.choice([-60.0, 60.0], size=(b, n0, n1)) * rs.uniform(0.5, 1.0, size=(b, n0, n1))
    return sc.astype(np.float32)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("shape", SK_SHAPES, ids=[f"{a}x{c}" for a, c in SK_SHAPES])
def test_sinkhorn_stage(models, shape, b):
    n0, n1 = shape
    eng = models["default"][1].engine
    si = SK_SHAPES.index(shape)
    for ki, kind in enumerate(("normal2", "planted16", "pm60")):
        bin_score = BINS[(si + ki + b) % 4]
        sc = sk_scores(kind, b, n0, n1, seed=5000 + 10 * si + ki + b)
        for iters in (0, 1, 3, 100):
            z = eng.sinkhorn(dev(sc), bin_score, iters).cpu().numpy()
            ref64 = so.sinkhorn(sc.astype(np.float64), bin_score, iters, np.float64)
            ref32 = so.sinkhorn(sc, bin_score, iters, np.float32)
            check_rel(f"sinkhorn b={b} {n0}x{n1} {kind} bin {bin_score} iters {iters}", z, ref64, ref32,
                      scale=max(1.0, float(np.abs(ref64).max())))


def test_sinkhorn_every_bin_score_on_every_shape_class(models):
    """The rotation above gives each shape three of the four bin scores; this covers the fourth on the multi-lane shapes."""
    eng = models["default"][1].engine
    for si, (n0, n1) in enumerate(SK_SHAPES):
        used = {BINS[(si + ki + b) % 4] for ki in range(3) for b in (1, 3)}
        for bin_score in sorted(set(BINS) - used):
            sc = sk_scores("normal2", 1, n0, n1, seed=6000 + si)
            z = eng.sinkhorn(dev(sc), bin_score, 100).cpu().numpy()
            ref64 = so.sinkhorn(sc.astype(np.float64), bin_score, 100, np.float64)
            check_rel(f"sinkhorn b=1 {n0}x{n1} normal2 bin {bin_score} iters 100", z, ref64, so.sinkhorn(sc, bin_score, 100, np.float32),
                      scale=max(1.0, float(np.abs(ref64).max())))


# ---------------------------------------------------------------------------------------------------------------------
# match tail: exactly the oracle's matches, ties planted across lane strides, quarters and chunks
# ---------------------------------------------------------------------------------------------------------------------
TAIL_N0 = [1, 63, 64, 65, 255, 256, 257, 513, 1030]
TAIL_N1 = [1, 63, 64, 65, 129, 700]


def tail_z(n0, n1, seed):
    rs = np.random.RandomState(seed)
    b = 3
    Z = rs.normal(-3, 1, size=(b, n0 + 1, n1 + 1)).astype(np.float32)
    for i in range(b):
        z = Z[i]
        # a constant row and a constant column
        if n0 > 2:
            z[n0 // 2, :n1] = np.float32(-0.5)
        if n1 > 2:
            z[:n0, n1 // 3] = np.float32(-0.25)
        # -inf entries
        z[:n0, :n1][rs.rand(n0, n1) < 0.05] = -np.inf
        if i == 2 and n0 > 1:
            z[1, :n1] = -np.inf             # a row of -inf only: first index wins
        v = np.float32(2.0 + i)              # above every random entry
        # row ties within one lane's stride: (r, j) and (r, j + 64)
        r = rs.randint(n0)
        j = rs.randint(max(1, n1 - 64)) if n1 > 64 else 0
        z[r, j] = v
        if j + 64 < n1:
            z[r, j + 64] = v
        # column ties across quarter / chunk boundaries: rows 63/64, 255/256, r/r+512 of one column each
        for k, (ra, rb) in enumerate(((63, 64), (255, 256), (i, i + 512))):
            c = (7 * k + 3 * i + 1) % n1
            if rb < n0:
                z[ra, c] = z[rb, c] = np.float32(v + 1 + k)
    return Z


@pytest.mark.parametrize("n1", TAIL_N1)
@pytest.mark.parametrize("n0", TAIL_N0)
def test_match_tail_exact(models, n0, n1):
    eng = models["default"][1].engine
    Z = tail_z(n0, n1, seed=7000 + n0 * 7 + n1)
    for th in (0.0, 0.2, 1.0):
        m0, m1, s0, s1 = (t.cpu().numpy() for t in eng.match_tail(dev(Z), th))
        ref = so.match_tail(Z, th)
        assert (m0 == ref["matches0"]).all(), th
        assert (m1 == ref["matches1"]).all(), th
        np.testing.assert_allclose(s0, ref["matching_scores0"], rtol=1e-6, atol=0)
        np.testing.assert_allclose(s1, ref["matching_scores1"], rtol=1e-6, atol=0)


def test_match_tail_score_equal_to_threshold_is_invalid(models):
    """Z = 0 everywhere: every score is exp(0) = 1 = threshold, so nothing is valid; with ties everywhere, row 0 and column 0
    are the only mutual pair."""
    eng = models["default"][1].engine
    Z = np.zeros((3, 258, 131), np.float32)
    m0, m1, s0, s1 = (t.cpu().numpy() for t in eng.match_tail(dev(Z), 1.0))
    ref = so.match_tail(Z, 1.0)
    assert (m0 == -1).all() and (m1 == -1).all()
    assert (s0 == ref["matching_scores0"]).all() and (s1 == ref["matching_scores1"]).all()
    assert s0[:, 0].tolist() == [1.0] * 3 and (s0[:, 1:] == 0).all()
    m0, _, _, _ = (t.cpu().numpy() for t in eng.match_tail(dev(Z), 0.99))
    assert m0[:, 0].tolist() == [0] * 3 and (m0[:, 1:] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------
# keypoint encoder: per-side image sizes, keypoints outside the image
# ---------------------------------------------------------------------------------------------------------------------
KENC_SIZES = [((480, 640), (640, 480)), ((640, 480), (481, 641)), ((481, 641), (1, 1)), ((1, 1), (480, 640))]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("sizes", KENC_SIZES, ids=["480x640-640x480", "640x480-481x641", "481x641-1x1", "1x1-480x640"])
def test_keypoint_encoder_sizes(models, sizes, n):
    sd, model = models["default"]
    (h0, w0), (h1, w1) = sizes
    n1 = max(1, n // 2 + 1)
    rs = np.random.RandomState(8000 + n + h0)
    inp = {}
    for s, (h, w), nn in ((0, (h0, w0), n), (1, (h1, w1), n1)):
        # a quarter of the image beyond every edge: some keypoints lie outside it
        x = rs.uniform(-0.25 * w, 1.25 * w, size=(3, nn))
        y = rs.uniform(-0.25 * h, 1.25 * h, size=(3, nn))
        inp[f"k{s}"] = np.stack([x, y], -1).astype(np.float32)
        inp[f"s{s}"] = rs.uniform(0, 1, size=(3, nn)).astype(np.float32)
        inp[f"d{s}"] = rs.normal(0, 0.1, size=(3, 256, nn)).astype(np.float32)
    o0, o1 = model.engine.keypoint_encode(dev(inp["k0"]), dev(inp["s0"]), dev(inp["d0"]), dev(inp["k1"]), dev(inp["s1"]),
                                          dev(inp["d1"]), (h0, w0), (h1, w1))
    err = 0.0
    for o, s, (h, w) in ((o0, 0, (h0, w0)), (o1, 1, (h1, w1))):
        ref = so.keypoint_encode(sd, inp[f"k{s}"], inp[f"s{s}"], inp[f"d{s}"], h, w, np.float64)
        err = max(err, float(np.abs(o.cpu().numpy() - ref).max()))
    print(f"\nkenc {sizes} n={n}/{n1}: max|err| {err:.3e}")
    assert err < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# forward through the module with per-side image sizes; batch independence
# ---------------------------------------------------------------------------------------------------------------------
def _golden_case(name):
    with open(os.path.join(GOLD, "sg_golden_meta.json")) as f:
        spec = json.load(f)["cases"][name]
    w = {k: v for k, v in spec["w"].items() if k not in ("kind", "seed")}
    sd = synthetic.make_superglue_state_dict(spec["w"]["seed"], len(spec["cfg"]["GNN_layers"]), **w)
    return sd, synthetic.make_superglue_inputs(**spec["inp"]), spec["cfg"], dict(np.load(os.path.join(GOLD, f"sg_{name}.npz")))


IN_KEYS = ("keypoints0", "scores0", "descriptors0", "keypoints1", "scores1", "descriptors1")


def test_sizes_golden_through_module_forward():
    """SuperGlue.forward(data) reads each side's size from image0 / image1 of different shapes."""
    sd, inp, cfg, gold = _golden_case("sizes")
    model = build(sd, dict(cfg, match_threshold=0.0))
    data = {k: dev(inp[k]) for k in IN_KEYS}
    b = inp["keypoints0"].shape[0]
    (h0, w0), (h1, w1) = inp["image_size0"], inp["image_size1"]
    assert (h0, w0) != (h1, w1) and h1 > w1
    data["image0"] = torch.empty(b, 1, int(h0), int(w0), device=DEV)
    data["image1"] = torch.empty(b, 1, int(h1), int(w1), device=DEV)
    pred = {k: v.cpu().numpy() for k, v in model(data).items()}
    ref, _ = so.forward(sd, inp, dict(cfg, match_threshold=0.0), np.float64)
    st = so.z_stats(gold["Z"].astype(np.float64))
    c0 = st["row_best"] - st["row_second"] > 1e-4
    serr = max(float(np.abs(pred[k] - ref[k]).max()) for k in ("matching_scores0", "matching_scores1"))
    print(f"\nsizes via forward(data): score err vs fp64 oracle {serr:.3e}  clear rows {c0.mean():.3f}")
    assert serr < so.FORWARD_STOL
    assert (pred["matches0"][c0] == ref["matches0"][c0]).all()
    # the golden's own threshold: the module's outputs equal the reference run's
    model = build(sd, cfg)
    pred = {k: v.cpu().numpy() for k, v in model(data).items()}
    assert (pred["matches0"][c0] == gold["matches0"][c0]).all()
    serr = max(float(np.abs(pred[k] - gold[k]).max()) for k in ("matching_scores0", "matching_scores1"))
    assert serr < so.FORWARD_STOL


@pytest.mark.parametrize("name", ["sizes", "peaked"])
def test_batch_items_independent(name):
    """Item i of a b = 3 forward is bitwise the same item run alone (the kernels reduce in a fixed order and carry the batch as
    a grid dimension: any difference is a stride bug)."""
    sd, inp, cfg, _ = _golden_case(name)
    if inp["keypoints0"].shape[0] == 1:      # make a batch of three different items from three seeds
        spec = dict(b=3, n0=inp["keypoints0"].shape[1], n1=inp["keypoints1"].shape[1], h=int(inp["image_size0"][0]),
                    w=int(inp["image_size0"][1]), h1=int(inp["image_size1"][0]), w1=int(inp["image_size1"][1]), seed=77)
        inp = synthetic.make_superglue_inputs(**spec)
    model = build(sd, cfg)
    b, n0, n1 = inp["keypoints0"].shape[0], inp["keypoints0"].shape[1], inp["keypoints1"].shape[1]
    hw0, hw1 = tuple(int(x) for x in inp["image_size0"]), tuple(int(x) for x in inp["image_size1"])

    def run(sl):
        z = torch.empty(sl.stop - sl.start, n0 + 1, n1 + 1, device=DEV)
        out = model.engine.forward(*(dev(inp[k][sl]) for k in IN_KEYS), hw0, hw1, z_out=z)
        return [o.cpu().numpy() for o in out] + [z.cpu().numpy()]
    full = run(slice(0, b))
    for i in range(b):
        one = run(slice(i, i + 1))
        for a, c in zip(full, one):
            assert a[i:i + 1].tobytes() == c.tobytes(), i
