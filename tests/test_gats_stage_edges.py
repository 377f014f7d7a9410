"""GATsSPG HIP stages at the edges where tiled kernels go wrong, against float64 restatements (tests/gats_stage_reference.py),
on the MI355X.

Rule (the same as tests/test_sg_hip_edges.py): a kernel's error against the float64 restatement may be at most C_REL
times the error of the float32 restatement of the same stage on the same inputs, plus 4 fp32 ulps of the output scale.  It is
applied to the arithmetics include/gatsspg.h calls fp32-class (fp32, bf16x6, fp16x4); the three-term modes (bf16x3, fp16x3) run
the same shapes through the same kernels and are held to the absolute STAGE_ATOL of tests/test_hip_parity.py.

Every case fills the engine's workspace with NaN before it loads the state, so a kernel that reads a column, a partial or a
counter it did not write shows up as a non-finite output.  The attention cases assert on the delta (state out - state in) per
side, where the residual cannot hide an error.  The shapes straddle the 64-column tiles of qkv_kv / mlp0 / mlp3, the 128-column
segment padding, the 4-point leaf tiles of the GATs kernels, the 128 x 64 tiles / 16-row strips / 512-column chunks of the score
and finalize kernels, and every launch-size threshold between two forms of a kernel (the table of gats_stage_reference.FORM_CASES,
which tests/test_gats_stage_reference.py checks against the launchers on the CPU).
"""
import functools

import numpy as np
import pytest
import torch

import gats_stage_reference as R
from conftest import TIE_GAP
from oracle import gatsspg_oracle as orc
from onepose_amd import GATsSuperGlue, synthetic, _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HP = dict(orc.DEFAULT_HPARAMS, match_threshold=0.0)
C_REL = 4.0                                # measured on the MI355X: at most 2.1
ULP = 2.0 ** -23
STAGE_ATOL = 2e-5                          # tests/test_hip_parity.py: the bar of the per-stage tensors (measured here: bf16x3 up to 1.6e-5, fp16x3 1.6e-6)
FP32_CLASS = ("fp32", "bf16x6", "fp16x4")
PRECISIONS = ["fp32", "bf16x3", "bf16x6", "fp16x3", "fp16x4"]
LEAF = 8                                   # num_leaf of the attention / score workspaces (those stages never read the leaves)


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)     # a copy: the shared references are read-only


def build(sd, precision="fp32"):
    m = GATsSuperGlue(HP, precision=precision).eval()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def weights():
    return synthetic.make_state_dict(0)


@functools.lru_cache(maxsize=None)
def model(precision):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return build(weights(), precision)


def poisoned_state(eng, x, y, num_leaf):
    """NaN over the whole workspace of these dims, then the state load: everything a stage reads it must have written."""
    dims = (x.shape[0], x.shape[2], y.shape[2], num_leaf, DEV)
    ws = eng.workspace(*dims)
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    return eng.load_state(dev(x), dev(y), num_leaf)


def check_rel(name, got, ref64, ref32, scale=None):
    """max |got - ref64| <= C_REL * max |ref32 - ref64| + 4 ulps of the scale; prints both errors and their ratio."""
    scale = float(np.abs(ref64).max()) if scale is None else scale
    assert np.isfinite(got).all(), name
    ek = float(np.abs(got.astype(np.float64) - ref64).max())
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    floor = 4 * ULP * max(scale, 1e-30)
    print(f"\n{name}: kernel {ek:.3e}  fp32 restatement {e32:.3e}  scale {scale:.3e}  ratio {ek / max(e32, floor):.2f}")
    assert ek <= C_REL * e32 + floor, (name, ek, e32, floor)
    return ek, e32


# ---------------------------------------------------------------------------------------------------------------------
# attention layer: one 'self' (attention layer 0 = gnn.layers.1) or 'cross' (1 = gnn.layers.2) layer on both sides
# ---------------------------------------------------------------------------------------------------------------------
ATTN_KINDS = {"self": (0, _native.LAYER_SELF, "gnn.layers.1"), "cross": (1, _native.LAYER_CROSS, "gnn.layers.2")}


@functools.lru_cache(maxsize=2)
def attention_reference(b, n1, n2, kind):
    """Inputs and the deltas of both sides in float64 and float32, computed once for all arithmetics of a shape."""
    x, y = R.attention_inputs(b, n1, n2)
    prefix = ATTN_KINDS[kind][2]
    d64 = R.attention_layer_deltas(weights(), prefix, x, y, kind, np.float64)
    d32 = R.attention_layer_deltas(weights(), prefix, x, y, kind, np.float32)
    for a in (x, y) + d64 + d32:
        a.setflags(write=False)
    return x, y, d64, d32


def _partial_tile_split(err, n):
    """Largest error on the columns of the last, partial 64-column tile and on the columns before it."""
    first = n // 64 * 64
    last = float(err[:, :, first:].max()) if first < n else float("nan")
    inner = float(err[:, :, :first].max()) if first > 0 else float("nan")
    return last, inner


def attention_case(what, precision, b, n1, n2, kind):
    x, y, d64, d32 = attention_reference(b, n1, n2, kind)
    layer, flag, _ = ATTN_KINDS[kind]
    eng = model(precision).engine
    dims = poisoned_state(eng, x, y, LEAF)
    eng.attn_layer(dims, layer, flag)
    outs = eng.store_state(dims)
    for side, (o, inp) in enumerate(zip(outs, (x, y))):
        o = o.cpu().numpy()
        name = f"attention[{what}] {kind} {precision} b={b} n1={n1} n2={n2} {'2D' if side == 0 else '3D'}"
        assert np.isfinite(o).all(), name
        delta = o.astype(np.float64) - inp.astype(np.float64)
        if precision in FP32_CLASS:
            check_rel(name, delta, d64[side], d32[side])
        else:
            err = np.abs(delta - d64[side])
            last, inner = _partial_tile_split(err, inp.shape[2])
            print(f"\n{name}: three-term error {err.max():.3e} (last partial tile {last:.3e}, columns before it {inner:.3e}; "
                  f"largest delta {np.abs(d64[side]).max():.3e})")
            assert err.max() < STAGE_ATOL, (name, float(err.max()))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("b", R.ATTN_B)
@pytest.mark.parametrize("n1,n2", R.ATTN_EDGE_SHAPES)
def test_attention_layer_segment_edges(n1, n2, b, kind, precision):
    """Segments that end on, one short of and one past a 64-column tile and the 128-column padding; the small form of every
    kernel (at most 30 tiles)."""
    attention_case("edges", precision, b, n1, n2, kind)


FORM_PARAMS = [pytest.param(purpose, b, n2, prec, id=f"{purpose.replace(' ', '_').replace(',', '')}-{prec}")
               for purpose, b, n2, _, precs in R.FORM_CASES for prec in precs]


@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("purpose,b,n2,precision", FORM_PARAMS)
def test_attention_layer_kernel_form_edges(purpose, b, n2, precision, kind):
    """Launch sizes on either side of every threshold between two forms of a kernel: the register-diet forms of the fp32
    qkv_kv / mlp0, Mlp3TileS against Mlp3TileTallW8, the narrow and the 128-column fp16 mlp0 tile, the three- and the
    two-stage ring of the fp16 mlp3."""
    attention_case(purpose, precision, b, R.FORM_N1, n2, kind)


# ---------------------------------------------------------------------------------------------------------------------
# GATs layer
# ---------------------------------------------------------------------------------------------------------------------
GATS_FLAGS = (1, 0, 3, 5, 7, 4)


@pytest.mark.parametrize("num_leaf", [8, 1, 3, 64])
@pytest.mark.parametrize("n2", [2, 3, 4, 5, 63, 64, 65, 129])
def test_gats_layer_leaf_tile_edges(n2, num_leaf):
    """Point counts around the 4-point leaf tiles of gats_leaf8x4_kernel (num_leaf = 8) and the generic kernel's tiles, every
    flag combination (the with_linear_transform ones run gats_wlt_kernel behind it), the first and the last GATs layer."""
    b, n1 = 2, 7
    sd = weights()
    data = synthetic.make_inputs(b=b, n1=n1, n2=n2, num_leaf=num_leaf, seed=300 + 7 * n2 + num_leaf)
    x, y, leaves = data["descriptors2d_query"], data["descriptors3d_db"], data["descriptors2d_db"]
    h2, h3 = np.transpose(leaves, (0, 2, 1)), np.transpose(y, (0, 2, 1))
    eng = model("fp32").engine
    d_leaves = dev(leaves)
    for layer in (0, 3):
        W, a = sd[f"gnn.layers.{3 * layer}.W"], sd[f"gnn.layers.{3 * layer}.a"]
        for flags in GATS_FLAGS:
            inc, add, wlt = bool(flags & 1), bool(flags & 2), bool(flags & 4)
            ref64 = np.transpose(R.graph_attention_layer(W, a, h2, h3, inc, add, wlt, np.float64), (0, 2, 1))
            ref32 = np.transpose(R.graph_attention_layer(W, a, h2, h3, inc, add, wlt, np.float32), (0, 2, 1))
            dims = poisoned_state(eng, x, y, num_leaf)
            eng.gats_layer(dims, layer, d_leaves, flags=flags)
            o2, o3 = eng.store_state(dims)
            assert torch.equal(o2.cpu(), torch.from_numpy(x)), "the GATs layer must not touch the 2D side"
            check_rel(f"gats layer {layer} flags {flags} L={num_leaf} n2={n2}", o3.cpu().numpy(), ref64, ref32)


# ---------------------------------------------------------------------------------------------------------------------
# final_proj + normalise, score / dual softmax / match (fp32 stage entries)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def score_reference(b, n1, n2, scale):
    x, y = R.score_inputs(b, n1, n2)
    r64 = R.score_reference(weights(), x, y, scale, np.float64)
    r32 = R.score_reference(weights(), x, y, scale, np.float32)
    return x, y, r64, r32


@pytest.mark.parametrize("scale", R.SCORE_SCALES)
@pytest.mark.parametrize("b", R.SCORE_B)
@pytest.mark.parametrize("n1,n2", R.SCORE_SHAPES)
def test_final_proj_and_score_stage_edges(n1, n2, b, scale):
    """Row counts around the 128-row score tiles and 16-row finalize strips, column counts around the 64-column score tiles and
    512-column finalize chunks, n2 % 4 != 0 (scalar finalize), planted pairs with conf of O(1); scale_factor 0.07 takes the
    one-pass dual softmax, 0.01 the max-subtracting one."""
    x, y, (m2_64, m3_64, c64), (m2_32, m3_32, c32) = score_reference(b, n1, n2, scale)
    what = f"b={b} n1={n1} n2={n2} scale {scale}"
    eng = model("fp32").engine
    dims = poisoned_state(eng, x, y, LEAF)
    eng.final_proj_norm(dims)
    m2, m3 = eng.store_state(dims, which=1)
    check_rel(f"final_proj_norm 2D {what}", m2.cpu().numpy(), m2_64, m2_32)
    check_rel(f"final_proj_norm 3D {what}", m3.cpu().numpy(), m3_64, m3_32)
    conf, m0, m1, s0, s1 = (t.cpu().numpy() for t in eng.score_match(dims, scale, 0.0))
    assert c64.max() > 0.9
    check_rel(f"conf {what}", conf, c64, c32)
    # matches: the float64 restatement's wherever its own arg-max is decided by more than what fp32 resolves
    tie = TIE_GAP["fp32"]
    rows_ok, cols_ok = R.top2_rel_gap(c64, 2) >= tie, R.top2_rel_gap(c64, 1) >= tie
    assert (~rows_ok).mean() <= 0.01 and (~cols_ok).mean() <= 0.01
    r0, r1 = R.mutual_matches(c64)
    np.testing.assert_array_equal(m0[rows_ok], r0[rows_ok])
    np.testing.assert_array_equal(m1[cols_ok], r1[cols_ok])
    # mscores: bitwise the conf entry the match points at, zero where the arg-max is not mutual (threshold 0)
    e0 = np.where(m0 >= 0, np.take_along_axis(conf, np.maximum(m0, 0)[:, :, None], axis=2)[:, :, 0], np.float32(0))
    e1 = np.where(m1 >= 0, np.take_along_axis(conf, np.maximum(m1, 0)[:, None, :], axis=1)[:, 0, :], np.float32(0))
    assert s0.dtype == np.float32 and np.array_equal(s0.view(np.uint32), e0.astype(np.float32).view(np.uint32))
    assert np.array_equal(s1.view(np.uint32), e1.astype(np.float32).view(np.uint32))
    assert (m0 >= 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# database cache against the plain forward where the windowed launches take another kernel form than the whole frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n2", [("fp32", 4000), ("bf16x6", 4000), ("fp16x4", 6000)])
def test_database_cache_at_form_edges(precision, n2):
    """prepare_database / forward(database=) run gnn.layers.1 and the projections of gnn.layers.2 on one-side windows, whose own
    tile count chooses the kernel form; the plain forward chooses by the whole frame's.  n1 = 100, n2 = 4000: the frame is 66
    tiles (fp32: register-diet qkv_kv / mlp0, Mlp3TileTallW8), the windows 2 and 64 (two-half loop, Mlp3TileS).  n2 = 6000,
    fp16x4: the frame is 96 tiles (128-column mlp0 tile), the 3D window 94 (64-column tile).  bf16x6 has one form per stage and
    must be bit-identical.  fp32 and fp16x4 are NOT (measured: max |d conf| 3.5e-8 and 1.1e-8 on conf entries up to 5e-3): the
    contract of include/gatsspg.h for this case is the one asserted -- the same matches, conf within the 2e-5 that
    test_hip_parity.py::test_trained_weights_database_cache_and_batch allows a re-associated launch."""
    n1 = 100
    assert R.launch_tiles(1, n1, n2) == {4000: 66, 6000: 96}[n2]
    m = build(synthetic.make_state_dict(8), precision)
    data = {k: dev(v) for k, v in synthetic.make_inputs(1, n1, n2, 8, seed=60).items()}
    plain = m.forward_batched(data)
    db = m.prepare_database(data)
    cached = m.forward_batched(data, database=db)
    bitwise = all(torch.equal(p, c) for p, c in zip(plain, cached))
    dconf = float((plain[0] - cached[0]).abs().max())
    print(f"\ndatabase cache at form edges [{precision}] n2={n2}: bitwise equal {bitwise}, max |d conf| {dconf:.3e}, "
          f"largest conf {float(plain[0].max()):.3e}, mutual matches {int((plain[1] >= 0).sum())}")
    assert torch.isfinite(cached[0]).all()
    if precision == "bf16x6":
        assert bitwise
    assert torch.equal(plain[1], cached[1]) and torch.equal(plain[2], cached[2]), "matches0 / matches1"
    assert dconf < 2e-5
