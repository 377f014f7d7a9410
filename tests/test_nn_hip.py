"""The HIP nearest-neighbour matcher against the fp64 oracle (tests/nn_oracle.py) under its comparison rule: tile edges, padding
masked by index, selection across tiles, exact ties, the ragged batch and the shared query plane from poisoned buffers, and the
reference-run goldens.  Small shapes around the 128 x 64 tile; every case is asserted to stay under the oracle's cap by the CPU
test tests/test_nn_oracle_golden.py::test_every_gpu_case_stays_under_the_cap."""
import json
import os

import numpy as np
import pytest
import torch

import nn_cases as nc
import nn_oracle as orc
from conftest import GOLDEN_DIR
from onepose_amd import NearestNeighbour

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(d0, d1, conf):
    """One pair through forward -> the four outputs as numpy [n0] / [n1]."""
    out = NearestNeighbour(conf)({"descriptors0": gpu(d0)[None], "descriptors1": gpu(d1)[None]})
    assert out["matches0"].dtype == torch.int64 and out["matches1"].dtype == torch.int64
    assert out["matching_scores0"].dtype == torch.float32 and out["matching_scores1"].dtype == torch.float32
    assert out["matches0"].shape == (1, d0.shape[1]) and out["matching_scores1"].shape == (1, d1.shape[1])
    return {k: v[0].cpu().numpy() for k, v in out.items()}


def check(d0, d1, conf, what):
    got = run(d0, d1, conf)
    left = orc.compare(got, orc.forward(d0, d1, conf), what)
    print(f"{what}: left out {left:.4f}")
    return got


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- 4. tile edges ----
@pytest.mark.parametrize("n1", nc.EDGE_N1)
@pytest.mark.parametrize("n0", nc.EDGE_N0)
def test_tile_edges(n0, n1):
    d0, d1 = nc.edge_pair(n0, n1)
    sim = NearestNeighbour().engine.similarity(gpu(d0), gpu(d1)).cpu().numpy()
    err = np.abs(sim - orc.similarity(d0, d1)).max()
    print(f"similarity {n0} x {n1}: max |err| vs fp64 {err:.3e} (2 gamma = {2 * orc.GAMMA:.3e})")
    assert sim.shape == (n0, n1) and err <= 2 * orc.GAMMA
    for c in nc.edge_confs(n0, n1):
        check(d0, d1, orc.CONFS[c], f"edge-{n0}x{n1}-{c}")


# ---- 5. padding is masked by index ----
@pytest.mark.parametrize("conf", sorted(nc.NEG_CONFS))
def test_padding_is_masked_by_index_when_every_similarity_is_negative(conf):
    d0, d1 = nc.negative_pair()
    got = check(d0, d1, nc.NEG_CONFS[conf], f"negative-{conf}")
    assert got["matches0"].max() < nc.NEG_N1 and got["matches1"].max() < nc.NEG_N0
    if conf in ("plain", "nomutual"):       # no test to fail: every column has its neighbour, with a score below 1/2
        assert (got["matches1"] >= 0).all() and (got["matching_scores1"] < 0.5).all() and (got["matching_scores1"] > 0).all()
    if conf == "nomutual":
        assert (got["matches0"] >= 0).all()


# ---- 6. selection across tiles ----
def test_selection_across_tiles():
    d0, d1 = nc.selection_pair()
    got = {c: check(d0, d1, conf, f"selection-{c}") for c, conf in nc.SEL_CONFS.items()}
    for r, a, _ in nc.SEL_ROWS:
        assert got["nomutual"]["matches0"][r] == a and got["plain"]["matches0"][r] == a and got["ratio"]["matches0"][r] == a
        assert got["tight"]["matches0"][r] == -1 and got["tight"]["matching_scores0"][r] == 0      # hinges on the true second
    for c, a, _ in nc.SEL_COLS:
        assert got["nomutual"]["matches1"][c] == a and got["ratio"]["matches1"][c] == a and got["tight"]["matches1"][c] == -1


# ---- 7. exact ties ----
def test_exact_ties_lowest_index_wins_and_the_second_equals_the_best():
    for side, rows, cols in (("rows", nc.TIE_ROWS, ()), ("cols", (), nc.TIE_COLS)):
        d0, d1 = nc.tie_pair(side)
        loose = check(d0, d1, {"do_mutual_check": False}, f"ties-{side}")
        mutual = check(d0, d1, {}, f"ties-{side}-mutual")
        strict = run(d0, d1, {"ratio_threshold": 0.99, "do_mutual_check": False})
        for r, a, b in rows:
            assert loose["matches0"][r] == min(a, b) and mutual["matches0"][r] == min(a, b)     # both duplicates point back at r
            assert loose["matches1"][a] == r and loose["matches1"][b] == r
            assert strict["matches0"][r] == -1 and strict["matching_scores0"][r] == 0           # second == best: ratio < 1 rejects
        for c, a, b in cols:
            assert loose["matches1"][c] == min(a, b)
            assert mutual["matches0"][min(a, b)] == c and mutual["matches0"][max(a, b)] == -1   # the column points at the lower row
            assert mutual["matching_scores0"][max(a, b)] > 0.9                                  # whose twin keeps its score
            assert strict["matches1"][c] == -1 and strict["matching_scores1"][c] == 0


# ---- 8. ragged ----
def poison(nn, b, cap0, cap1):
    """NaN workspace, -7 / NaN output buffers."""
    nn.engine.workspace(b, cap0, cap1, torch.device(DEV)).fill_(0xFF)
    return (torch.full((b, cap0), -7, device=DEV, dtype=torch.int64), torch.full((b, cap1), -7, device=DEV, dtype=torch.int64),
            torch.full((b, cap0), float("nan"), device=DEV), torch.full((b, cap1), float("nan"), device=DEV))


def padded(ds, cap, fill):
    out = torch.full((len(ds), orc.D, cap), fill, device=DEV, dtype=torch.float32)
    for i, d in enumerate(ds):
        out[i, :, :d.shape[1]] = gpu(d)
    return out


@pytest.mark.parametrize("poisoned", [False, True])
def test_ragged_items_are_bitwise_their_single_calls(poisoned):
    nn = NearestNeighbour(nc.RAGGED_CONF)
    pairs = [orc.make_pair(*item) for item in nc.RAGGED_ITEMS]
    n0, n1 = [p[0].shape[1] for p in pairs], [p[1].shape[1] for p in pairs]
    cap0, cap1 = max(n0), max(n1)
    fill = float("nan") if poisoned else 0.0       # what lies past an item's counts may hold anything
    out = poison(nn, len(pairs), cap0, cap1) if poisoned else None
    got = nn.engine.match_ragged(padded([p[0] for p in pairs], cap0, fill), padded([p[1] for p in pairs], cap1, fill), n0, n1, out=out)
    single = [nn({"descriptors0": gpu(p[0])[None], "descriptors1": gpu(p[1])[None]}) for p in pairs]
    for i, s in enumerate(single):
        for k, key in enumerate(orc.OUT_KEYS):
            n = n0[i] if key.endswith("0") else n1[i]
            assert same_bytes(got[k][i, :n], s[key][0]), (i, key)
            assert (got[k][i, n:] == (-1 if k < 2 else 0)).all(), (i, key)
        orc.compare({k: v[0].cpu().numpy() for k, v in s.items()}, orc.forward(*pairs[i], nc.RAGGED_CONF), f"ragged-{n0[i]}x{n1[i]}")
    # match_pairs is the same call behind the module's list contract
    res = nn.match_pairs([{"descriptors0": gpu(p[0])[None], "descriptors1": gpu(p[1])[None]} for p in pairs], max_items=2)
    assert all(same_bytes(r[key], s[key]) for r, s in zip(res, single) for key in orc.OUT_KEYS)


@pytest.mark.parametrize("poisoned", [False, True])
def test_shared_plane_is_bitwise_the_expanded_batch(poisoned):
    nn = NearestNeighbour(nc.RAGGED_CONF)
    views, q = nc.shared_items()
    n0, n1 = list(nc.SHARED_N0), [nc.SHARED_N1] * len(views)
    d0 = padded(views, max(n0), float("nan") if poisoned else 0.0)
    out = poison(nn, len(views), max(n0), nc.SHARED_N1) if poisoned else None
    shared = nn.engine.match_ragged(d0, gpu(q), n0, n1, out=out)
    expanded = nn.engine.match_ragged(d0, gpu(q)[None].expand(len(views), -1, -1), n0, n1)
    for k, key in enumerate(orc.OUT_KEYS):
        for i, v in enumerate(views):
            n = n0[i] if key.endswith("0") else n1[i]
            assert same_bytes(shared[k][i, :n], expanded[k][i, :n]), (i, key)
            assert (shared[k][i, n:] == (-1 if k < 2 else 0)).all()
    for i, v in enumerate(views):
        s = nn({"descriptors0": gpu(v)[None], "descriptors1": gpu(q)[None]})
        assert all(same_bytes(shared[k][i, :(n0[i] if key.endswith("0") else n1[i])], s[key][0]) for k, key in enumerate(orc.OUT_KEYS))
        orc.compare({k: x[0].cpu().numpy() for k, x in s.items()}, orc.forward(v, q, nc.RAGGED_CONF), f"shared-{n0[i]}")


def test_uniform_batch_and_preallocated_outputs():
    """A batch of pairs through forward is item by item the single call, also into out= buffers."""
    nn = NearestNeighbour({"ratio_threshold": 0.8})
    pairs = [orc.make_pair(70, 90, seed) for seed in (7, 8, 9)]
    d0, d1 = gpu(np.stack([p[0] for p in pairs])), gpu(np.stack([p[1] for p in pairs]))
    out = nn.engine.forward(d0, d1, out=poison(nn, 3, 70, 90))
    for i, p in enumerate(pairs):
        s = nn({"descriptors0": d0[i:i + 1], "descriptors1": d1[i:i + 1]})
        assert all(same_bytes(out[k][i], s[key][0]) for k, key in enumerate(orc.OUT_KEYS))


# ---- 9. the reference-run goldens ----
@pytest.mark.parametrize("name", ["tiny", "plain", "ratio", "distance", "both", "nomutual", "batch"])
def test_reference_goldens(name):
    g = np.load(os.path.join(GOLDEN_DIR, f"nn_{name}.npz"))
    conf = json.loads(str(g["conf"]))
    out = NearestNeighbour(conf)({"descriptors0": gpu(g["descriptors0"]), "descriptors1": gpu(g["descriptors1"])})
    for i in range(g["descriptors0"].shape[0]):
        ref = orc.forward(g["descriptors0"][i], g["descriptors1"][i], conf)
        orc.compare({k: out[k][i].cpu().numpy() for k in orc.OUT_KEYS}, ref, f"golden {name}[{i}] (module vs oracle)")
        # and against the recorded reference outputs themselves, on the entries the rule compares
        for side, dec in (("0", ref["decided0"]), ("1", ref["decided1"])):
            assert np.array_equal(out["matches" + side][i].cpu().numpy()[dec], g["matches" + side][i][dec])
            err = np.abs(out["matching_scores" + side][i].cpu().numpy().astype(np.float64) - g["matching_scores" + side][i])
            assert err[ref["score_decided0"] if side == "0" else dec].max() <= 2 * orc.GAMMA
