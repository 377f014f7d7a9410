"""The cases of the nearest-neighbour GPU tests (tests/test_nn_hip.py), built from seeds on the host: shared with the CPU test
that asserts, for every one of them, that the comparison rule of nn_oracle leaves out no more than its cap."""
import numpy as np

import nn_oracle as orc
from nn_oracle import D, unit

BM, BN = 128, 64                      # NNM_TILE_ROWS x NNM_TILE_COLS (onepose_amd._native_sg.NNM_TILE; asserted by the ABI test)
EDGE_N0 = (1, 2, BM - 1, BM, BM + 1, 2 * BM + 3)
EDGE_N1 = (2, BN - 1, BN, BN + 1, 3 * BN + 5)


def edge_confs(n0, n1):
    """The configurations a tile-edge shape runs: the ratio test needs two points on both sides."""
    return ["plain", "distance"] + (["ratio", "both"] if min(n0, n1) >= 2 else [])


def edge_pair(n0, n1):
    return orc.make_pair(n0, n1, seed=1000 + 7 * n0 + n1)


# ---- padding is masked by index: every real similarity is negative, n no tile multiple ----
NEG_N0, NEG_N1 = 100, 75
NEG_CONFS = {"plain": {}, "ratio": {"ratio_threshold": 0.999}, "distance": {"distance_threshold": 1.9},
             "nomutual": {"do_mutual_check": False}}


def negative_pair():
    """descriptors1 = -(descriptors0 permuted, plus noise), all around one common direction: every similarity is below -0.4, so the
    0 of a padded column or row would beat them all."""
    rng = np.random.default_rng(77)
    c = unit(rng.standard_normal((D, 1)))
    u = unit(rng.standard_normal((D, NEG_N0)))
    d0 = unit(c + 0.7 * u)
    perm = rng.permutation(NEG_N0)[:NEG_N1]
    d1 = -unit(c + 0.7 * u[:, perm] + 0.1 * unit(rng.standard_normal((D, NEG_N1))))
    return d0.astype(np.float32), d1.astype(np.float32)


# ---- selection across tiles: (row, column of its best, column of its second) and the same for columns ----
SEL_N0, SEL_N1 = 2 * BM + 3, 3 * BN + 5
SEL_ROWS = [(0, 3, 40),                     # best and second in the same tile
            (1, 5, SEL_N1 - 2),             # best in the first column tile, second in the last
            (2, SEL_N1 - 3, 7),             # the reverse
            (3, SEL_N1 - 1, BN + 1)]        # the best sits in the last valid column before the padding
SEL_COLS = [(100, 10, 90),                  # (column, row of its best, row of its second): one row tile
            (101, 12, SEL_N0 - 2),          # first and last row tile
            (102, SEL_N0 - 1, 130)]         # the last valid row, second in the middle tile
SEL_CONFS = {"plain": {}, "ratio": {"ratio_threshold": 0.8}, "tight": {"ratio_threshold": 0.22}, "nomutual": {"do_mutual_check": False}}


def _near(rng, v, noise):
    return unit(v + noise * unit(rng.standard_normal((D, 1))))[:, 0]


def selection_pair():
    """Random unit descriptors with planted best (noise 0.1: similarity 0.995) and second (noise 0.3: 0.958) neighbours.  The
    ratio test at 0.22 (ratio^2 = 0.048 < dist0 / dist1 = 0.12) rejects with the true second and would accept with any other
    column's similarity in its place; at 0.8 it accepts."""
    rng = np.random.default_rng(78)
    d0 = unit(rng.standard_normal((D, SEL_N0)))
    d1 = unit(rng.standard_normal((D, SEL_N1)))
    for r, a, b in SEL_ROWS:
        d1[:, a], d1[:, b] = _near(rng, d0[:, r:r + 1], 0.1), _near(rng, d0[:, r:r + 1], 0.3)
    for c, a, b in SEL_COLS:
        d0[:, a], d0[:, b] = _near(rng, d1[:, c:c + 1], 0.1), _near(rng, d1[:, c:c + 1], 0.3)
    return d0.astype(np.float32), d1.astype(np.float32)


# ---- exact ties: duplicated columns (rows) are bitwise equal similarities ----
TIE_ROWS = [(0, 5, 2 * BN + 9),             # (row, the duplicated best columns): in different tiles
            (1, BN + 2, BN + 40)]           # in one tile
TIE_COLS = [(150, 20, BM + 30)]             # (column, the duplicated best rows): in different row tiles


def tie_pair(side):
    """side "rows": duplicated columns of descriptors1 (TIE_ROWS); "cols": duplicated rows of descriptors0 (TIE_COLS).  Two cases,
    because a duplicated descriptor is also the tied best of whichever other points happen to prefer it."""
    rng = np.random.default_rng(79)
    d0 = unit(rng.standard_normal((D, SEL_N0)))
    d1 = unit(rng.standard_normal((D, SEL_N1)))
    if side == "rows":
        for r, a, b in TIE_ROWS:
            d1[:, a] = _near(rng, d0[:, r:r + 1], 0.2)
            d1[:, b] = d1[:, a]
    else:
        for c, a, b in TIE_COLS:
            d0[:, a] = _near(rng, d1[:, c:c + 1], 0.2)
            d0[:, b] = d0[:, a]
    return d0.astype(np.float32), d1.astype(np.float32)


# ---- ragged: (n0, n1, seed) per item; the shared-plane call gives every item the n1 of the first ----
RAGGED_ITEMS = [(2, 2, 31), (BM + 1, 3 * BN + 5, 32), (200, 70, 33)]
RAGGED_CONF = {"ratio_threshold": 0.8, "distance_threshold": 0.7}
SHARED_N0 = (2, BM + 1, 200)
SHARED_N1 = 3 * BN + 5


def shared_items():
    """Three views of their own sizes against ONE query plane: (d0 list, d1)."""
    d1 = orc.make_pair(SHARED_N0[-1], SHARED_N1, seed=40)[1]
    rng = np.random.default_rng(41)
    views = []
    for n in SHARED_N0:
        v = unit(rng.standard_normal((D, n)))
        k = max(1, n // 2)
        src, noise = rng.permutation(SHARED_N1)[:k], np.linspace(0.05, 1.0, k) / 16.0
        v[:, :k] = unit(d1[:, src] + noise * rng.standard_normal((D, k)))
        views.append(v.astype(np.float32))
    return views, d1


def all_cases():
    """(name, d0, d1, conf) of every pair a GPU test compares with the oracle under the comparison rule."""
    for n0 in EDGE_N0:
        for n1 in EDGE_N1:
            d0, d1 = edge_pair(n0, n1)
            for c in edge_confs(n0, n1):
                yield f"edge-{n0}x{n1}-{c}", d0, d1, orc.CONFS[c]
    d0, d1 = negative_pair()
    for c, conf in NEG_CONFS.items():
        yield f"negative-{c}", d0, d1, conf
    d0, d1 = selection_pair()
    for c, conf in SEL_CONFS.items():
        yield f"selection-{c}", d0, d1, conf
    for side in ("rows", "cols"):
        yield f"ties-{side}", *tie_pair(side), {}
    for n0, n1, seed in RAGGED_ITEMS:
        yield f"ragged-{n0}x{n1}", *orc.make_pair(n0, n1, seed), RAGGED_CONF
    views, q = shared_items()
    for v in views:
        yield f"shared-{v.shape[1]}", v, q, RAGGED_CONF
