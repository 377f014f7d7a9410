"""numpy fp64 restatement of the reference NearestNeighbour matcher (src/models/matchers/nn/nearest_neighbour.py:5-63), the
test generator and the comparison rule of the nearest-neighbour tests.

Tie rule: on exactly equal similarities the lowest index wins (``np.argmax``); the second value is the second of the
multiset, so a duplicated maximum gives second == best (as ``topk(2)`` does).

Comparison rule.  GAMMA = 256 * 2^-24 bounds the error of any fp32 summation order of a 256-term dot product of unit
vectors (sum |a_i b_i| <= 1 by Cauchy-Schwarz), the reference's and the kernel's alike.  A row or column is DECIDED when, in
fp64, its top-2 gap exceeds 4 GAMMA and every threshold inequality the configuration evaluates is farther than 8 GAMMA from
equality.  On decided rows and columns indices and masks must be equal and scores agree within 2 GAMMA; an undecided one is
left out of the index comparison.  With the mutual check, matches0[i] is a function of row i AND of the column j it points
at: it is compared when both are decided, or when row i is more than 4 GAMMA below column j's best (the column cannot point
back then, whatever it decides).  At most CAP = 2 % of rows plus columns may be left out per case.
"""
import numpy as np

D = 256
GAMMA = D * 2.0 ** -24
CAP = 0.02
OUT_KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1")
DEFAULT_CONF = {"match_threshold": None, "ratio_threshold": None, "distance_threshold": None, "do_mutual_check": True}
CONFS = {"plain": {}, "ratio": {"ratio_threshold": 0.8}, "distance": {"distance_threshold": 0.7},
         "both": {"ratio_threshold": 0.9, "distance_threshold": 0.9}}


def unit(x):
    return x / np.linalg.norm(x, axis=0, keepdims=True)


def make_pair(n0, n1, seed, planted=0.7):
    """Random unit descriptors [256,n0], [256,n1] (fp32) with planted pairs: a fraction ``planted`` of the smaller side reappears
    on the other side with per-pair noise spread from 0.05 to 1.0, in units of 1/16 per channel (noise 1.0 has the norm of the
    descriptor: similarity about 0.7)."""
    rng = np.random.default_rng(seed)
    d0 = unit(rng.standard_normal((D, n0)))
    d1 = unit(rng.standard_normal((D, n1)))
    k = max(1, int(planted * min(n0, n1)))
    src, dst = rng.permutation(n0)[:k], rng.permutation(n1)[:k]
    noise = np.linspace(0.05, 1.0, k) / 16.0
    d1[:, dst] = unit(d0[:, src] + noise * rng.standard_normal((D, k)))
    return d0.astype(np.float32), d1.astype(np.float32)


def similarity(d0, d1):
    """[256,n0], [256,n1] -> [n0,n1] in fp64."""
    return d0.astype(np.float64).T @ d1.astype(np.float64)


def find_nn(sim, ratio, distance):
    """find_nn (:5-15) on the rows of ``sim`` -> (matches, scores, decided)."""
    n, m = sim.shape
    rows = np.arange(n)
    idx = np.argmax(sim, axis=1)
    best = sim[rows, idx]
    if m >= 2:
        rest = sim.copy()
        rest[rows, idx] = -np.inf
        second = rest.max(axis=1)
    else:
        if ratio:
            raise ValueError("the ratio test needs a second neighbour")
        second = np.full(n, -np.inf)
    dist0, dist1 = 2 * (1 - best), 2 * (1 - second)
    mask = np.ones(n, dtype=bool)
    decided = (best - second) > 4 * GAMMA
    if ratio:
        mask &= dist0 <= ratio ** 2 * dist1
        decided &= np.abs(dist0 - ratio ** 2 * dist1) > 8 * GAMMA
    if distance:
        mask &= dist0 <= distance ** 2
        decided &= np.abs(dist0 - distance ** 2) > 8 * GAMMA
    return np.where(mask, idx, -1).astype(np.int64), np.where(mask, (best + 1) / 2, 0.0), decided


def forward(d0, d1, conf=None):
    """One pair: d0 [256,n0], d1 [256,n1] -> the four outputs (matches int64, scores fp64), ``decided0`` / ``decided1`` (with the
    mutual check decided0 also asks for the column a row points at) and ``left_out``, the share of rows plus columns that are
    not decided."""
    conf = {**DEFAULT_CONF, **(conf or {})}
    sim = similarity(d0, d1)
    m0, s0, dec0 = find_nn(sim, conf["ratio_threshold"], conf["distance_threshold"])
    m1, s1, dec1 = find_nn(sim.T, conf["ratio_threshold"], conf["distance_threshold"])
    score_dec0 = dec0
    if conf["do_mutual_check"]:         # mutual_check (:18-23): matches0 only
        ptr = np.where(m0 > -1, m0, 0)
        # the column a row points at decides with it -- unless the row is more than 4 GAMMA below that column's best: then the
        # column cannot point back whatever it decides, and the row is dropped either way
        contender = sim[np.arange(len(m0)), ptr] >= sim[:, ptr].max(axis=0) - 4 * GAMMA
        dec0 = dec0 & ~((m0 > -1) & ~dec1[ptr] & contender)
        m0 = np.where((m0 > -1) & (m1[ptr] == np.arange(len(m0))), m0, -1)
    left = (np.count_nonzero(~dec0) + np.count_nonzero(~dec1)) / (len(dec0) + len(dec1))
    return {"matches0": m0, "matches1": m1, "matching_scores0": s0, "matching_scores1": s1, "decided0": dec0, "decided1": dec1,
            "score_decided0": score_dec0, "left_out": left}


def compare(got, ref, what=""):
    """``got``: the four outputs of one pair as arrays [n0] / [n1] (the module's, or the reference's); ``ref``: ``forward`` of the same
    pair.  Asserts the comparison rule and returns the share left out."""
    assert ref["left_out"] <= CAP, f"{what}: {ref['left_out']:.4f} of rows + columns undecided, cap {CAP}"
    for side, dec, sdec in (("0", ref["decided0"], ref["score_decided0"]), ("1", ref["decided1"], ref["decided1"])):
        m, s = np.asarray(got["matches" + side]), np.asarray(got["matching_scores" + side], dtype=np.float64)
        rm, rs = ref["matches" + side], ref["matching_scores" + side]
        assert m.shape == rm.shape and s.shape == rs.shape, f"{what}: shapes of side {side}"
        bad = np.flatnonzero(dec & (m != rm))
        assert bad.size == 0, f"{what}: matches{side} differs on decided entries {bad[:8]}: got {m[bad[:8]]}, oracle {rm[bad[:8]]}"
        err = np.abs(s - rs)[sdec]
        assert err.size == 0 or err.max() <= 2 * GAMMA, f"{what}: matching_scores{side} off by {err.max():.3e} > 2 gamma"
        n_other = len(ref["matches" + ("1" if side == "0" else "0")])
        assert ((m >= -1) & (m < n_other)).all(), f"{what}: matches{side} out of range"
    return ref["left_out"]
