"""Seeded cases of the extractor head's edge tests (tests/test_spp_detect_edges.py): constructed score maps and dense descriptors, the
oracle's result on them (oracle/superpoint_oracle.py: simple_nms, select_keypoints, sample_descriptors) and the conditions under which a
case reaches the path of spp_detect_kernels.hip it is meant for.  A condition is a (name, bool) pair that the oracle alone decides; where
it depends on a seed, sub-seeds are tried in turn until every condition of the case holds -- the search is deterministic and no case is
ever dropped or filtered by a test.  tests/test_spp_cases.py asserts the conditions of every case the GPU tests use.

Every discrete output (NMS map, counts, keypoints with their order, scores) is compared by equality; only the descriptors carry a bound
(sample_reference below: the fp64 restatement that bound is taken against).

Geometry of the kernels the cases aim at (spp_detect_kernels.hip):
  nms_kernel      a T x T output tile inside a 64 x 64 region, T = min(32, 64 - 10 R): 32, 32, 32, 24, 14, 4 for R = 1 .. 6; halo 5 R
  rowscan_kernel  1024 threads, ceil(H / 1024) consecutive rows each
  select_kernel   radix digits of 12 + 12 + 8 bits; ordered compaction in chunks of 1024 candidates
  rank_kernel     a 64 x 16 grid of 256 x 256 blocks: a second trip over j above 4096 survivors, over i above 16384
  sample_kernel   16 keypoints per workgroup
"""
import functools

import numpy as np

from oracle import superpoint_oracle as so

F32 = np.float32
NMS_E = 64


def tile(radius):
    return min(32, NMS_E - 10 * radius)


def config(radius, threshold, border, max_kp):
    return {"descriptor_dim": 256, "nms_radius": radius, "keypoint_threshold": threshold, "remove_borders": border, "max_keypoints": max_kp}


def oracle_detect(score, radius, threshold, border, max_kp):
    """The oracle on a batch [b, H, W] -> (nms [b, H, W], [yx int64 [n, 2]], [scores [n]], candidates per image before the top-k)."""
    nms = np.stack([so.simple_nms(s, radius) for s in score])
    sel = [so.select_keypoints(m, threshold, border, max_kp) for m in nms]
    ncand = [len(so.select_keypoints(m, threshold, border, -1)[1]) for m in nms]
    return nms, [s[0] for s in sel], [s[1] for s in sel], ncand


def detect_case(score, radius, threshold, border, max_kp, conditions, **more):
    score = np.ascontiguousarray(score, F32)
    nms, yx, sc, ncand = oracle_detect(score, radius, threshold, border, max_kp)
    return dict(score=score, cfg=config(radius, threshold, border, max_kp), nms=nms, yx=yx, sc=sc, ncand=ncand, conditions=list(conditions), **more)


@functools.lru_cache(maxsize=None)
def dense_normal(b, hc, wc, seed=0):
    """Standard-normal dense descriptors [b, 256, hc, wc] for the cases whose subject is not the sampler."""
    return np.random.RandomState(7000 + seed).standard_normal((b, 256, hc, wc)).astype(F32)


# ---- A.1  chains of peaks: a pixel's fate depends on a pixel 5 R away -----------------------------------------------------------------
CHAIN_H, CHAIN_W = 72, 104
CHAIN_PEAKS = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2], F32)
CHAIN_FAMILIES = {"row": (0, 1), "col": (1, 0), "diag": (1, 1)}       # step of the chain in (y, x), times R
CHAIN_BATCH = 8
RADII = [1, 2, 3, 4, 5, 6]


def chain_start(radius, k, length):
    """A start coordinate with start = -k mod T (peak 0 exactly k pixels before a tile boundary) whose chain of 8 peaks fits in `length`;
    odd k take the second boundary where the chain still fits, so not every peak 0 sits in the first tile."""
    t, span = tile(radius), 7 * radius
    start = -(-k // t) * t - k
    if k % 2 == 1 and start + t + span < length:
        start += t
    assert 0 <= start and start + span < length and (start + k) % t == 0
    return start


def chain_specs(radius):
    """[(family, y0, x0)]: for each family every k in 1 .. 5 R on the axis (both axes for the diagonal) the chain runs along, plus one
    chain that starts on coordinate 0 and one that ends on the last row / column."""
    span = 7 * radius
    specs = []
    for k in range(1, 5 * radius + 1):
        cross_y, cross_x = (7 * k + 3 * radius) % CHAIN_H, (11 * k + 5 * radius) % CHAIN_W
        specs.append(("row", cross_y, chain_start(radius, k, CHAIN_W)))
        specs.append(("col", chain_start(radius, k, CHAIN_H), cross_x))
        specs.append(("diag", chain_start(radius, k, CHAIN_H), chain_start(radius, k, CHAIN_W)))
    specs += [("row", 0, 0), ("row", CHAIN_H - 1, CHAIN_W - 1 - span), ("col", 0, 0), ("col", CHAIN_H - 1 - span, CHAIN_W - 1),
              ("diag", 0, 0), ("diag", CHAIN_H - 1 - span, CHAIN_W - 1 - span)]
    return specs


def chain_points(family, radius, y0, x0):
    dy, dx = CHAIN_FAMILIES[family]
    return [(y0 + i * dy * radius, x0 + i * dx * radius) for i in range(len(CHAIN_PEAKS))]


@functools.lru_cache(maxsize=None)
def chain_case(radius):
    """Every chain of chain_specs(radius) and its twin without peak 0: maps [n, 72, 104] (a chain at 2 j, its twin at 2 j + 1).
    -> detect_case fields + specs, points, kept [n]: the set of peak numbers the oracle keeps in each map."""
    specs = chain_specs(radius)
    maps, points = [], []
    for family, y0, x0 in specs:
        pts = chain_points(family, radius, y0, x0)
        for twin in (False, True):
            m = np.zeros((CHAIN_H, CHAIN_W), F32)
            for i, (y, x) in enumerate(pts):
                if not (twin and i == 0):
                    m[y, x] = CHAIN_PEAKS[i]
            maps.append(m)
            points.append(pts)
    c = detect_case(np.stack(maps), radius, 0.05, 0, -1, [], specs=specs, points=points)
    kept = []
    for m, pts in zip(c["nms"], points):
        on = {i for i, (y, x) in enumerate(pts) if m[y, x] != 0}
        assert int((m != 0).sum()) == len(on)                       # nothing but peaks survives
        kept.append(on)
    c["kept"] = kept
    t = tile(radius)
    cond = [("full chains keep peaks 0, 2, 4", all(k == {0, 2, 4} for k in kept[0::2])),
            ("twins keep peaks 1, 3, 5", all(k == {1, 3, 5} for k in kept[1::2]))]
    for axis, name in ((0, "y"), (1, "x")):
        along = [p[0][axis] for s, p in zip(specs, points[0::2]) if CHAIN_FAMILIES[s[0]][axis]]
        last = [p[-1][axis] for s, p in zip(specs, points[0::2]) if CHAIN_FAMILIES[s[0]][axis]]
        cond.append((f"{name}: peak 0 at every k in 1 .. 5 R before a tile boundary", all(any((a + k) % t == 0 for a in along) for k in range(1, 5 * radius + 1))))
        cond.append((f"{name}: a chain starts on coordinate 0", 0 in along))
        cond.append((f"{name}: a chain ends on the last coordinate", (CHAIN_H, CHAIN_W)[axis] - 1 in last))
    c["conditions"] = cond
    return c


# ---- A.2  quantised random maps: equal floats everywhere ------------------------------------------------------------------------------
QUANT_LEVELS = [16, 256]
QUANT_SHAPES = [(72, 104), (88, 80)]


def nms_trace(scores, radius):
    """simple_nms restated with the number of pixels each suppression round adds to the mask -> (nms, [added in round 1, in round 2])."""
    zeros = np.zeros_like(scores)
    max_mask = scores == so._max_pool_same(scores, radius)
    added = []
    for _ in range(2):
        supp_mask = so._max_pool_same(max_mask.astype(F32), radius) > 0
        supp_scores = np.where(supp_mask, zeros, scores)
        new_max_mask = supp_scores == so._max_pool_same(supp_scores, radius)
        grown = max_mask | (new_max_mask & (~supp_mask))
        added.append(int(grown.sum() - max_mask.sum()))
        max_mask = grown
    return np.where(max_mask, scores, zeros), added


def near_tile_edges(nms, radius):
    """Survivors within R of a tile boundary, on each side of it, on both axes -> four bools (y before, y after, x before, x after)."""
    t = tile(radius)
    ys, xs = np.nonzero(nms)
    r = min(radius, t)
    return [bool((ys % t >= t - r).any()), bool((ys % t < r).any()), bool((xs % t >= t - r).any()), bool((xs % t < r).any())]


def has_plateau(nms):
    on = nms != 0
    return bool((on[:, 1:] & on[:, :-1] & (nms[:, 1:] == nms[:, :-1])).any() or (on[1:] & on[:-1] & (nms[1:] == nms[:-1])).any())


@functools.lru_cache(maxsize=None)
def quant_case(levels, shape, radius, seed=0, tries=200):
    """Two maps of randint(1, L + 1) / (L + 1).  L = 256: both suppression rounds add to the mask, in each image; L = 16: two adjacent
    equal survivors (a plateau) in each image; both: survivors within R of a tile boundary, on either side, on both axes, in each image."""
    h, w = shape
    for sub in range(tries):
        rs = np.random.RandomState(100000 * seed + 1000 * sub + 10 * radius + (levels == 256))
        score = (rs.randint(1, levels + 1, (2, h, w)) / (levels + 1)).astype(F32)
        cond = []
        for i, s in enumerate(score):
            nms, added = nms_trace(s, radius)
            assert np.array_equal(nms, so.simple_nms(s, radius))
            if levels == 256:
                cond.append((f"image {i}: both suppression rounds add to the mask", added[0] > 0 and added[1] > 0))
            else:
                cond.append((f"image {i}: a plateau of adjacent equal survivors", has_plateau(nms)))
            cond.append((f"image {i}: survivors within R of a tile boundary on both axes, both sides", all(near_tile_edges(nms, radius))))
        if all(ok for _, ok in cond):
            return detect_case(score, radius, 0.5, 0, -1, cond, sub=sub)
    raise AssertionError(f"no sub-seed gives a quantised map (L = {levels}, {h} x {w}, R = {radius}) that meets the conditions")


@functools.lru_cache(maxsize=None)
def radius0_case():
    """R = 0: the NMS map is the input, bit for bit -- arbitrary non-negative patterns, zeros, subnormals and the largest normal included."""
    rs = np.random.RandomState(11)
    bits = rs.randint(0, 0x7F800000, (3, 40, 72)).astype(np.uint32)
    bits[0, 0, :4] = [0, 1, 0x007FFFFF, 0x7F7FFFFF]
    score = bits.view(F32)
    cond = [("non-negative and finite", bool(np.isfinite(score).all() and (score >= 0).all())), ("a subnormal is present", bool(((bits > 0) & (bits < 0x00800000)).any()))]
    return detect_case(score, 0, 0.5, 0, -1, cond)


# ---- B  threshold, border, row scan, compaction ---------------------------------------------------------------------------------------
SCAN_SHAPES = [(1032, 8), (2056, 8), (8, 1032)]
SCAN_BORDERS = [0, 3]
SCAN_THRESHOLD = 0.25
SCAN_LEVELS = np.array([0.125, 0.25, 0.375, 0.5], F32)


@functools.lru_cache(maxsize=None)
def scan_case(shape, border, seed=0, tries=50):
    """R = 2, keep-all, b = 2, a sparse map of four levels of which one IS the threshold (kept only if strictly above).  Tall maps:
    rowscan_kernel gives a thread ceil(H / 1024) = 2 or 3 consecutive rows (two planted plateaus of the top level fill all the rows of one
    thread each: survivors within R of each other exist only on a plateau).  The wide map: rowcount / compact walk 17 chunks of 64."""
    h, w = shape
    per = (h + 1023) // 1024
    for sub in range(tries):
        rs = np.random.RandomState(1000 * seed + sub + h + 3 * border)
        score = np.where(rs.uniform(size=(2, h, w)) < 0.15, SCAN_LEVELS[rs.randint(0, 4, (2, h, w))], F32(0)).astype(F32)
        if h > 1024:                              # plateaus of the top level over all the rows of one thread, inside the border too
            for y in (per * 100, per * ((h - 8) // per)):
                score[:, y:y + per, 3:5] = SCAN_LEVELS[-1]
        c = detect_case(score, 2, SCAN_THRESHOLD, border, -1, [])
        cond = []
        for i, (nms, yx) in enumerate(zip(c["nms"], c["yx"])):
            inner = nms[border:h - border, border:w - border]
            cond.append((f"image {i}: a surviving value equals the threshold", bool((inner == F32(SCAN_THRESHOLD)).any())))
            cond.append((f"image {i}: no kept score equals the threshold", bool((c["sc"][i] > F32(SCAN_THRESHOLD)).all())))
            rows = np.bincount(yx[:, 0], minlength=h)
            if h > 1024:
                first = int(np.nonzero(rows[1024:])[0][0]) + 1024 if rows[1024:].any() else -1
                cond.append((f"image {i}: candidates in rows >= 1024", first >= 0))
                cond.append((f"image {i}: the first such row has a non-zero offset", first >= 0 and int(rows[:first].sum()) > 0))
                # the offset of a thread's second (third) row is its first row's plus what that row holds: used only if both have candidates
                later = [y for y in range(h) if y % per and rows[y] and rows[y - y % per:y].any()]
                cond.append((f"image {i}: a thread's later row and an earlier row of the same thread both hold candidates", len(later) > 0))
                cond.append((f"image {i}: such a pair at or above row 1024", any(y >= 1024 for y in later)))
            else:
                chunks = [np.unique(yx[yx[:, 0] == y, 1] // 64) for y in range(h)]
                cond.append((f"image {i}: a row with candidates in several 64-pixel chunks, the last (partial) one included",
                             any(len(u) > 1 and u[-1] == (w - 1) // 64 for u in chunks)))
        if all(ok for _, ok in cond):
            c["conditions"], c["sub"] = cond, sub
            c["capacity"] = max(c["ncand"]) + 7
            return c
    raise AssertionError(f"no sub-seed gives a row-scan case of {h} x {w}, border {border}")


@functools.lru_cache(maxsize=None)
def border_case(border):
    """remove_borders >= H / 2: nothing is left, counts [0, 0] (16 x 24, b = 2, every pixel a candidate otherwise)."""
    score = (np.random.RandomState(5).randint(1, 17, (2, 16, 24)) / 17).astype(F32)
    c = detect_case(score, 0, 0.0, border, -1, [])
    c["conditions"] = [("border >= H / 2", border >= 8), ("every pixel is above the threshold", bool((score > 0).all())), ("the oracle keeps nothing", c["ncand"] == [0, 0])]
    return c


TRUNC_CAPACITY = 40


@functools.lru_cache(maxsize=None)
def truncation_case():
    """Keep-all, b = 2, capacity 40: image 0 fits, image 1 overflows -- counts [n0, n0] and [40, n1], image 1's first 40 in row-major order."""
    rs = np.random.RandomState(3)
    score = rs.uniform(0.1, 1.0, (2, 24, 32)).astype(F32)
    score[0][rs.uniform(size=(24, 32)) < 0.96] = 0
    c = detect_case(score, 1, 0.05, 0, -1, [])
    n0, n1 = c["ncand"]
    c["conditions"] = [("image 0 fits", 0 < n0 <= TRUNC_CAPACITY), ("image 1 overflows", n1 > TRUNC_CAPACITY)]
    return c


# ---- C  top-k: radix select, ordered compaction, rank, scatter ------------------------------------------------------------------------
TOPK_K = [1, 255, 1024, 1025, 3000, 4095]
TOPK_KINDS = ["low", "mid", "top"]


@functools.lru_cache(maxsize=None)
def topk_scores(kind):
    """64 x 64 positive normal fp32 scores, from bit patterns: R = 0, threshold 0, border 0 make the map the candidate table itself.
      low  0x3C000000 + randint(0, 256): only the last radix digit differs, sixteen candidates per value on average
      mid  0x3C000000 + (randint(0, 4096) << 8) + 0x55: only the middle digit differs
      top  log-uniform in [1e-30, 1]: the first digit decides"""
    rs = np.random.RandomState(0)
    if kind == "low":
        bits = (0x3C000000 + rs.randint(0, 256, (64, 64))).astype(np.uint32)
    elif kind == "mid":
        bits = (0x3C000000 + (rs.randint(0, 4096, (64, 64)) << 8) + 0x55).astype(np.uint32)
    else:
        bits = (10.0 ** rs.uniform(-30, 0, (64, 64))).astype(F32).view(np.uint32)
    return np.ascontiguousarray(bits).view(F32)[None]


def cut_counts(scores, k):
    """(candidates equal to the k-th largest score, how many of them are kept)."""
    s = np.sort(scores.ravel())[::-1]
    cut = s[k - 1]
    return int((s == cut).sum()), k - int((s > cut).sum())


@functools.lru_cache(maxsize=None)
def topk_case(kind, k):
    score = topk_scores(kind)
    bits = score.view(np.uint32).ravel()
    ties, kept = cut_counts(score, k)
    cond = [("positive and normal", bool((bits >= 0x00800000).all() and (bits < 0x7F800000).all())), ("more candidates than k", bits.size > k)]
    if kind == "low":
        cond += [("one top and one middle digit", len(np.unique(bits >> 8)) == 1), ("more candidates equal the cut score than are kept, at least one is kept", ties > kept >= 1)]
    elif kind == "mid":
        cond += [("one top digit, one low digit", len(np.unique(bits >> 20)) == 1 and len(np.unique(bits & 0xFF)) == 1),
                 ("more than 2000 middle digits", len(np.unique((bits >> 8) & 0xFFF)) > 2000)]
    else:
        cond += [("more than 500 top digits", len(np.unique(bits >> 20)) > 500)]
    return detect_case(score, 0, 0.0, 0, k, cond, ties=ties, kept=kept)


ALL_EQUAL_K = [1500, 4095]


@functools.lru_cache(maxsize=None)
def all_equal_case(k):
    """4096 scores of 0.25: the survivors are the first k pixels in row-major order, the quota (k) spans the 1024-candidate chunks."""
    c = detect_case(np.full((1, 64, 64), 0.25, F32), 0, 0.0, 0, k, [])
    first_k = np.stack(np.divmod(np.arange(k), 64), axis=1)
    c["conditions"] = [("the oracle keeps the first k pixels in row-major order", np.array_equal(c["yx"][0], first_k))]
    return c


QUOTA_KINDS = ["across_chunks", "all_ties"]


@functools.lru_cache(maxsize=None)
def quota_case(kind):
    """100 pixels of 0.5 planted in a 64 x 64 map.  across_chunks: 0.25 everywhere else, k = 1600 -- the cut score is 0.25 with a quota of
    1500 of its 3996 candidates.  all_ties: 0.25 and 0.125 elsewhere, k = 100 + #(0.25) -- the quota equals the number of ties."""
    rs = np.random.RandomState(21)
    score = np.full(4096, 0.25, F32)
    if kind == "all_ties":
        score[rs.uniform(size=4096) < 0.5] = 0.125
    score[rs.choice(4096, 100, replace=False)] = 0.5
    k = 1600 if kind == "across_chunks" else 100 + int((score == 0.25).sum())
    score = score.reshape(1, 64, 64)
    ties, quota = cut_counts(score, k)
    cond = [("100 scores above the cut", int((score == 0.5).sum()) == 100 and k - quota == 100), ("more candidates than k", k < 4096)]
    if kind == "across_chunks":
        cond += [("quota above 1024 and no multiple of it", quota > 1024 and quota % 1024 != 0), ("fewer kept than tied", quota < ties)]
        flat = score.ravel()
        last_kept = np.nonzero(flat == 0.25)[0][quota - 1]
        cond += [("scores above the cut follow the last kept tie, in its chunk and in later ones",
                  bool((flat[last_kept + 1:(last_kept // 1024 + 1) * 1024] == 0.5).any() and (flat[(last_kept // 1024 + 1) * 1024:] == 0.5).any()))]
    else:
        cond += [("the quota equals the number of ties", quota == ties), ("ties in every chunk of 1024", all((score.ravel()[j:j + 1024] == 0.25).any() for j in range(0, 4096, 1024)))]
    return detect_case(score, 0, 0.0, 0, k, cond, quota=quota, ties=ties)


MIXED_K = 50
MIXED_CAPACITIES = [50, 80]


@functools.lru_cache(maxsize=None)
def mixed_batch_case():
    """b = 3, k = 50: no candidates; exactly k (row-major order, unsorted); k + 1 (sorted, the lowest dropped)."""
    rs = np.random.RandomState(8)
    score = np.zeros((3, 24 * 32), F32)
    for i, n in ((1, MIXED_K), (2, MIXED_K + 1)):
        score[i, rs.choice(24 * 32, n, replace=False)] = rs.permutation(np.arange(1, n + 1) / F32(64)).astype(F32)
    c = detect_case(score.reshape(3, 24, 32), 0, 0.0, 0, MIXED_K, [])
    c["conditions"] = [("candidates 0, k, k + 1", c["ncand"] == [0, MIXED_K, MIXED_K + 1]), ("kept 0, k, k", [len(s) for s in c["sc"]] == [0, MIXED_K, MIXED_K]),
                       ("image 1 is in row-major order and not sorted", bool((np.diff(c["yx"][1][:, 0] * 32 + c["yx"][1][:, 1]) > 0).all() and (np.diff(c["sc"][1]) > 0).any())),
                       ("image 2 is sorted and not in row-major order", bool((np.diff(c["sc"][2]) < 0).all() and (np.diff(c["yx"][2][:, 0] * 32 + c["yx"][2][:, 1]) < 0).any())),
                       ("image 2 drops its lowest score", float(c["sc"][2].min()) > float(score[2][score[2] > 0].min()))]
    return c


LARGE_K = [4097, 16385, 20000]


@functools.lru_cache(maxsize=None)
def large_scores():
    return (np.random.RandomState(4).randint(1, 16384, (1, 256, 256)) / 16384).astype(F32)


@functools.lru_cache(maxsize=None)
def large_case(k):
    """256 x 256, values randint(1, 16384) / 16384 (four candidates per value on average), capacity k: the second trips of rank_kernel."""
    score = large_scores()
    c = detect_case(score, 0, 0.0, 0, k, [])
    yx, sc = c["yx"][0], c["sc"][0]
    pix = yx[:, 0] * 256 + yx[:, 1]
    pos = np.argsort(np.argsort(pix))                       # position of each survivor in select_kernel's row-major compaction
    far256 = far4096 = False
    order = np.argsort(sc, kind="stable")
    for grp in np.split(order, np.nonzero(np.diff(sc[order]))[0] + 1):
        if len(grp) > 1:
            p = pos[grp]
            far256 = far256 or len(np.unique(p // 256)) > 1
            far4096 = far4096 or len(np.unique(p // 4096)) > 1
    c["conditions"] = [("more candidates than k", c["ncand"][0] == 65536 > k), ("equal survivors in different blocks of 256", far256), ("equal survivors in different blocks of 4096", far4096),
                       ("a second trip over j", k > 4096), ("a second trip over i, or k <= 16384", k <= 16384 or (k + 255) // 256 > 64)]
    return c


REUSE_SEQUENCE = [3000, -1, 10, 3000]


@functools.lru_cache(maxsize=None)
def reuse_case(k):
    """The `low` scores of topk_scores under max_keypoints = k (-1: keep all): the steps of one module's workspace through the top-k
    buffers, past them, and back."""
    c = detect_case(topk_scores("low"), 0, 0.0, 0, k, [])
    c["conditions"] = [("4096 candidates", c["ncand"] == [4096]), ("k of them kept, or all", len(c["sc"][0]) == (k if k > 0 else 4096)),
                       ("the top-k is engaged, or keep-all", k < 4096)]
    return c


# ---- D  descriptor sampling -----------------------------------------------------------------------------------------------------------
DESC_SHAPES = [(8, 8), (8, 64), (64, 8), (40, 72)]
ULP32 = 2.0 ** -23
C_REL = 4.0


def planted_coordinates(length):
    """0, the last, the middle, and 3 and 4 (the two sides of a cell centre) in the first, a middle and the last cell."""
    cells = sorted({0, (length // 8) // 2, length // 8 - 1})
    return sorted({0, length - 1, length // 2} | {8 * c + o for c in cells for o in (3, 4)})


def sample_reference(kp_xy, raw, align_corners, dtype):
    """so.dense_descriptors' normalisation, so.grid_sample_bilinear and so.sample_descriptors restated with a dtype: the grid coordinates
    ix, iy and their floor stay in fp32 (as in the oracle and in sample_kernel), the cell norms, the weights, the sum over the four taps and
    the final norm are in `dtype`.  raw [C, h, w] un-normalised, kp_xy [n, 2] (x, y) -> [C, n].  With dtype = float32 it IS the oracle."""
    c, h, w = raw.shape
    d = raw.astype(dtype)
    norm = np.sqrt((d ** 2).sum(axis=0, keepdims=True))
    d = (d / np.maximum(norm, dtype(1e-12))).astype(dtype)
    kp = kp_xy.astype(F32) - F32(4) + F32(0.5)
    kp = kp / np.array([w * 8 - 4 - 0.5, h * 8 - 4 - 0.5], F32)[None]
    kp = kp * F32(2) - F32(1)
    gx, gy = kp[:, 0], kp[:, 1]
    if align_corners:
        ix = (gx + F32(1)) / F32(2) * F32(w - 1)
        iy = (gy + F32(1)) / F32(2) * F32(h - 1)
    else:
        ix = ((gx + F32(1)) * F32(w) - F32(1)) / F32(2)
        iy = ((gy + F32(1)) * F32(h) - F32(1)) / F32(2)
    assert ix.dtype == F32 and iy.dtype == F32
    x0, y0 = np.floor(ix), np.floor(iy)
    out = np.zeros((c, len(gx)), dtype)
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wgt = (dtype(1) - np.abs(ix.astype(dtype) - xi.astype(dtype))) * (dtype(1) - np.abs(iy.astype(dtype) - yi.astype(dtype)))
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            xi_c, yi_c = np.clip(xi, 0, w - 1).astype(np.int64), np.clip(yi, 0, h - 1).astype(np.int64)
            out += d[:, yi_c, xi_c] * (wgt * ok).astype(dtype)[None]
            taps.append((ok, yi_c, xi_c))
    n = np.sqrt((out ** 2).sum(axis=0, keepdims=True))
    return (out / np.maximum(n, dtype(1e-12))).astype(dtype), taps


def special_cells(hc, wc, image):
    """(zero cell, cell scaled by 1e15) of an image, as (cy, cx) or None: opposite corners, swapped between the two images; a map of one
    cell is all zero in image 0 and all scaled in image 1."""
    first, last = (0, 0), (hc - 1, wc - 1)
    if first == last:
        return (first, None) if image == 0 else (None, first)
    return (first, last) if image == 0 else (last, first)


@functools.lru_cache(maxsize=None)
def descriptor_case(shape, align_corners):
    """b = 2.  Score maps hold single pixels of 1.0 (threshold 0.5, R = 0, border 0) at planted_coordinates(H) x planted_coordinates(W); the
    dense descriptors are standard normal with one all-zero cell and one cell scaled by 1e15 (special_cells).
    -> detect_case fields + dense [2, 256, hc, wc], kp [n, 2] (x, y) float32, ref64 / ref32 [2][256, n], zero_kp [2][n] bool: every in-range
    tap of the keypoint lies in the zero cell."""
    h, w = shape
    hc, wc = h // 8, w // 8
    ys, xs = planted_coordinates(h), planted_coordinates(w)
    score = np.zeros((2, h, w), F32)
    score[:, np.array(ys)[:, None], np.array(xs)[None, :]] = 1.0
    rs = np.random.RandomState(31 + h + 7 * w)
    dense = rs.standard_normal((2, 256, hc, wc)).astype(F32)
    for i in range(2):
        zero, big = special_cells(hc, wc, i)
        if zero is not None:
            dense[i][:, zero[0], zero[1]] = 0
        if big is not None:
            dense[i][:, big[0], big[1]] *= F32(1e15)
    c = detect_case(score, 0, 0.5, 0, -1, [], dense=dense)
    planted = np.array([(y, x) for y in ys for x in xs], np.int64)
    kp = planted[:, ::-1].astype(F32)
    ref64, ref32, zero_kp = [], [], []
    same_as_oracle, mixes = True, False
    for i in range(2):
        r64, taps = sample_reference(kp, dense[i], align_corners, np.float64)
        r32, _ = sample_reference(kp, dense[i], align_corners, F32)
        orc = so.sample_descriptors(kp, (dense[i] / np.maximum(np.sqrt((dense[i] ** 2).sum(axis=0, keepdims=True)), F32(1e-12))).astype(F32), 8, align_corners)
        same_as_oracle = same_as_oracle and np.array_equal(r32, orc)
        zero, big = special_cells(hc, wc, i)
        in_zero = np.ones(len(kp), bool)
        in_big, in_other = np.zeros(len(kp), bool), np.zeros(len(kp), bool)
        for ok, yi, xi in taps:
            in_zero &= (~ok | ((yi == zero[0]) & (xi == zero[1]))) if zero is not None else ~ok
            if big is not None:
                in_big |= ok & (yi == big[0]) & (xi == big[1])
                in_other |= ok & ~((yi == big[0]) & (xi == big[1]))
        mixes = mixes or bool((in_big & in_other).any())
        ref64.append(r64)
        ref32.append(r32)
        zero_kp.append(in_zero)
    corners = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}
    mids = {(0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)}
    have = set(map(tuple, planted.tolist()))
    cond = [("the oracle's keypoints are the planted ones, in both images", all(np.array_equal(yx, planted) for yx in c["yx"])),
            ("the fp32 restatement is the oracle, bit for bit", same_as_oracle),
            ("corners and edge midpoints", corners <= have and mids <= have),
            ("both sides of a cell centre on both axes", {3, 4} <= {y % 8 for y in ys} and {3, 4} <= {x % 8 for x in xs}),
            ("an interior point", any(0 < y < h - 1 and 0 < x < w - 1 for y, x in have)),
            ("a keypoint with every tap in the zero cell", bool(zero_kp[0].any())),
            ("such keypoints have an all-zero reference descriptor", all(not r[:, z].any() for r, z in zip(ref64, zero_kp))),
            ("a keypoint whose taps mix the scaled cell with another, or the map is one cell", mixes or hc * wc == 1),
            ("more than one workgroup of 16 keypoints, or the map has room for fewer", len(kp) > 16 or h * w <= 64),
            ("the reference is finite", all(np.isfinite(r).all() for r in ref64 + ref32))]
    c.update(conditions=cond, kp=kp, ref64=ref64, ref32=ref32, zero_kp=zero_kp, align_corners=align_corners, capacity=len(kp) + 3)
    return c


def descriptor_bound(ref64, ref32):
    """DESIGN 13's rule per keypoint: 4 x the fp32 oracle's own error against the fp64 restatement, plus 4 ulps of fp32 at the output scale
    (unit descriptors: 1.0) -> [n]."""
    return C_REL * np.abs(ref32.astype(np.float64) - ref64).max(axis=0) + 4 * ULP32
