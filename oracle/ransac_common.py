"""What the numpy oracles of the geometry kernels (oracle/pnp_oracle.py, tests/detector_oracle.py, tests/mapping_oracle.py) share
with each other and, as integer arithmetic and fixed-order additions, with the kernels: the counter-based sampler of
csrc/ransac_sample.h and the lane-tree sum of csrc/wg_primitives.h.  TEST INFRASTRUCTURE ONLY, like the rest of oracle/.
"""
from __future__ import annotations

import numpy as np

_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample_indices(seed, hyp, n, k):
    """k distinct indices in [0, n) for hypothesis `hyp`: successive hash draws, duplicates rejected (a duplicate consumes its
    counter value; sampling::distinct<k> on the GPU)."""
    out, ctr = [], 0
    while len(out) < k:
        r = _splitmix64(((seed << 40) & _M64) ^ (hyp << 8) ^ ctr)
        ctr += 1
        idx = int((r >> 11) % n)
        if idx not in out:
            out.append(idx)
    return out


def lane_tree_sum(vals, lanes):
    """vals [m] or [m, Q] summed over the first axis as wg::tree_sum's callers do: lane t adds the rows t, t + lanes, ... in
    turn, then v[t] += v[t + s] for s = lanes / 2 .. 1."""
    vals = np.asarray(vals)
    part = np.zeros((lanes,) + vals.shape[1:], vals.dtype)
    for c0 in range(0, len(vals), lanes):
        chunk = vals[c0:c0 + lanes]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    s = lanes // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]
