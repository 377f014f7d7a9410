"""The thin-slab sweep behind PNP_FLATNESS_TAU (include/pnp.h) / FLATNESS_TAU (oracle/pnp_oracle.py): EPnP WITHOUT the flatness guard
over slabs of thickness 1 .. 1e-12 of their extent, binned by the decade of the covariance eigenvalue ratio (sigma_3 / sigma_1)^2.

    python tools/pnp_flatness_sweep.py                     the oracle (CPU), its guard switched off
    python tools/pnp_flatness_sweep.py --kernel LIB        also pnp_epnp of LIB, a libpnp_hip.so built with -DPNP_FLATNESS_TAU=-1e300

13 thickness ratios x {axis-aligned, three tilts} x two centroid offsets x six poses x n in {5, 6, 8, 40}; noise-free fp32 data as in
tests/pnp_geometry_cases.py.  Per decade: cases, refused (NaN / singular), broken (a finite pose whose worst reprojection exceeds
E_MAX = 2^-10 px), and the worst finite reprojection.  The guard belongs two decades above the highest decade with a broken case.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pnp_geometry_cases as gc          # noqa: E402
from oracle import pnp_oracle as po      # noqa: E402

THICKNESS = [10.0 ** -k for k in range(13)]
TILTS = [None, gc.TILT, gc.rotation([0.2, 0.1, 1.0], 1.3), gc.rotation([1.0, 1.0, 0.0], 0.4)]
OFFSETS = [np.zeros(3), gc.OFFSET]
VIEWS = ["generic", "identity", "corner", "near", "rot180x", "generic"]
NS = [5, 6, 8, 40]


def cases():
    for ti, th in enumerate(THICKNESS):
        for ri, tilt in enumerate(TILTS):
            for oi, off in enumerate(OFFSETS):
                for vi, view in enumerate(VIEWS):
                    for n in NS:
                        rs = np.random.RandomState(gc.seed_of("sweep", ti, ri, oi, vi, n))
                        p = rs.uniform(-gc.HALF, gc.HALF, (n, 3)) * np.array([1.0, 1.0, th])
                        p = (p @ tilt.T if tilt is not None else p) + off
                        yield gc.make(p.astype(np.float32), off, view, rs)


def oracle_unguarded(c):
    try:
        return gc.oracle_pose(c)
    except np.linalg.LinAlgError:
        return np.full((3, 4), np.nan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", metavar="LIB", help="a libpnp_hip.so built without the guard")
    ap.add_argument("--out", help="write the table as JSON here")
    args = ap.parse_args()
    po.FLATNESS_TAU = -math.inf                                          # the guard off: only a NaN or all-zero covariance is refused by it
    solvers = {"oracle": oracle_unguarded}
    if args.kernel:
        import torch
        from onepose_amd import _native_pnp, pnp
        _native_pnp.LIB_PATH = os.path.abspath(args.kernel)
        solvers["kernel"] = lambda c: pnp.epnp(c["K"], torch.from_numpy(c["pts_2d"]).cuda(), torch.from_numpy(c["pts_3d"]).cuda(), scale=gc.SCALE).cpu().numpy()
    table = {name: {} for name in solvers}
    for c in cases():
        ratio = gc.eigen_ratio(c["pts_3d"])
        decade = int(math.floor(math.log10(ratio))) if ratio > 0 else -99
        for name, solve in solvers.items():
            pose = solve(c)
            row = table[name].setdefault(decade, dict(cases=0, refused=0, broken=0, worst_px=0.0))
            row["cases"] += 1
            identity = np.array_equal(pose, np.eye(4)[:3])               # pnp_epnp's refusal
            if identity or not np.isfinite(pose).all():
                row["refused"] += 1
                continue
            e = gc.worst_reprojection(pose, c)
            row["worst_px"] = max(row["worst_px"], e)
            row["broken"] += int(not e <= c["e_max"])
    for name, rows in table.items():
        print(f"{name}: decade of the eigenvalue ratio | cases | refused | broken (> E_MAX) | worst finite reprojection, px")
        for decade in sorted(rows, reverse=True):
            r = rows[decade]
            print(f"  {'exactly 0' if decade == -99 else f'1e{decade:+d}':>10} | {r['cases']:5d} | {r['refused']:5d} | {r['broken']:5d} | {r['worst_px']:.3e}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({name: {str(d): r for d, r in rows.items()} for name, rows in table.items()}, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
