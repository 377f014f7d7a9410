"""Generate the map update golden (tests/golden/track_golden.npz) by RUNNING THE REFERENCE'S OWN FUNCTIONS on the CPU.

Build container only (needs the reference checkout):
    ONEPOSE_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_track_golden.py

``BATracker._triangulatePy`` and ``BATracker.cm_degree_5_metric`` (src/tracker/ba_tracker.py:251-265, 105-111) and ``project``
(src/tracker/tracking_utils.py:74-88) are imported unmodified and run on the inputs of ``track_cases.golden_cases``.
``ba_tracker.py`` imports ``cv2`` and ``DeepLM`` at the top; where they are not installed, empty stand-in modules of those names are
put into ``sys.modules`` before the import -- the three functions use neither library.  Per case the golden also holds the DLT
solution from ``numpy.linalg.svd`` of A itself (the last right singular vector): a second reference-grade answer whose distance
to the first gives the tolerance its scale.  Stored: results only -- data, nothing of the reference's text.
"""
import importlib
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["ONEPOSE_REFERENCE"])
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402


def stand_in(name, **attrs):
    """An empty module under `name` (and its parents) unless the real one imports."""
    try:
        importlib.import_module(name)
        return
    except Exception:
        pass
    parts = name.split(".")
    for k in range(1, len(parts) + 1):
        sys.modules.setdefault(".".join(parts[:k]), types.ModuleType(".".join(parts[:k])))
    for key, value in attrs.items():
        setattr(sys.modules[name], key, value)


stand_in("cv2")
stand_in("DeepLM.TorchLM.solver", Solve=None)

from src.tracker.ba_tracker import BATracker  # noqa: E402  (reference)
from src.tracker.tracking_utils import project  # noqa: E402  (reference)
import track_cases  # noqa: E402


def svd_dlt(P1, P2, a, b):
    out = []
    for p1, p2 in zip(a, b):
        A = np.stack([p1[0] * P1[2] - P1[0], p1[1] * P1[2] - P1[1], p2[0] * P2[2] - P2[0], p2[1] * P2[2] - P2[1]])
        v = np.linalg.svd(A)[2][3]
        out.append(v[:3] / v[3])
    return np.array(out)


def main():
    out = {}
    for name, c in sorted(track_cases.golden_cases().items()):
        i = np.where(c["matches0"] >= 0)[0]
        j = c["matches0"][i]
        ids = c["kf_pt_ids"][i]
        cand, known = ids == -1, ids >= 0
        P1, P2 = c["K_kf"] @ c["pose_kf"][:3], c["K_q"] @ c["pose_q"][:3]
        a, b = c["kf_xy"][i[cand]], c["q_xy"][j[cand]]
        X = BATracker._triangulatePy(None, P1, P2, a, b)
        out[name + "/X"] = X
        out[name + "/X_svd"] = svd_dlt(P1, P2, a.astype(np.float64), b.astype(np.float64))
        out[name + "/rep_q"] = project(X, c["K_q"], c["pose_q"][:3])
        out[name + "/rep_kf"] = project(X, c["K_kf"], c["pose_kf"][:3])
        out[name + "/known_rep_q"] = project(c["points"][ids[known]], c["K_q"], c["pose_q"][:3])
    out["metric"] = np.array([BATracker.cm_degree_5_metric(None, p, t) for p, t in track_cases.METRIC_POSES])
    path = os.path.join(HERE, "track_golden.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
