"""The oracle of the flow step against OpenCV itself, where cv2 is importable (it is not where this was developed: these tests
are skipped there, and parity with cv2.calcOpticalFlowPyrLK is NOT claimed anywhere).  They RECORD the differences -- printed
with -s -- the share of equal statuses and the distribution of the point distances.  No bound on those is fixed: nobody has
measured them (OpenCV keeps the points and the 2x2 algebra in fp32 and accumulates in SIMD order).  The one assertion is what
both must do: recover a planted shift.  tests/golden/make_flow_golden.py records the same figures into
tests/golden/flow_cv2_record.json."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import flow_cases as fc  # noqa: E402
from onepose_amd import flow  # noqa: E402,F401


def compare(case):
    """Share of equal statuses and the distances between the two results over the points both tracked."""
    criteria = (cv2.TERM_CRITERIA_EPS | cv2.TERM_CRITERIA_COUNT, case.max_iter, case.eps)
    ref, ref_status, _ = cv2.calcOpticalFlowPyrLK(case.first, case.second, case.pts[:, None], None, winSize=case.win,
                                                  maxLevel=case.max_level, criteria=criteria)
    nxt, status = case.result[:2]
    ref, ref_status = ref[:, 0], ref_status[:, 0].astype(np.int32)
    both = (status == 1) & (ref_status == 1)
    dist = np.linalg.norm(nxt[both].astype(np.float64) - ref[both], axis=1)
    q = np.quantile(dist, [0.5, 0.9, 0.99, 1.0]).tolist() if both.any() else [float("nan")] * 4
    return {"case": case.name, "points": len(status), "equal_status_share": float((status == ref_status).mean()),
            "oracle_tracked": int(status.sum()), "cv2_tracked": int(ref_status.sum()),
            "distance_px": dict(zip(("median", "p90", "p99", "max"), q))}, ref, ref_status


@pytest.mark.parametrize("case", fc.planted_cases() + [fc.short_pyramid_case(), fc.border_case(), fc.noisy_case()], ids=lambda c: c.name)
def test_record_the_differences_to_cv2(case):
    rec, ref, ref_status = compare(case)
    print(rec)
    if case.planted is not None and case.name.startswith("planted"):
        assert ref_status.all() and np.abs(ref - (case.pts + np.array(case.planted, np.float32))).max() < 0.5      # a gross failure only
