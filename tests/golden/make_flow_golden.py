"""Record what cv2.calcOpticalFlowPyrLK gives on the flow step's seeded cases, next to the oracle's results.

    python tests/golden/make_flow_golden.py     (needs cv2)

Writes tests/golden/flow_cv2_record.json: per case the share of equal statuses, how many points each side tracked and the
distribution (median, 90 %, 99 %, max) of the distance between the two results over the points both tracked.  Nothing here has
been run where the flow step was developed (no cv2): parity with OpenCV is unpinned until this file exists.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import flow_cases as fc  # noqa: E402


def main():
    import cv2
    from test_flow_cv2 import compare
    rec = {"cv2": cv2.__version__, "cases": [compare(case)[0] for case in fc.all_cases() if case.init is None]}
    with open(os.path.join(HERE, "flow_cv2_record.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
