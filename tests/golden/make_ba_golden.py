"""Generate the bundle-adjustment residual golden (tests/golden/ba_residual_golden.npz) by RUNNING THE REFERENCE'S RESIDUAL.

Build container only (needs the reference checkout):
    ONEPOSE_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ba_golden.py

``SnavelyReprojectionErrorV2`` (src/tracker/tracking_utils.py:91-169) is imported unmodified and run on the CPU in fp64 on the
inputs of ``ba_cases.golden_inputs`` (rotation angles exactly 0, 1e-8, 1e-3, about 1 and pi - 1e-3); the Jacobians are its
autograd's.  Stored: the inputs, the residuals and the Jacobians -- data only, nothing of the reference's text.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["ONEPOSE_REFERENCE"])
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.tracker.tracking_utils import SnavelyReprojectionErrorV2  # noqa: E402  (reference)
import ba_cases  # noqa: E402


def main():
    cams, points, feats = ba_cases.golden_inputs()
    M = len(cams)
    c = torch.tensor(cams, dtype=torch.float64, requires_grad=True)
    p = torch.tensor(points, dtype=torch.float64, requires_grad=True)
    f = torch.tensor(feats, dtype=torch.float64)
    res = SnavelyReprojectionErrorV2(p, c, f)
    Jc, Jp = np.empty((M, 2, 6)), np.empty((M, 2, 3))
    for row in range(2):        # observation m depends on row m of the cameras and points alone: one backward pass per residual row
        gc, gp = torch.autograd.grad(res[:, row].sum(), [c, p], retain_graph=True)
        Jc[:, row], Jp[:, row] = gc.numpy(), gp.numpy()
    path = os.path.join(HERE, "ba_residual_golden.npz")
    np.savez_compressed(path, cams=cams, points=points, features=feats, residual=res.detach().numpy(), Jc=Jc, Jp=Jp)
    print(f"{M} observations, {os.path.getsize(path)} bytes, residuals finite: {bool(np.isfinite(res.detach().numpy()).all())}, "
          f"Jacobians finite: {bool(np.isfinite(Jc).all() and np.isfinite(Jp).all())}")


if __name__ == "__main__":
    main()
