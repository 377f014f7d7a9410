"""Generate the nearest-neighbour golden vectors (tests/golden/nn_*.npz) by RUNNING THE REFERENCE MODULE.

Build container only (needs the reference checkout):
    ONEPOSE_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nn_golden.py

The reference ``NearestNeighbour`` (src/models/matchers/nn/nearest_neighbour.py:26-63) is imported unmodified and run on CPU in
fp32 on the pairs of ``nn_oracle.make_pair``.  Stored per case: the inputs, the configuration (JSON) and the four reference
outputs -- data only, nothing of the reference's text.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["ONEPOSE_REFERENCE"])
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.models.matchers.nn.nearest_neighbour import NearestNeighbour  # noqa: E402  (reference)
import nn_oracle  # noqa: E402

# name -> (pairs of one batch as (n0, n1, seed), conf)
CASES = {
    "tiny": ([(2, 2, 1)], {"ratio_threshold": 0.8}),
    "plain": ([(63, 65, 2)], {}),
    "ratio": ([(64, 128, 3)], {"ratio_threshold": 0.8}),
    "distance": ([(129, 127, 4)], {"distance_threshold": 0.7}),
    "both": ([(200, 170, 5)], {"ratio_threshold": 0.9, "distance_threshold": 0.9}),
    "nomutual": ([(129, 127, 6)], {"ratio_threshold": 0.8, "distance_threshold": 0.7, "do_mutual_check": False}),
    "batch": ([(70, 90, 7), (70, 90, 8), (70, 90, 9)], {"ratio_threshold": 0.8, "distance_threshold": 0.7}),
}


def main():
    for name, (pairs, conf) in CASES.items():
        d = [nn_oracle.make_pair(*p) for p in pairs]
        d0, d1 = np.stack([x[0] for x in d]), np.stack([x[1] for x in d])
        with torch.no_grad():
            out = NearestNeighbour(conf)({"descriptors0": torch.from_numpy(d0), "descriptors1": torch.from_numpy(d1)})
        path = os.path.join(HERE, f"nn_{name}.npz")
        np.savez_compressed(path, descriptors0=d0, descriptors1=d1, conf=np.array(json.dumps(conf)),
                            **{k: out[k].numpy() for k in nn_oracle.OUT_KEYS})
        print(f"{name}: {os.path.getsize(path)} bytes, dtypes {[str(out[k].dtype) for k in nn_oracle.OUT_KEYS]}, "
              f"{int((out['matches0'] > -1).sum())} of {out['matches0'].numel()} rows matched")


if __name__ == "__main__":
    main()
