"""K forwards of a bench.py config through gatsspg_forward with GATSSPG_FLAG_NO_DB_REUSE, one frame at a time: the PLAIN chain, whose per-launch
traffic bench.py's roofline prices (profiles/pmc_traffic.json).  A PMC pass through bench.py itself would average the empty and the windowed
launches of the reusing path into the per-launch figures.

    rocprofv3 --kernel-trace --pmc FETCH_SIZE -d OUT -o p -- python tools/plain_chain_steps.py [--config headline] [--steps 8]
"""
import argparse
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onepose_amd import _native
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="headline")
ap.add_argument("--steps", type=int, default=8)
a = ap.parse_args()
cfg = bench.CONFIGS[a.config]
dev = torch.device("cuda:0")
w = bench.Weights(dev, cfg["precision"])
w.flags |= _native.FLAG_NO_DB_REUSE
r = bench.Runner(dev, w, b=cfg["b"], n1=cfg["n1"], n2=cfg["n2"], golden_seed=bench.GOLDEN_SEEDS.get(cfg["golden"]))
for i in range(a.steps):
    r.step(i)
torch.cuda.synchronize()
print(f"{a.steps} plain-chain forwards of '{a.config}'")
