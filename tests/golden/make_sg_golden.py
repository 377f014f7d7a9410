"""Generate the SuperGlue golden vectors (tests/golden/sg_*.npz) by RUNNING THE REFERENCE MODULE.

Build container only (needs the reference checkout):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sg_golden.py

The reference ``SuperGlue`` (src/models/matchers/SuperGlue/superglue.py:173-276) is imported unmodified, loaded with the
seeded synthetic weights of ``onepose_amd.synthetic`` and run on CPU in fp32.  Weights and inputs are regenerated from seeds
where the goldens are consumed; only reference OUTPUTS are stored: the four outputs and either the full log transport plan
Z (small cases) or its row / column best and second-best values plus the dustbin row and column (large cases).
"""
import json
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("ONEPOSE_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.models.matchers.SuperGlue.superglue import SuperGlue  # noqa: E402  (reference)
from onepose_amd import synthetic  # noqa: E402
import superglue_oracle  # noqa: E402

OUTDOOR = {"descriptor_dim": 256, "GNN_layers": ["self", "cross"] * 9, "sinkhorn_iterations": 100, "match_threshold": 0.7}
SHORT = {"GNN_layers": ["self", "cross"]}

CASES = {
    "tiny": dict(w=dict(kind="rand", seed=0), inp=dict(b=2, n0=37, n1=53, h=480, w=640, seed=1), cfg={}, store="full"),
    "iters0": dict(w=dict(kind="rand", seed=2), inp=dict(b=1, n0=37, n1=53, h=480, w=640, seed=3),
                   cfg=dict(SHORT, sinkhorn_iterations=0), store="full"),
    "iters1": dict(w=dict(kind="rand", seed=2), inp=dict(b=1, n0=37, n1=53, h=480, w=640, seed=3),
                   cfg=dict(SHORT, sinkhorn_iterations=1), store="full"),
    "n1": dict(w=dict(kind="rand", seed=4), inp=dict(b=1, n0=1, n1=40, h=512, w=512, seed=5), cfg=dict(OUTDOOR), store="full"),
    "planted": dict(w=dict(kind="passthrough", seed=6), inp=dict(b=1, n0=300, n1=400, h=512, w=512, seed=7, planted=120),
                    cfg=dict(OUTDOOR), store="full"),
    "outdoor": dict(w=dict(kind="rand", seed=8), inp=dict(b=1, n0=512, n1=700, h=512, w=512, seed=9), cfg=dict(OUTDOOR),
                    store="stats"),
    "headline": dict(w=dict(kind="rand", seed=10), inp=dict(b=1, n0=2048, n1=2048, h=512, w=512, seed=11), cfg=dict(OUTDOOR),
                     store="stats"),
    "stress": dict(w=dict(kind="rand", seed=12), inp=dict(b=1, n0=4096, n1=4096, h=512, w=512, seed=13), cfg=dict(OUTDOOR),
                   store="stats"),
    # peaked attention (attn_gain scales the q / k projections: median row logit spread 9.7-13.9 in every layer), K/V tile tails
    # (517 = 8 * 64 + 5, 300 = 2 * 128 + 44), per-side image sizes, planted pairs that pass threshold 0.2
    "peaked": dict(w=dict(kind="rand", seed=50, attn_gain=30.0, proj_gain=20.0),
                   inp=dict(b=1, n0=300, n1=517, h=512, w=512, h1=480, w1=640, seed=51, planted=100),
                   cfg=dict(OUTDOOR, match_threshold=0.2), store="full"),
    # default weights, b = 3, one query block plus one point / one K/V tile plus one source, per-side sizes, side 1 taller than wide
    "sizes": dict(w=dict(kind="rand", seed=52), inp=dict(b=3, n0=129, n1=65, h=480, w=640, h1=700, w1=300, seed=53),
                  cfg=dict(OUTDOOR, match_threshold=0.2), store="full"),
}


def weights(spec, n_layers):
    fn = synthetic.make_superglue_passthrough_state_dict if spec["kind"] == "passthrough" else synthetic.make_superglue_state_dict
    return fn(spec["seed"], n_layers, **{k: v for k, v in spec.items() if k not in ("kind", "seed")})


def full_config(cfg):
    return {**SuperGlue.default_config, **cfg}


def run_case(spec):
    cfg = full_config(spec["cfg"])
    sd = weights(spec["w"], len(cfg["GNN_layers"]))
    model = SuperGlue(dict(cfg)).eval()
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    inp = synthetic.make_superglue_inputs(**spec["inp"])
    b = spec["inp"]["b"]
    data = {k: torch.from_numpy(inp[k]) for k in ("keypoints0", "keypoints1", "scores0", "scores1", "descriptors0", "descriptors1")}
    for s in (0, 1):      # each side's own image size: normalize_keypoints reads data["image<s>"].shape
        h, w = (int(x) for x in inp[f"image_size{s}"])
        data[f"image{s}"] = torch.zeros(b, 1, h, w)
    captured = {}

    # capture Z: the last log_optimal_transport output is what forward thresholds; recompute it from the scores the
    # reference computed (hook on final_proj, not an edit of the module)
    def hook(mod, args, out):
        captured.setdefault("mdesc", []).append(out.detach())
    hdl = model.final_proj.register_forward_hook(hook)
    with torch.no_grad():
        pred = model(data)
    hdl.remove()
    md0, md1 = captured["mdesc"]
    from src.models.matchers.SuperGlue.superglue import log_optimal_transport
    with torch.no_grad():
        scores = torch.einsum("bdn,bdm->bnm", md0, md1) / 256 ** 0.5
        Z = log_optimal_transport(scores, model.bin_score, iters=cfg["sinkhorn_iterations"]).numpy()
    out = {k: v.numpy() for k, v in pred.items()}
    out["matches0"] = out["matches0"].astype(np.int64)
    out["matches1"] = out["matches1"].astype(np.int64)
    if spec["store"] == "full":
        out["Z"] = Z.astype(np.float32)
    else:
        out.update({k: v.astype(np.float32) for k, v in superglue_oracle.z_stats(Z).items()})
    return out, cfg


def main():
    meta = {"cases": {}, "state_dict_keys": list(SuperGlue(dict(OUTDOOR)).state_dict().keys())}
    only = sys.argv[1:]
    for name, spec in CASES.items():
        if only and name not in only:
            continue
        out, cfg = run_case(spec)
        path = os.path.join(HERE, f"sg_{name}.npz")
        np.savez_compressed(path, **out)
        meta["cases"][name] = dict(spec, cfg=cfg)
        print(f"{name}: {os.path.getsize(path) / 1e3:.1f} kB, matches0 valid {int((out['matches0'] >= 0).sum())}", flush=True)
    mp = os.path.join(HERE, "sg_golden_meta.json")
    if only and os.path.exists(mp):
        with open(mp) as f:
            old = json.load(f)
        old["cases"].update(meta["cases"])
        meta["cases"] = old["cases"]
    with open(mp, "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
