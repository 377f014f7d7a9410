"""Golden for the post-processing of the object database builder, produced by RUNNING THE REFERENCE:
pairs_from_poses.covis_from_pose, filter_tkl.get_tkl, filter_points.filter_3d and merge, feature_process.get_kpt_ann.

Run where the reference is available:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_map_golden.py

The input is a synthetic COLMAP model (onepose_amd.synthetic.make_map_model, regenerated from its seed wherever the golden is
consumed) written with the reference's own write_model into a temporary directory, with pose files and a box file beside it.
cv2, h5py, loguru and matplotlib are imported by those modules but not touched by the functions used here: they are stubbed in
sys.modules, and the h5py stub's File returns the features as a dict of numpy arrays (which satisfy the
``feature[...].__array__()`` accesses).  Only the reference's OUTPUTS are stored, in tests/golden/map_post.npz.
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REF = os.environ.get("ONEPOSE_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("GOLDEN_OUT", HERE)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
FEATURES = {}
for name in ("cv2", "loguru", "h5py", "matplotlib", "matplotlib.pyplot"):
    if name not in sys.modules:
        m = types.ModuleType(name)
        m.logger = None
        sys.modules[name] = m
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
sys.modules["h5py"].File = lambda path, mode="r": FEATURES

import numpy as np  # noqa: E402

from src.sfm import pairs_from_poses  # noqa: E402  (reference)
from src.sfm.postprocess import feature_process, filter_points, filter_tkl  # noqa: E402  (reference)
from src.utils.colmap import read_write_model as rw  # noqa: E402  (reference)
from onepose_amd import synthetic  # noqa: E402

SEED = 7


def main():
    model = synthetic.make_map_model(SEED)
    V, T = len(model["poses"]), len(model["xyz"])
    with tempfile.TemporaryDirectory() as tmp:
        names = [os.path.join(tmp, "obj", model["seq_ids"][v], "color", f"{v}.png") for v in range(V)]
        for v, name in enumerate(names):
            os.makedirs(os.path.dirname(name).replace("/color", "/poses_ba"), exist_ok=True)
            np.savetxt(name.replace("/color/", "/poses_ba/").replace(".png", ".txt"), np.concatenate([model["poses"][v], [[0, 0, 0, 1.0]]]))
            FEATURES[name] = model["features"][v]
        box_path = os.path.join(tmp, "obj", "box3d_corners.txt")
        np.savetxt(box_path, model["box"])
        pairs_file = os.path.join(tmp, "pairs.txt")
        pairs_from_poses.covis_from_pose(names, pairs_file, 10, max_rotation=50)
        index = {n: v for v, n in enumerate(names)}
        with open(pairs_file) as f:
            pairs = np.array([[index[a], index[b]] for a, b in (line.split(" ") for line in f.read().split("\n") if line)], np.int64)

        outputs_dir = os.path.join(tmp, "outputs")
        model_dir = os.path.join(outputs_dir, "sfm_ws", "model")
        os.makedirs(model_dir)
        offs, obs_image, obs_kpt = model["track_offsets"], model["obs_image"], model["obs_kpt"]
        cameras = {1: rw.Camera(id=1, model="PINHOLE", width=128, height=96, params=np.array([280.0, 280.0, 64.0, 48.0]))}
        images = {}
        for v in range(V):
            ids = np.full(len(model["features"][v]["keypoints"]), -1, np.int64)
            images[v + 1] = [ids, model["features"][v]["keypoints"].astype(np.float64)]
        points = {}
        for t in range(T):
            s, e = offs[t], offs[t + 1]
            for v, k in zip(obs_image[s:e], obs_kpt[s:e]):
                images[v + 1][0][k] = t
            points[t] = rw.Point3D(id=t, xyz=model["xyz"][t], rgb=np.zeros(3, np.uint8), error=0.0, image_ids=obs_image[s:e] + 1,
                                   point2D_idxs=obs_kpt[s:e])
        images = {i: rw.Image(id=i, qvec=rw.rotmat2qvec(model["poses"][i - 1][:, :3]), tvec=model["poses"][i - 1][:, 3], camera_id=1,
                              name=names[i - 1], xys=xys, point3D_ids=ids) for i, (ids, xys) in images.items()}
        rw.write_model(cameras, images, points, model_dir, ".bin")

        track_length, _ = filter_tkl.get_tkl(model_dir, thres=model["max_num_kp3d"], show=False)
        xyzs, points_idxs = filter_points.filter_3d(model_dir, track_length, box_path)
        merge_xyzs, merge_idxs = filter_points.merge(xyzs, points_idxs, dist_threshold=1e-3)
        cfg = types.SimpleNamespace(network=types.SimpleNamespace(detection="superpoint"))
        feature_process.get_kpt_ann(cfg, names, "feats.h5", outputs_dir, merge_idxs, merge_xyzs)
        anno = os.path.join(outputs_dir, "anno")
        avg, clt, idxs = np.load(os.path.join(anno, "anno_3d_average.npz")), np.load(os.path.join(anno, "anno_3d_collect.npz")), np.load(
            os.path.join(anno, "idxs.npy"))
        members = [np.asarray(merge_idxs[k]) for k in range(len(merge_idxs))]
        out = dict(pairs=pairs, track_length=np.int64(track_length), kept_xyz=np.asarray(xyzs), kept_ids=np.asarray(points_idxs),
                   merged_xyz=np.asarray(merge_xyzs), member_offsets=np.concatenate([[0], np.cumsum([len(m) for m in members])]),
                   members=np.concatenate(members), idxs=idxs,
                   avg_keypoints3d=avg["keypoints3d"], avg_descriptors3d=avg["descriptors3d"], avg_scores3d=avg["scores3d"],
                   clt_keypoints3d=clt["keypoints3d"], clt_descriptors3d=clt["descriptors3d"], clt_scores3d=clt["scores3d"])
    for k, v in out.items():
        print(k, v.dtype, v.shape)
    print("track_length", track_length, "kept", len(out["kept_ids"]), "merged", len(members), "largest", max(len(m) for m in members))
    np.savez_compressed(os.path.join(OUT, "map_post.npz"), **out)


if __name__ == "__main__":
    main()
