"""Host side of the object database builder that no kernel and no golden sees: track building on hand-written edges (the oracle
chain shares ``build_tracks`` with the module, so only this file can find a mistake in it), pair de-duplication, the frame lists
and the command line's exit when the scan is absent.  No GPU needed."""
import os

import numpy as np

from onepose_amd import mapping


def tracks_of(n_kpts, pairs, edges, **kw):
    offs, img, kpt = mapping.build_tracks(n_kpts, pairs, [np.array(e, np.int64).reshape(-1, 2) for e in edges], **kw)
    return [list(zip(img[s:e].tolist(), kpt[s:e].tolist())) for s, e in zip(offs[:-1], offs[1:])]


def test_components_are_ordered_by_smallest_node_and_observations_by_image():
    # images 0, 1, 2 with 5 keypoints each; component A = {(0,3), (1,0), (2,4)}, component B = {(0,1), (2,0)}, C = {(1,2), (2,1)}
    pairs = [(0, 1), (1, 2), (0, 2), (1, 2)]
    edges = [[(3, 0)], [(0, 4)], [(1, 0)], [(2, 1)]]
    assert tracks_of([5, 5, 5], pairs, edges) == [[(0, 1), (2, 0)], [(0, 3), (1, 0), (2, 4)], [(1, 2), (2, 1)]]
    # the orientation and the order of the pairs do not matter
    assert tracks_of([5, 5, 5], [(2, 1), (2, 0), (1, 0), (2, 1)], [[(1, 2)], [(0, 1)], [(0, 3)], [(4, 0)]]) == [
        [(0, 1), (2, 0)], [(0, 3), (1, 0), (2, 4)], [(1, 2), (2, 1)]]


def test_an_image_seen_twice_in_a_component_keeps_its_lowest_keypoint():
    # (0,2)-(1,3) and (0,2)-(1,1): image 1 occurs twice; (1,1)-(2,0) hangs on the one that is kept, (1,3)-(2,4) on the dropped one
    pairs = [(0, 1), (0, 1), (1, 2), (1, 2)]
    edges = [[(2, 3)], [(2, 1)], [(1, 0)], [(3, 4)]]
    assert tracks_of([4, 4, 5], pairs, edges) == [[(0, 2), (1, 1), (2, 0)]]          # image 2 too: keypoint 0 of {0, 4}


def test_ragged_keypoint_counts_and_unmatched_keypoints():
    assert tracks_of([1, 7, 2], [(0, 1), (1, 2)], [[(0, 6)], [(6, 1)]]) == [[(0, 0), (1, 6), (2, 1)]]
    offs, img, kpt = mapping.build_tracks([3, 3], [(0, 1)], [np.zeros((0, 2), np.int64)])
    assert offs.tolist() == [0] and len(img) == len(kpt) == 0
    assert offs.dtype == img.dtype == kpt.dtype == np.int32


def test_a_track_longer_than_the_bound_keeps_its_first_observations():
    n = 9
    pairs = [(v, v + 1) for v in range(n - 1)]
    edges = [[(0, 0)]] * (n - 1)
    assert tracks_of([1] * n, pairs, edges) == [[(v, 0) for v in range(n)]]
    assert tracks_of([1] * n, pairs, edges, max_track_length=4) == [[(v, 0) for v in range(4)]]
    two = tracks_of([2] * n, pairs, [[(0, 0), (1, 1)]] * (n - 1), max_track_length=4)
    assert two == [[(v, 0) for v in range(4)], [(v, 1) for v in range(4)]]


def test_unordered_pairs_are_matched_once_in_their_first_orientation():
    assert mapping.unique_pairs([(0, 1), (1, 0), (2, 1), (0, 1), (1, 2), (3, 0)]) == [(0, 1), (2, 1), (3, 0)]


def test_point_observations_follow_members_then_images():
    offs = np.array([0, 3, 5, 8], np.int32)
    img = np.array([0, 1, 2, 0, 2, 1, 2, 3], np.int32)
    kpt = np.array([5, 6, 7, 1, 2, 8, 9, 4], np.int32)
    mask = np.array([1, 0, 1, 1, 1, 1, 1, 0], np.int32)
    # kept tracks 2, 0 (positions 0, 1 of kept_ids [0, 2]); merged point 0 = {position 0, 1}, i.e. tracks 0 then 2
    po, gi, gk = mapping.point_observations(offs, img, kpt, mask, np.array([0, 2]), np.array([0, 2]), np.array([0, 1]))
    assert po.tolist() == [0, 4] and gi.tolist() == [0, 2, 1, 2] and gk.tolist() == [5, 7, 8, 9]


def test_frame_lists_take_every_fifth_frame_in_index_order(tmp_path):
    for seq, frames in (("obj-1", [0, 3, 5, 10, 100, 20]), ("obj-2", [15, 7])):
        os.makedirs(tmp_path / "obj" / seq / "color")
        for k in frames:
            (tmp_path / "obj" / seq / "color" / f"{k}.png").write_bytes(b"")
    root, imgs, seq_ids = mapping.scan_lists(str(tmp_path), "obj")
    assert [os.path.basename(f) for f in imgs] == ["0.png", "5.png", "10.png", "20.png", "100.png", "15.png"]
    assert seq_ids == ["obj-1"] * 5 + ["obj-2"] and root == str(tmp_path / "obj")
    assert mapping.scan_lists(str(tmp_path), "obj", ["obj-2"])[2] == ["obj-2"]


def test_command_line_says_what_it_looked_for_and_exits_zero(tmp_path, capsys):
    assert mapping.main(["--data-dir", str(tmp_path), "--object", "0408-colorbox-box", "--models-dir", str(tmp_path / "models")]) == 0
    out = capsys.readouterr().out
    assert "nothing to build" in out and "superpoint_v1.pth" in out and "superglue_outdoor.pth" in out and "box3d_corners.txt" in out
    assert os.path.join("<sequence>", "color", "*.png") in out
