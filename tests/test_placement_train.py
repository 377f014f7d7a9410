"""Placement tests of the matcher's training head (include/gatsspg_train.h): every entry point with its device arguments carved
exactly, back to back with 64 KiB guards, from an arena (tests/arena.py), under the fill patterns 0xFF and 0x00.  The arena run writes
nothing outside its outputs and its workspace of exactly gtr_workspace_bytes, equals the plain run bit for bit, and gives the same
bits under both patterns.  Then the two things no test had passed before: a ``cls`` that is not 4-byte aligned, and class values
other than 0, 1, 2.  Every test runs a second time with each call captured and replayed (arena.run_captured).  All comparisons are bitwise; the oracle comparisons stay in tests/test_training_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import train_oracle
from arena import bitwise_equal, captured_twin, run_placement
from onepose_amd import _native_train

BINDING = _native_train
ROLES = {
    "gtr_build_target": dict(pairs="in", cls="out", negative_pairs="out"),
    "gtr_loss_head": dict(x="in", y="in", cls="in", loss="out", counts="out", dx="out", dy="out", workspace="scratch"),
    "gtr_scores_exp": dict(x="in", y="in", E="out", r="out", c="out", workspace="scratch"),
    "gtr_loss_terms": dict(E="in", r="in", c="in", cls="in", loss_sums="out", counts="out", loss="out", rowsum_h="out", colsum_h="out",
                           workspace="scratch"),
    "gtr_score_grad": dict(E="in", r="in", c="in", cls="in", counts="in", rowsum_h="in", colsum_h="in", dS="out", workspace="scratch"),
}
CASES = ["1x1x1_only_positive", "1x127x63", "2x129x65_pad0_gamma1.5", "2x200x333"]
BAND = "3x128x64_ignored_band"
# the multi-tile case with m % 4 == 0 (128 x 64 tiles: two row tiles, three column tiles), with an ignored band as BAND has
M132 = (dict(b=2, n=130, m=132, k=20, seed=21, noise=0.8, n_orig=120, m_orig=125, pad_val=-1), train_oracle.DEFAULT)
_cache = {}


def case(name):
    """x, y, pairs, cls (torch, on the host) and the focal arguments of a case, built once and shared read-only"""
    if name not in _cache:
        inputs, focal = M132 if name == "2x130x132" else train_oracle.GPU_CASES[name]
        x, y, pairs, target = train_oracle.make_head_case(**inputs)
        _cache[name] = dict(x=torch.from_numpy(x), y=torch.from_numpy(y), pairs=pairs, cls=torch.from_numpy(train_oracle.classes(target)),
                            focal=focal, inputs=inputs)
    return _cache[name]


def shape(c):
    return c["x"].shape[0], c["x"].shape[2], c["y"].shape[2]


def workspace(mem, b, n, m):
    nbytes = BINDING.load().gtr_workspace_bytes(b, n, m)
    assert nbytes > 0
    return mem.place(nbytes, "scratch", "workspace")


def head_body(c, grads=True, cls=None, cls_skew=0):
    b, n, m = shape(c)
    f = c["focal"]

    def body(mem):
        x, y = mem.place(c["x"], "in", "x"), mem.place(c["y"], "in", "y")
        k = mem.place(c["cls"] if cls is None else cls, "in", "cls", skew=cls_skew)
        assert k.data_ptr() % 4 == cls_skew
        loss, counts = mem.place(torch.empty(1), "out", "loss"), mem.place(torch.empty(3, dtype=torch.int64), "out", "counts")
        dx, dy = (mem.place(torch.empty_like(c["x"]), "out", "dx"), mem.place(torch.empty_like(c["y"]), "out", "dy")) if grads else (None, None)
        ws = workspace(mem, b, n, m)
        mem.call(BINDING, "gtr_loss_head", x, y, k, b, n, m, f["alpha"], f["gamma"], f["pos_w"], f["neg_w"], f["scale"], loss, counts, dx, dy,
                 ws, ws.numel())
        return dict(loss=loss, counts=counts, dx=dx, dy=dy) if grads else dict(loss=loss, counts=counts)
    return body


pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("grads", [True, False], ids=["with_dx_dy", "forward_only"])
@pytest.mark.parametrize("name", CASES)
def test_loss_head(name, grads, run=run_placement):
    got = run(head_body(case(name), grads), DEV, ROLES)
    assert not torch.isnan(got["loss"]).any() and int(got["counts"].sum()) == case(name)["cls"].numel()


@pytest.mark.parametrize("name", CASES)
def test_stage_entries(name, run=run_placement):
    """gtr_scores_exp, then gtr_loss_terms on its E, r, c, then gtr_score_grad on the counts and H sums of that: the outputs of one
    stage are the ``const`` inputs of the next, and protected there."""
    c = case(name)
    b, n, m = shape(c)
    f = c["focal"]
    focal = (f["alpha"], f["gamma"], f["pos_w"], f["neg_w"])

    def body(mem):
        x, y, cls = mem.place(c["x"], "in", "x"), mem.place(c["y"], "in", "y"), mem.place(c["cls"], "in", "cls")
        E, r, cc = (mem.place(torch.empty(s), "out", nm) for s, nm in (((b, n, m), "E"), ((b, n), "r"), ((b, m), "c")))
        sums, counts = mem.place(torch.empty(2, dtype=torch.float64), "out", "loss_sums"), mem.place(torch.empty(3, dtype=torch.int64), "out", "counts")
        loss, rowh, colh = (mem.place(torch.empty(s), "out", nm) for s, nm in (((1,), "loss"), ((b, n), "rowsum_h"), ((b, m), "colsum_h")))
        dS = mem.place(torch.empty(b, n, m), "out", "dS")
        ws = workspace(mem, b, n, m)
        mem.call(BINDING, "gtr_scores_exp", x, y, b, n, m, f["scale"], E, r, cc, ws, ws.numel())
        mem.call(BINDING, "gtr_loss_terms", E, r, cc, cls, b, n, m, *focal, sums, counts, loss, rowh, colh, ws, ws.numel())
        mem.call(BINDING, "gtr_score_grad", E, r, cc, cls, counts, rowh, colh, b, n, m, *focal, dS, ws, ws.numel())
        return dict(E=E, r=r, c=cc, loss_sums=sums, counts=counts, loss=loss, rowsum_h=rowh, colsum_h=colh, dS=dS)

    got = run(body, DEV, ROLES)
    assert not any(torch.isnan(v.double()).any() for v in got.values())


@pytest.mark.parametrize("name", CASES)
def test_build_target(name, run=run_placement):
    """The case's pairs, with one pair of negative indices and one past the shape appended to the first sample (kcap two over the
    longest list); n_orig, m_orig as the case pads, else two short of the shape so that the pad band exists."""
    c = case(name)
    b, n, m = shape(c)
    i = c["inputs"]
    lists = [np.concatenate([p, [[-1, n], [0, 0]]], axis=1) if j == 0 else p for j, p in enumerate(c["pairs"])]
    kcap = max(p.shape[1] for p in lists) + 2
    packed = torch.zeros(b, 2, kcap, dtype=torch.int32)
    for j, p in enumerate(lists):
        packed[j, :, :p.shape[1]] = torch.from_numpy(np.asarray(p, dtype=np.int32))
    host = [(ctypes.c_int32 * b)(*v) for v in ([p.shape[1] for p in lists], [i.get("n_orig") or max(n - 2, 0)] * b, [i.get("m_orig") or max(m - 2, 0)] * b)]

    def body(mem):
        pairs = mem.place(packed, "in", "pairs")
        cls, neg = mem.place(torch.empty(b, n, m, dtype=torch.int8), "out", "cls"), mem.place(torch.empty(1, dtype=torch.int32), "out", "negative_pairs")
        mem.call(BINDING, "gtr_build_target", pairs, *host, b, kcap, n, m, int(i.get("pad_val", 0) == 0), cls, neg)
        return dict(cls=cls, negative_pairs=neg)

    got = run(body, DEV, ROLES)
    assert got["negative_pairs"].item() == 1 and set(got["cls"].unique().tolist()) <= {0, 1, 2}


@pytest.mark.parametrize("name", [BAND, "2x130x132"])
def test_a_cls_that_is_not_4_byte_aligned(name, run=run_placement):
    """m % 4 == 0: the aligned placement reads four classes per load, one byte further it must take the byte path -- same bits."""
    c = case(name)
    assert shape(c)[2] % 4 == 0
    aligned = run(head_body(c), DEV, ROLES)
    skewed = run(head_body(c, cls_skew=1), DEV, ROLES)
    for k in aligned:
        assert bitwise_equal(aligned[k], skewed[k]), k
    assert aligned["counts"][2] > 0


def test_foreign_class_values_count_as_ignored(run=run_placement):
    """The header: "any other value counts as ignored".  The ignored band rewritten with -128, -1, 3 and 127 mixed."""
    c = case(BAND)
    cls = c["cls"].clone()
    band = cls == 2
    assert band.sum() > 1000
    cls[band] = torch.tensor([-128, -1, 3, 127], dtype=torch.int8).repeat(int(band.sum()) // 4 + 1)[:int(band.sum())]
    assert not (cls == 2).any() and bool(((cls == 1) == (c["cls"] == 1)).all())
    want = run(head_body(c), DEV, ROLES)
    got = run(head_body(c, cls=cls), DEV, ROLES)
    for k in ("loss", "counts", "dx", "dy"):
        assert bitwise_equal(want[k], got[k]), k


# every case again with each library call captured in a graph and replayed (arena.run_captured): the stream contract
test_loss_head_captured = captured_twin(test_loss_head)
test_stage_entries_captured = captured_twin(test_stage_entries)
test_build_target_captured = captured_twin(test_build_target)
test_a_cls_that_is_not_4_byte_aligned_captured = captured_twin(test_a_cls_that_is_not_4_byte_aligned)
test_foreign_class_values_count_as_ignored_captured = captured_twin(test_foreign_class_values_count_as_ignored)
