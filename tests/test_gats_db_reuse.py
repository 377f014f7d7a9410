"""gatsspg_forward reuses the first-three-layer work of an unchanged database, on the MI355X.

The reference for "identical" is always gatsspg_forward with GATSSPG_FLAG_NO_DB_REUSE -- the plain chain -- on the same inputs;
the five outputs (conf, matches0 / 1, mscores0 / 1) are compared bitwise.  What a call did is read from the workspace's state block (its last
256 bytes, include/gatsspg.h) after a synchronise.

Shapes.  The reusing path is taken by frames of more than 64 column tiles, b * (round_up(n1, 128) + round_up(n2, 128)) / 64 > 64
(db_reuse_shape: SMALL_NT3 = DIET_MIN_TILES = 64), and a side is padded to 128 columns = 2 tiles.  b = 1: the smallest such frame
has 66 tiles, n1 <= 128 with 3969 <= n2 <= 4096: (100, 4000).  Its windows are 2 and 64 tiles, so left to themselves they would
take the OTHER fp32 mlp.3 tile (Mlp3TileS) than the frame (Mlp3TileTallW8): the case that made the explicit database cache differ
from the plain forward (tests/test_gats_stage_edges.py::test_database_cache_at_form_edges).  b = 2: 2 * 34 = 68 tiles, (100, 2000).
The fp16 arithmetics have their own form threshold (the 128-column mlp.0 tile at 96..128 tiles): (100, 6000) is 96 tiles, its 3D
window 94.  Below the threshold: (100, 3900) is 64 tiles.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import gatsspg_oracle as orc
from onepose_amd import GATsSuperGlue, _native, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HP = dict(orc.DEFAULT_HPARAMS, match_threshold=0.0)
LEAF = 8
N1, N2 = 100, 4000            # 66 tiles: the smallest b = 1 frame of the reusing path
N2_B2 = 2000                  # b = 2: 68 tiles
N2_FP16 = 6000                # 96 tiles: the fp16 modes' 128-column mlp.0 tile, 3D window on the 64-column one if left alone
N2_BELOW = 3900               # 64 tiles: the plain chain
WORDS = dict(magic=0, b=1, n1p=2, n2=3, num_leaf=4, flags=5, fingerprint=6, snapshot_valid=7, miss=8, strike=9, hit=10, copy=11)
PRECISIONS = ["fp32", "bf16x3", "bf16x6", "fp16x3", "fp16x4"]


def tiles(b, n1, n2):
    up = lambda n: (n + 127) // 128 * 128
    return b * (up(n1) + up(n2)) // 64


def test_the_shapes_are_the_edges_the_docstring_names():
    assert tiles(1, N1, N2) == 66 and tiles(1, 128, 3968) == 64 and tiles(2, N1, N2_B2) == 68 and tiles(2, 128, 1920) == 64
    assert tiles(1, N1, N2_FP16) == 96 and tiles(1, N1, N2_BELOW) == 64
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gatsspg.h")).read()
    assert int(re.search(r"^#define GATSSPG_FLAG_NO_DB_REUSE\s+(0x[0-9a-fA-F]+)", header, flags=re.M).group(1), 0) == _native.FLAG_NO_DB_REUSE
    lib = _native.load()
    assert lib.gatsspg_version() >= 413
    # a workspace with an area holds the database a second time, the cache twice and 17 MB of weights; without one it is smaller than the database
    for b, n2, has in ((1, N2, True), (2, N2_B2, True), (1, N2_FP16, True), (1, N2_BELOW, False), (1, 3968, False)):
        database = 4 * b * 256 * n2 * (1 + LEAF)
        assert (lib.gatsspg_workspace_bytes(b, N1, n2, LEAF) > 2 * database) == has, (b, n2)


@functools.lru_cache(maxsize=None)
def model(precision):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    m = GATsSuperGlue(HP, precision=precision).eval()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synthetic.make_state_dict(3).items()}, strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def inputs(b, n1, n2, seed):
    """(query, desc3d_db, desc2d_db) on the device; treated as read-only (a test that modifies a database clones it first)."""
    d = synthetic.make_inputs(b, n1, n2, LEAF, seed=seed)
    return tuple(torch.from_numpy(np.ascontiguousarray(d[k])).to(DEV) for k in ("descriptors2d_query", "descriptors3d_db", "descriptors2d_db"))


class Slot:
    """A workspace and its outputs for one shape, straight on the C ABI."""

    def __init__(self, b, n1, n2, precision="fp32", stream=None, extra=0):
        self.lib = _native.load()
        self.b, self.n1, self.n2 = b, n1, n2
        self.nbytes = self.lib.gatsspg_workspace_bytes(b, n1, n2, LEAF)
        self.ws = torch.zeros(self.nbytes + extra, device=DEV, dtype=torch.uint8)
        self.off = self.nbytes - 256 if tiles(b, n1, n2) > 64 else 0      # the state block: the last piece of a workspace with a reuse area
        self.stream = stream
        self.set_precision(precision)

    def set_precision(self, precision):
        eng = model(precision).engine
        self.packed, self.flags = eng.packed_weights(DEV), eng.flags()
        assert not self.flags & _native.FLAG_NO_DB_REUSE, "engine.flags() never sets the flag"

    def forward(self, q, d3, d2db, flags=None, packed=None, ws=None):
        b, n1, n2 = self.b, self.n1, self.n2
        out = (torch.empty(b, n1, n2, device=DEV), torch.empty(b, n1, device=DEV, dtype=torch.int64), torch.empty(b, n2, device=DEV, dtype=torch.int64),
               torch.empty(b, n1, device=DEV), torch.empty(b, n2, device=DEV))
        st = (self.stream or torch.cuda.current_stream(DEV)).cuda_stream
        ws = self.ws if ws is None else ws
        _native.check(self.lib.gatsspg_forward((self.packed if packed is None else packed).data_ptr(), q.data_ptr(), d3.data_ptr(), d2db.data_ptr(), b, n1, n2,
                                               LEAF, self.flags if flags is None else flags, 0.07, 0.0, *(o.data_ptr() for o in out), ws.data_ptr(),
                                               self.nbytes, st), "gatsspg_forward")
        return out

    def reference(self, q, d3, d2db, packed=None):
        """The plain chain on a workspace of its own."""
        ws = torch.empty(self.nbytes, device=DEV, dtype=torch.uint8)
        return self.forward(q, d3, d2db, flags=self.flags | _native.FLAG_NO_DB_REUSE, packed=packed, ws=ws)

    def word(self, name):
        torch.cuda.synchronize(DEV)
        return int(self.ws[self.off: self.off + 64].view(torch.int32)[WORDS[name]])

    def state_bytes(self):
        torch.cuda.synchronize(DEV)
        return self.ws[self.off: self.off + 64].clone()


def same(got, ref, what):
    torch.cuda.synchronize(DEV)
    for name, g, r in zip(("conf", "matches0", "matches1", "mscores0", "mscores1"), got, ref):
        g, r = (g.view(torch.int32), r.view(torch.int32)) if g.dtype == torch.float32 else (g, r)
        assert torch.equal(g, r), f"{what}: {name} differs from the plain chain in {int((g != r).sum())} entries"
    assert int((got[1] >= 0).sum()) > 0, f"{what}: no match at all"


def queries(b, n1, n2, count):
    return [inputs(b, n1, n2, 100 + i)[0] for i in range(count)]


def warm(slot, d3, d2db, q):
    """Two misses, then a hit: the state of a workspace that has seen one database for a while."""
    for _ in range(3):
        slot.forward(q, d3, d2db)
    assert slot.word("hit") == 1 and slot.word("snapshot_valid") == 1


# ---------------------------------------------------------------------------------------------------------------------
# 1. three calls with one database and three query frames: miss, miss, hit; all identical to the plain chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n2", [(p, N2) for p in PRECISIONS] + [("fp16x4", N2_FP16), ("fp16x3", N2_FP16)])
def test_third_call_on_one_database_hits_and_all_are_identical(precision, n2):
    _, d3, d2db = inputs(1, N1, n2, 7)
    slot = Slot(1, N1, n2, precision)
    seen = []
    for i, q in enumerate(queries(1, N1, n2, 3)):
        got = slot.forward(q, d3, d2db)
        seen.append((slot.word("hit"), slot.word("miss"), slot.word("strike"), slot.word("snapshot_valid")))
        same(got, slot.reference(q, d3, d2db), f"{precision} call {i + 1}")
    assert seen == [(0, 0, 0, 0), (0, 0, 1, 1), (1, 0, 1, 1)], seen      # (the miss word is cleared again by the end of every call)
    assert slot.word("magic") != 0 and (slot.word("b"), slot.word("n1p"), slot.word("n2"), slot.word("num_leaf")) == (1, 128, n2, LEAF)


def test_flags_of_the_linear_transform_path_hit_and_are_identical():
    """with_linear_transform / additional: the GATs layer of the prepare chain is two launches (aggregate, W^T + elu), both gated."""
    hp = dict(HP, with_linear_transform=True, additional=True)
    m = GATsSuperGlue(hp).eval()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synthetic.make_state_dict(3).items()}, strict=True)
    m.to(DEV)
    slot = Slot(1, N1, N2)
    slot.packed, slot.flags = m.engine.packed_weights(DEV), m.engine.flags()
    assert slot.flags & _native.FLAG_WITH_LINEAR_TRANSFORM
    _, d3, d2db = inputs(1, N1, N2, 7)
    for i, q in enumerate(queries(1, N1, N2, 3)):
        same(slot.forward(q, d3, d2db), slot.reference(q, d3, d2db), f"linear transform, call {i + 1}")
    assert slot.word("hit") == 1


# ---------------------------------------------------------------------------------------------------------------------
# 2. a change of the database or of the weights, in place, is caught
# ---------------------------------------------------------------------------------------------------------------------
def flip_one_bit(t, index):
    v = t.view(-1).view(torch.int32)
    v[index] ^= 1 << 20          # a mantissa bit of one element


def test_one_flipped_bit_in_database_or_weights_is_a_miss():
    q, d3, d2db = (t.clone() for t in inputs(1, N1, N2, 7))
    slot = Slot(1, N1, N2)
    packed = slot.packed.clone()
    warm(slot, d3, d2db, q)
    big = 768 * 256 + 512 * 512 + 256 * 512
    layer = big + 768 + 512 + 256 + 8                    # floats of one attention layer's block (gatsspg_common.h AttnW::SIZE)
    targets = (("desc2d_db", d2db, d2db.numel() - 12345), ("desc3d_db", d3, 54321),
               ("mlp.3 weight of attention layer 1", packed, layer + 768 * 256 + 768 + 512 * 512 + 512 + 1000))
    for what, t, index in targets:
        flip_one_bit(t, index)
        got = slot.forward(q, d3, d2db, packed=packed)
        assert (slot.word("hit"), slot.word("miss")) == (0, 0), what
        same(got, slot.reference(q, d3, d2db, packed=packed), f"after a bit of {what} flipped")
        # the sample of the fingerprint does not hold the flipped word: a second strike at once, the next call hits again
        got = slot.forward(q, d3, d2db, packed=packed)
        assert slot.word("hit") == 1, f"the call after the miss on {what}"
        same(got, slot.reference(q, d3, d2db, packed=packed), f"hit after a bit of {what} flipped")


# ---------------------------------------------------------------------------------------------------------------------
# 3. overwriting the workspace is harmless
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_overwritten_workspace_misses_and_is_identical(fill):
    q, d3, d2db = inputs(1, N1, N2, 7)
    slot = Slot(1, N1, N2)
    warm(slot, d3, d2db, q)
    slot.ws.fill_(fill)               # 0xFF: every float a NaN, every word of the state -1
    got = slot.forward(q, d3, d2db)
    assert (slot.word("hit"), slot.word("miss"), slot.word("snapshot_valid")) == (0, 0, 0)
    same(got, slot.reference(q, d3, d2db), f"after filling the workspace with {fill:#x}")
    slot.forward(q, d3, d2db)
    got = slot.forward(q, d3, d2db)
    assert slot.word("hit") == 1
    same(got, slot.reference(q, d3, d2db), "hit after the refill")


def test_overwritten_cache_alone_is_a_miss():
    """Only the cache (the head of the reuse area) is scribbled on, snapshot and state stay: what a call of another shape on the same
    memory does.  The cache is compared with its second copy."""
    q, d3, d2db = inputs(1, N1, N2, 7)
    slot = Slot(1, N1, N2)
    warm(slot, d3, d2db, q)
    # the area, from its end (gatsspg_common.h: cache | snapshot pieces 0..6 | cache copy | state, every piece on 256 bytes)
    up = lambda n: (n + 255) // 256 * 256
    plane, big = 4 * 256 * N2, 768 * 256 + 512 * 512 + 256 * 512
    copy = up(2 * plane + 4 * 4 * (64 * 64 + 64 + 8))
    snapshot = up(plane) + up(plane * LEAF) + up(4 * (512 + 256 * 256)) + 2 * up(4 * (big + 768 + 512 + 256 + 8)) + 2 * up(2 * 5 * big)
    cache_off = slot.off - copy - snapshot - up(slot.lib.gatsspg_db_cache_bytes(1, N2))
    assert cache_off > slot.lib.gatsspg_workspace_bytes(1, N1, N2_BELOW, LEAF)     # behind the plain workspace of a smaller shape without an area
    torch.cuda.synchronize(DEV)
    assert torch.equal(slot.ws[cache_off: cache_off + 2 * plane], slot.ws[slot.off - copy: slot.off - copy + 2 * plane]), "the layout this test assumes"
    slot.ws[cache_off + plane + 4 * 77777] ^= 1            # one bit of one element of the cached 3D-side Q
    got = slot.forward(q, d3, d2db)
    assert (slot.word("hit"), slot.word("miss")) == (0, 0)
    same(got, slot.reference(q, d3, d2db), "after the cache was written to")


# ---------------------------------------------------------------------------------------------------------------------
# 4. each workspace keeps its own state
# ---------------------------------------------------------------------------------------------------------------------
def test_two_workspaces_on_two_streams_with_two_databases():
    qa, d3a, d2a = inputs(1, N1, N2, 7)
    qb, d3b, d2b = inputs(1, N1, N2, 8)
    torch.cuda.synchronize(DEV)
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    a, b = Slot(1, N1, N2, stream=sa), Slot(1, N1, N2, stream=sb)
    for _ in range(3):
        ga, gb = a.forward(qa, d3a, d2a), b.forward(qb, d3b, d2b)
    assert a.word("hit") == 1 and b.word("hit") == 1
    assert a.word("fingerprint") != b.word("fingerprint")
    same(ga, a.reference(qa, d3a, d2a), "workspace A")
    same(gb, b.reference(qb, d3b, d2b), "workspace B")


def test_one_workspace_alternating_between_two_databases_never_hits():
    qa, d3a, d2a = inputs(1, N1, N2, 7)
    qb, d3b, d2b = inputs(1, N1, N2, 8)
    slot = Slot(1, N1, N2)
    for i in range(6):
        q, d3, d2 = (qa, d3a, d2a) if i % 2 == 0 else (qb, d3b, d2b)
        got = slot.forward(q, d3, d2)
        assert (slot.word("hit"), slot.word("strike"), slot.word("snapshot_valid")) == (0, 0, 0), f"call {i + 1}"
        same(got, slot.reference(q, d3, d2), f"alternating, call {i + 1}")


def test_batch_of_two_samples_with_different_databases():
    a, b = inputs(1, N1, N2_B2, 7), inputs(1, N1, N2_B2, 8)
    q, d3, d2 = (torch.cat([x, y]).contiguous() for x, y in zip(a, b))
    slot = Slot(2, N1, N2_B2)
    for i in range(3):
        same(slot.forward(q, d3, d2), slot.reference(q, d3, d2), f"b = 2, call {i + 1}")
    assert slot.word("hit") == 1
    d3 = d3.clone()
    flip_one_bit(d3, d3.numel() - 7)              # the SECOND sample's database
    got = slot.forward(q, d3, d2)
    assert (slot.word("hit"), slot.word("miss")) == (0, 0)
    same(got, slot.reference(q, d3, d2), "b = 2 after a bit of sample 1's database flipped")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the stamp separates call shapes and flags
# ---------------------------------------------------------------------------------------------------------------------
def test_another_shape_or_precision_on_the_same_memory_in_between_is_a_miss():
    q, d3, d2db = inputs(1, N1, N2, 7)
    slot = Slot(1, N1, N2)
    warm(slot, d3, d2db, q)
    # the same memory under another n2: its reuse area lies elsewhere and overlaps this one
    n2o = N2 + 90
    other = Slot(1, N1, n2o)
    assert other.nbytes > slot.nbytes and other.off != slot.off
    big = torch.zeros(other.nbytes, device=DEV, dtype=torch.uint8)
    big[: slot.nbytes] = slot.ws
    slot.ws = other.ws = big
    qo, d3o, d2o = inputs(1, N1, n2o, 9)
    for i in range(3):
        same(other.forward(qo, d3o, d2o), other.reference(qo, d3o, d2o), f"the other shape, call {i + 1}")
    got = slot.forward(q, d3, d2db)
    assert (slot.word("hit"), slot.word("miss")) == (0, 0), "back on the first shape"
    same(got, slot.reference(q, d3, d2db), "back on the first shape")
    warm(slot, d3, d2db, q)
    # another arithmetic on the same shape: the same state block, another stamp
    slot.set_precision("bf16x6")
    got = slot.forward(q, d3, d2db)
    assert (slot.word("hit"), slot.word("miss"), slot.word("strike")) == (0, 0, 0)
    same(got, slot.reference(q, d3, d2db), "bf16x6 in between")
    slot.set_precision("fp32")
    got = slot.forward(q, d3, d2db)
    assert (slot.word("hit"), slot.word("miss")) == (0, 0), "back in fp32"
    same(got, slot.reference(q, d3, d2db), "back in fp32")


# ---------------------------------------------------------------------------------------------------------------------
# 6. below the thresholds the plain chain runs
# ---------------------------------------------------------------------------------------------------------------------
def test_below_the_thresholds_nothing_is_kept():
    q, d3, d2db = inputs(1, N1, N2_BELOW, 7)
    probe = Slot(1, N1, N2)                        # how large an area would be, had the shape one
    slot = Slot(1, N1, N2_BELOW, extra=probe.nbytes)
    assert slot.off == 0
    slot.ws[slot.nbytes:].fill_(0xA5)
    for i in range(3):
        same(slot.forward(q, d3, d2db), slot.reference(q, d3, d2db), f"64 tiles, call {i + 1}")
    torch.cuda.synchronize(DEV)
    assert bool((slot.ws[slot.nbytes:] == 0xA5).all()), "bytes behind the plain workspace were written"


def test_the_flag_leaves_the_state_block_alone():
    q, d3, d2db = inputs(1, N1, N2, 7)
    slot = Slot(1, N1, N2)
    slot.ws[slot.off: slot.off + 64].fill_(0x5A)
    before = slot.state_bytes()
    for _ in range(3):
        slot.forward(q, d3, d2db, flags=slot.flags | _native.FLAG_NO_DB_REUSE)
    assert torch.equal(slot.state_bytes(), before)


# ---------------------------------------------------------------------------------------------------------------------
# 7. gatsspg_forward_profiled takes the plain chain
# ---------------------------------------------------------------------------------------------------------------------
def test_profiled_forward_takes_the_plain_chain():
    """Launch #0 of mlp0 is the whole frame's (66 tiles) on the plain chain and the query window's (2 tiles) on the cached one.  The
    state block is not touched, the outputs are the plain chain's, and the bracketed launch takes the time of the 66-tile launch: more
    than half of what the same bracket measures under GATSSPG_FLAG_NO_DB_REUSE (a 2-tile launch is 8 of its 264 workgroups)."""
    q, d3, d2db = inputs(1, N1, N2, 7)
    slot = Slot(1, N1, N2)
    warm(slot, d3, d2db, q)
    before = slot.state_bytes()
    out = (torch.empty(1, N1, N2, device=DEV), torch.empty(1, N1, device=DEV, dtype=torch.int64), torch.empty(1, N2, device=DEV, dtype=torch.int64),
           torch.empty(1, N1, device=DEV), torch.empty(1, N2, device=DEV))

    def timed(flags):
        best = float("inf")
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()           # (a torch event has no handle before its first record)
            e1.record()
            _native.check(slot.lib.gatsspg_forward_profiled(
                slot.packed.data_ptr(), q.data_ptr(), d3.data_ptr(), d2db.data_ptr(), 1, N1, N2, LEAF, flags, 0.07, 0.0, *(o.data_ptr() for o in out),
                slot.ws.data_ptr(), slot.nbytes, torch.cuda.current_stream(DEV).cuda_stream, _native.KERNEL_IDS["mlp0"], 0, e0.cuda_event, e1.cuda_event),
                "gatsspg_forward_profiled")
            torch.cuda.synchronize(DEV)
            best = min(best, e0.elapsed_time(e1))
        return best

    t_default = timed(slot.flags)
    same(out, slot.reference(q, d3, d2db), "profiled forward")
    assert torch.equal(slot.state_bytes(), before), "the profiled forward wrote the state block"
    t_plain = timed(slot.flags | _native.FLAG_NO_DB_REUSE)
    print(f"\nmlp0 launch #0, event-timed: default flags {t_default * 1e3:.1f} us, plain chain {t_plain * 1e3:.1f} us")
    assert t_default > 0.5 * t_plain
