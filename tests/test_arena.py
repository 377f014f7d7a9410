"""The guard-band helper (tests/arena.py) on the CPU: its layout, and that the detector detects.  Small torch-on-CPU stand-ins for a
library call -- a correct one, one that writes one byte behind an output, one that writes one element before the workspace, one that
modifies an input, one whose result reads a guard byte -- are driven through the arena; the first passes, each of the others is
reported with the right piece and offset.  Then the ROLES table of every placement test module against the ``const`` of the header
prototypes.  No GPU: nothing here launches anything."""
import importlib

import pytest
import torch

import arena
from arena import Arena, GuardViolation, run_placement

CPU = torch.device("cpu")
SMALL = dict(guard=4096, capacity=2 << 20)           # the stand-ins move a few bytes: a small arena keeps this file quick
N = 37                                               # floats: 148 bytes, no multiple of anything
PLACEMENT_MODULES = ["test_placement_train", "test_placement_gats", "test_placement_spp", "test_placement_sg", "test_placement_det",
                     "test_placement_map", "test_placement_trk", "test_placement_pnp"]


def beyond(t, first, count):
    """``count`` elements of ``t``'s storage starting ``first`` elements from its start (negative: before it): how a stand-in steps
    outside the buffer it was given"""
    return torch.as_strided(t, (count,), (1,), t.storage_offset() + first)


def correct(x, out, ws):
    ws.copy_(x)
    out.copy_(ws * 2)


def writes_behind_output(x, out, ws):
    correct(x, out, ws)
    beyond(out.view(torch.uint8), out.numel() * 4, 1).fill_(7)


def writes_before_workspace(x, out, ws):
    correct(x, out, ws)
    beyond(ws, -1, 1).fill_(1.0)


def modifies_input(x, out, ws):
    correct(x, out, ws)
    x[5] += 1


def reads_guard(x, out, ws):
    correct(x, out, ws)
    out[N - 1] += beyond(x.view(torch.uint8), N * 4, 1)[0].float()      # the byte behind the input


def placed(fn, fill=0xFF):
    """``fn`` on pieces of a fresh arena, between snapshot() and check()"""
    a = Arena(CPU, fill=fill, **SMALL)
    x = a.place(torch.arange(N, dtype=torch.float32), "in", "x")
    out = a.place(torch.empty(N), "out", "out")
    ws = a.place(torch.empty(N), "scratch", "workspace")
    a.snapshot()
    fn(x, out, ws)
    a.check()
    return out


def body_of(fn):
    def body(mem):
        x = mem.place(torch.arange(N, dtype=torch.float32), "in", "x")
        out = mem.place(torch.empty(N), "out", "out")
        ws = mem.place(torch.empty(N), "scratch", "workspace")
        mem.guarded(lambda: fn(x, out, ws), [out, ws])
        return {"out": out}
    return body


def test_layout():
    a = Arena(CPU, guard=4096, fill=0xAB, capacity=2 << 20)
    assert bool((a.buf == 0xAB).all())
    t = torch.arange(15, dtype=torch.float64).reshape(3, 5)
    views = [a.place(t, "in", "t"), a.place(7, "scratch"), a.place(torch.empty(301, dtype=torch.int32), "out"), a.place(torch.arange(40, dtype=torch.int8), "in", skew=1)]
    assert torch.equal(views[0], t) and views[0].dtype == torch.float64 and views[0].shape == (3, 5)
    assert views[1].dtype == torch.uint8 and views[1].numel() == 7 and bool((views[1] == 0xAB).all())
    assert bool((views[2] == torch.tensor(0xABABABAB - (1 << 32), dtype=torch.int64)).all())       # an output keeps the fill
    for v, p, skew in zip(views, a.pieces, (0, 0, 0, 1)):
        assert v.is_contiguous() and v.data_ptr() % 256 == skew and p.nbytes == v.numel() * v.element_size()
    assert [p.nbytes for p in a.pieces] == [120, 7, 1204, 40] and a.pieces[0].name == "t" and a.pieces[1].name == "piece1"
    assert a.pieces[0].start - a.base >= 4096
    for p, q in zip(a.pieces, a.pieces[1:]):
        assert 4096 <= q.start - p.end < 4096 + 256 + 1
    assert a.buf.numel() - a.pieces[-1].end >= 4096 + (1 << 20)
    with pytest.raises(MemoryError):
        a.place(1 << 20, "scratch")


def test_a_correct_call_passes():
    out = placed(correct)
    assert torch.equal(out, 2 * torch.arange(N, dtype=torch.float32))
    got = run_placement(body_of(correct), CPU, **SMALL)
    assert torch.equal(got["out"], out)


def test_one_byte_behind_an_output_is_reported():
    with pytest.raises(GuardViolation, match=rf"1 byte\(s\) changed behind piece 'out' \({N * 4} bytes\): offsets {N * 4} \.\. {N * 4} "):
        placed(writes_behind_output)
    with pytest.raises(GuardViolation, match="behind piece 'out'"):
        placed(writes_behind_output, fill=0x00)
    with pytest.raises(GuardViolation, match="behind piece 'out'"):
        run_placement(body_of(writes_behind_output), CPU, **SMALL)


def test_one_element_before_the_workspace_is_reported():
    # 1.0f is 00 00 80 3f: under the fill 0xFF all four bytes change, under 0x00 the upper two
    with pytest.raises(GuardViolation, match=r"4 byte\(s\) changed before piece 'workspace': offsets -4 \.\. -1 "):
        placed(writes_before_workspace)
    with pytest.raises(GuardViolation, match=r"2 byte\(s\) changed before piece 'workspace': offsets -2 \.\. -1 "):
        placed(writes_before_workspace, fill=0x00)


def test_a_modified_input_is_reported():
    # 5.0f -> 6.0f: 0x40a00000 -> 0x40c00000, one byte
    with pytest.raises(GuardViolation, match=r"1 byte\(s\) changed inside in piece 'x', which this call may not write: offsets 22 \.\. 22 "):
        placed(modifies_input)


def test_a_piece_the_call_was_not_given_is_protected():
    a = Arena(CPU, **SMALL)
    x = a.place(torch.zeros(4), "in", "x")
    blob = a.place(64, "scratch", "blob")
    out = a.place(torch.empty(4), "out", "out")
    a.snapshot()
    blob.fill_(1)
    out.fill_(1)
    a.check()                                          # by default a scratch piece is writable ...
    a.snapshot()
    blob[63] = 2
    with pytest.raises(GuardViolation, match=r"inside scratch piece 'blob'.*offsets 63 \.\. 63 "):
        a.check([out])                                 # ... but not in a call that takes it as const
    assert x.sum() == 0


def test_a_result_that_reads_a_guard_byte_is_reported():
    """check() cannot see a read: both runs of one pattern read that pattern.  The two patterns give different results."""
    assert placed(reads_guard)[N - 1] == 2 * (N - 1) + 255 and placed(reads_guard, fill=0)[N - 1] == 2 * (N - 1)
    # 72.0f against 327.0f: three bytes of the last element (bytes 144 .. 147) differ
    with pytest.raises(AssertionError, match=r"out: the result depends on the fill pattern \(3 byte\(s\), the first at byte 145, the last at byte 147\)"):
        run_placement(body_of(reads_guard), CPU, **SMALL)


def test_rows_the_header_calls_unwritten_are_compared_per_pattern_only():
    def body(mem):
        out = mem.place(torch.empty(8, dtype=torch.int32), "out", "out")
        mem.guarded(lambda: out[:5].fill_(3), [out])
        return {"out": out}, {"out": out[:5]}
    got = run_placement(body, CPU, **SMALL)
    assert got["out"].tolist() == [3] * 5 + [-1] * 3
    with pytest.raises(AssertionError, match="depends on the fill pattern"):
        run_placement(lambda mem: body(mem)[0], CPU, **SMALL)


def test_the_header_parser_keeps_const():
    p = arena.parameters("gtr_loss_head")
    assert [(q[2], q[3]) for q in p[:3]] == [("x", True), ("y", True), ("cls", True)] and p[2][0] == "int8_t"
    assert [(q[2], q[3]) for q in p if q[2] in ("loss", "dx", "workspace")] == [("loss", False), ("dx", False), ("workspace", False)]
    assert arena.parameters("gtr_version") == [] and len(arena.parameters("gatsspg_forward_profiled")) == 23


@pytest.mark.parametrize("module", PLACEMENT_MODULES)
def test_declared_roles_agree_with_the_const_of_the_prototypes(module):
    mod = importlib.import_module(module)
    assert mod.ROLES, module
    arena.check_roles(mod.BINDING, mod.ROLES)


def test_check_roles_refuses_a_wrong_or_missing_role():
    from onepose_amd import _native_train
    good = dict(x="in", y="in", E="out", r="out", c="out", workspace="scratch")
    arena.check_roles(_native_train, {"gtr_scores_exp": good})
    with pytest.raises(AssertionError, match="const float\\* y is declared 'out'"):
        arena.check_roles(_native_train, {"gtr_scores_exp": dict(good, y="out")})
    with pytest.raises(AssertionError, match="float\\* E is declared 'in'"):
        arena.check_roles(_native_train, {"gtr_scores_exp": dict(good, E="in")})
    with pytest.raises(AssertionError, match="roles declared for"):
        arena.check_roles(_native_train, {"gtr_scores_exp": {k: v for k, v in good.items() if k != "r"}})
