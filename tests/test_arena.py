"""The guard-band helper (tests/arena.py) on the CPU: its layout, and that the detector detects.  Small torch-on-CPU stand-ins for a
library call -- a correct one, one that writes one byte behind an output, one that writes one element before the workspace, one that
modifies an input, one whose result reads a guard byte -- are driven through the arena; the first passes, each of the others is
reported with the right piece and offset.  Then the ROLES table of every placement test module against the ``const`` of the header
prototypes.  Then the captured mode (``run_captured``): the stand-ins enqueue their writes on ``arena.HostGraph`` as a library call
enqueues kernels, and one that writes while it is recorded, one that updates an argument in place, one that modifies an input, one that
enqueues nothing and one that raises are each answered as the stream contract says.  Last, every function the headers declare with a
stream parameter has a captured case or a reason in ``arena.NOT_CAPTURED``.  No GPU: nothing here launches anything."""
import importlib

import pytest
import torch

import arena
from arena import Arena, CaptureFailure, GuardViolation, HostGraph, run_captured, run_placement

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
        mem.guarded(lambda: fn(x, out, ws), [out, ws], inputs=[x], name=fn.__name__)
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


# ---- the captured mode: stand-ins that enqueue their writes, as a library call enqueues kernels on its stream ----
def enqueued(fn):
    def call(*tensors):
        HostGraph.enqueue(lambda: fn(*tensors))
    call.__name__ = fn.__name__
    return call


def strays_from_the_stream(x, out, ws):
    """the first five elements are written when the call is made, not when its stream runs: a launch on another stream"""
    out[:5].copy_(2 * x[:5])
    HostGraph.enqueue(lambda: (ws.copy_(x), out[5:].copy_(ws[5:] * 2)))


def test_a_correct_call_passes_captured():
    got = run_captured(body_of(enqueued(correct)), CPU, **SMALL)
    assert arena.bitwise_equal(got["out"], run_placement(body_of(correct), CPU, **SMALL)["out"])
    assert torch.equal(got["out"], 2 * torch.arange(N, dtype=torch.float32))
    assert HostGraph.capturing is None


def test_a_write_made_while_the_call_is_recorded_is_reported():
    """the plain run is right (outside a capture every launch runs at once); the replay lacks the five elements: they hold the fill"""
    assert torch.equal(run_placement(body_of(strays_from_the_stream), CPU, **SMALL)["out"], 2 * torch.arange(N, dtype=torch.float32))
    with pytest.raises(AssertionError, match=r"out: the captured run differs from the plain run under fill 0xff in 20 byte\(s\), the first at "
                                             r"byte 0, the last at byte 19"):
        run_captured(body_of(strays_from_the_stream), CPU)


def in_place_body(fn):
    def body(mem):
        x = mem.place(torch.arange(N, dtype=torch.float32), "out", "x", copy=True)
        mem.guarded(lambda: fn(x), [x], name="add_one")
        return {"x": x}
    return body


def test_an_argument_updated_in_place_is_replayed_from_its_start_value():
    """x += 1 once per replay, each replay from x0: x0 + 1, not x0 + 2 (no restore) or x0 + 3 (the capture ran it as well)"""
    got = run_captured(in_place_body(lambda x: HostGraph.enqueue(lambda: x.add_(1))), CPU)
    assert torch.equal(got["x"], torch.arange(N, dtype=torch.float32) + 1)
    with pytest.raises(CaptureFailure, match="add_one: the captured graph is empty"):        # done at once: nothing was enqueued
        run_captured(in_place_body(lambda x: x.add_(1)), CPU)


def test_a_modified_input_is_reported_captured():
    with pytest.raises(AssertionError, match=r"modifies_input inputs\[0\]: an input was modified \(1 byte\(s\), the first at byte 22, the last at byte 22\)"):
        run_captured(body_of(enqueued(modifies_input)), CPU)


def test_replays_that_differ_are_reported():
    """state kept outside the pieces: the second replay writes something else"""
    runs = []

    def counts_its_runs(x, out, ws):
        HostGraph.enqueue(lambda: (runs.append(0), correct(x, out, ws), out[3].fill_(len(runs) % 2)))
    with pytest.raises(AssertionError, match=r"counts_its_runs writable\[0\]: two replays from the same contents differ in \d byte\(s\), the first at byte 1[2-5]"):
        run_captured(body_of(counts_its_runs), CPU)


def test_an_empty_graph_and_a_failed_capture():
    def nothing(x, out, ws):
        pass

    def refuses(x, out, ws):
        """as a call that allocates: fine on a stream of its own, an error while the stream is captured"""
        if HostGraph.capturing is not None:
            raise RuntimeError("operation not permitted when stream is capturing")
        out.fill_(1)

    def empty_body(fn, empty_ok):
        def body(mem):
            out = mem.place(torch.zeros(N), "out", "out", copy=True)
            mem.guarded(lambda: fn(None, out, None), [out], name=fn.__name__, empty_ok=empty_ok)
            return {"out": out}
        return body
    with pytest.raises(CaptureFailure, match="nothing: the captured graph is empty"):
        run_captured(empty_body(nothing, None), CPU)
    assert not run_captured(empty_body(nothing, "n = 0 enqueues nothing"), CPU)["out"].any()
    def fills(x, out, ws):
        HostGraph.enqueue(lambda: out.fill_(1))
    with pytest.raises(CaptureFailure, match=r"fills: the call enqueued work, but its call site says that it enqueues nothing \(n = 0"):
        run_captured(empty_body(fills, "n = 0 enqueues nothing"), CPU)
    with pytest.raises(CaptureFailure, match="refuses could not be captured.*RuntimeError: operation not permitted when stream is capturing"):
        run_captured(empty_body(refuses, None), CPU)
    assert HostGraph.capturing is None


def test_rows_the_header_calls_unwritten_are_compared_per_pattern_only_captured():
    def body(mem):
        out = mem.place(torch.empty(8, dtype=torch.int32), "out", "out")
        mem.guarded(lambda: HostGraph.enqueue(lambda: out[:5].fill_(3)), [out])
        return {"out": out}, {"out": out[:5]}
    got = run_captured(body, CPU)
    assert got["out"].tolist() == [3] * 5 + [-1] * 3
    with pytest.raises(AssertionError, match="depends on the fill pattern"):
        run_captured(lambda mem: body(mem)[0], CPU)


# ---- every stream-taking function of the headers: a captured case, or a reason ----
def covered_and_excused(streams, covered, excused):
    """the complaints of the completeness rule: [] when every name of ``streams`` is in exactly one of the two tables and ``excused``
    names nothing else"""
    bad = [f"{n} takes a stream and has neither a captured case nor a reason in NOT_CAPTURED" for n in streams if n not in covered and n not in excused]
    bad += [f"{n} has a captured case and a reason in NOT_CAPTURED" for n in streams if n in covered and n in excused]
    bad += [f"NOT_CAPTURED names {n}, which no header declares with a stream parameter" for n in excused if n not in streams]
    return bad


def roles_of_all_modules():
    return {name for module in PLACEMENT_MODULES for name in importlib.import_module(module).ROLES}


def test_every_entry_point_with_a_stream_is_captured_or_excused():
    streams, covered = arena.stream_functions(), roles_of_all_modules()
    assert len(streams) > 60 and "ba_solve" in streams and "pnp_workspace_bytes" not in streams
    assert covered_and_excused(streams, covered, arena.NOT_CAPTURED) == []
    allowed = ("stage entry for tests: enqueues a prefix or a slice of the launches of ", "records events by design")
    for name, reason in arena.NOT_CAPTURED.items():
        assert reason.startswith(allowed), (name, reason)
        if reason.startswith(allowed[0]):
            assert reason[len(allowed[0]):].split(",")[0] in covered, (name, reason)


def test_the_completeness_rule_complains():
    streams, covered = arena.stream_functions(), roles_of_all_modules()
    less = {k: v for k, v in arena.NOT_CAPTURED.items() if k != "sg_layer"}
    assert covered_and_excused(streams, covered, less) == ["sg_layer takes a stream and has neither a captured case nor a reason in NOT_CAPTURED"]
    assert covered_and_excused(streams + ["new_entry"], covered, arena.NOT_CAPTURED)[0].startswith("new_entry takes a stream")
    assert "has a captured case and a reason" in covered_and_excused(streams, covered, dict(arena.NOT_CAPTURED, ba_solve="x"))[0]
    assert "which no header declares" in covered_and_excused(streams, covered, dict(arena.NOT_CAPTURED, gone="x"))[0]
