"""Guard-band memory for the placement tests (tests/test_placement_*.py).  TEST INFRASTRUCTURE ONLY: a plain module the tests
import, never imported by the product.

``Arena`` hands out pieces of ONE uint8 tensor: every piece starts on a 256-byte boundary and is exactly as long as asked, with
``guard`` bytes between neighbours, before the first piece and behind the last, and at least 1 MiB of tail.  The whole tensor holds
``fill`` before anything is placed.  ``snapshot()`` just before a call and ``check()`` after it: every byte that is not inside a piece
the call may write (role "out" or "scratch") must be unchanged -- guards, tail, inputs and the pieces the call was not given.
64 KiB of guard is a condition, not a measurement: twice the largest block one workgroup here stores (a 128 x 64 fp32 tile, 32 KiB).

``run_placement(body, device, roles)`` is the rule of the placement tests: ``body(mem)`` makes the library calls of one case through
``mem.place`` / ``mem.call`` and returns its outputs; it is run on plain ``torch.empty`` buffers and in an arena, under the fill
patterns 0xFF (every float a NaN, every integer -1) and 0x00.  Per pattern the arena's outputs equal the plain run's bit for bit, and
what the call wrote is the same bits under both patterns.  No tolerance anywhere.

The role of a device pointer comes from the header: ``const T*`` is "in", ``T*`` is "out", or "scratch" for a workspace, a packed
blob or a cache that the call fills.  ``prototypes()`` is the header parser of tests/test_abi_tables.py, restated, keeping ``const``;
``check_roles`` holds a test module's ROLES table to it (tests/test_arena.py, no GPU).

``run_captured(body, device, roles)`` runs the same bodies against the other clause every header carries -- "work enqueued on
`stream`, no allocation, no synchronisation": in the arena run's place every single library call is captured in a graph of its own
on a side stream and replayed twice, each time from the contents its pieces had before the call.  A launch or memset sent to
stream 0, a host read of a device count and a lazy allocation give the right bits on the default stream; here the capture fails, or
the replay lacks what ran outside it.  ``NOT_CAPTURED`` names the stream-taking functions that have no case, and why."""
import functools
import glob
import inspect
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN = 256
TAIL = 1 << 20
ROLE_NAMES = ("in", "out", "scratch")
PATTERNS = (0xFF, 0x00)


class GuardViolation(AssertionError):
    pass


class Piece:
    def __init__(self, name, role, start, nbytes):
        self.name, self.role, self.start, self.nbytes = name, role, start, nbytes

    @property
    def end(self):
        return self.start + self.nbytes


def _bytes_of(t):
    """``t`` (contiguous) as a flat uint8 tensor over the same memory"""
    return t.reshape(-1).view(torch.uint8)


def bitwise_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes_of(a.contiguous()), _bytes_of(b.contiguous()))


class Arena:
    def __init__(self, device, guard=65536, fill=0xFF, capacity=64 << 20):
        self.device, self.guard, self.fill = torch.device(device), guard, fill
        self.buf = torch.full((capacity + ALIGN,), fill, dtype=torch.uint8, device=self.device)
        self.base = -self.buf.data_ptr() % ALIGN           # offset of the first 256-byte boundary
        self.cursor = self.base                            # end of the last piece (or the start of the arena)
        self.pieces = []
        self.by_address = {}
        self.snap = None

    def place(self, what, role, name=None, skew=0, copy=None):
        """A piece for ``what`` (a tensor: a contiguous typed view with its contents copied in; an int: that many bytes, uint8).
        "out" and "scratch" pieces keep the fill, unless ``copy``: an argument the header declares ``T*`` and the call updates.
        ``skew``: start that many bytes behind the 256-byte boundary (the one alignment stress of the placement tests; the guard
        before the piece is then ``skew`` bytes longer)."""
        assert role in ROLE_NAMES, role
        nbytes = what if isinstance(what, int) else what.numel() * what.element_size()
        start = -(-(self.cursor + self.guard - self.base) // ALIGN) * ALIGN + self.base + skew
        if start + nbytes + self.guard + TAIL > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes is too small for a piece of {nbytes} bytes at {start}")
        piece = Piece(name or f"piece{len(self.pieces)}", role, start, nbytes)
        self.pieces.append(piece)
        self.cursor = piece.end
        view = self.buf[start:start + nbytes]
        if not isinstance(what, int):
            view = view.view(what.dtype).view(what.shape)
            if role == "in" if copy is None else copy:
                view.copy_(what)
        assert view.is_contiguous() and (view.data_ptr() - skew) % ALIGN == 0
        self.by_address[view.data_ptr()] = piece
        return view

    def piece_of(self, tensor):
        return self.by_address[tensor.data_ptr()]

    def snapshot(self):
        self._sync()
        self.snap = self.buf.clone()

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def check(self, writable=None):
        """Synchronise and compare with the snapshot: one mask, one reduction on the device.  ``writable``: the pieces (or their
        tensors) the call may write; default: every "out" and "scratch" piece."""
        assert self.snap is not None, "check() without a snapshot()"
        self._sync()
        if writable is None:
            writable = [p for p in self.pieces if p.role != "in"]
        writable = [w if isinstance(w, Piece) else self.piece_of(w) for w in writable]
        changed = self.buf != self.snap
        for p in writable:
            changed[p.start:p.end] = False
        count = int(changed.sum().item())
        if count:
            raise GuardViolation(self._describe(changed.nonzero().reshape(-1).cpu().tolist(), writable))
        self.snap = None

    def _describe(self, offsets, writable):
        """Name every offending run of bytes by the piece it belongs to: inside a protected piece, or in the guard before /
        behind the nearest piece.  Offsets are relative to the start of that piece."""
        groups = {}
        for o in offsets:
            inside = next((p for p in self.pieces if p.start <= o < p.end), None)
            if inside is not None:
                key = (inside, "inside")
            else:
                before = min((p for p in self.pieces if p.start > o), key=lambda p: p.start - o, default=None)
                behind = min((p for p in self.pieces if p.end <= o), key=lambda p: o - p.end, default=None)
                if behind is None or (before is not None and before.start - o <= o - behind.end + 1):
                    key = (before, "before")
                else:
                    key = (behind, "behind")
            groups.setdefault(key, []).append(o - key[0].start)
        lines = []
        for (p, side), rel in groups.items():
            where = {"inside": f"inside {p.role} piece '{p.name}', which this call may not write",
                     "before": f"before piece '{p.name}'", "behind": f"behind piece '{p.name}' ({p.nbytes} bytes)"}[side]
            lines.append(f"{len(rel)} byte(s) changed {where}: offsets {min(rel)} .. {max(rel)} relative to the piece")
        return f"{len(offsets)} byte(s) outside the writable pieces changed; " + "; ".join(lines)


# ---- the header side: which pointer is const ----
def prototypes():
    """{name: [(type without const, stars, parameter name, is_const)]} of every function the headers under include/ declare."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "**", "*.h"), recursive=True)):
        with open(path) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
        for _, name, params in re.findall(r"([\w \*]+?)\b(\w+)\s*\(([^()]*)\)\s*;", text):
            plist = []
            for p in (q.strip() for q in params.split(",")):
                if p == "void":
                    continue
                words = re.findall(r"\w+|\*", p)
                pname = words.pop()
                plist.append((" ".join(w for w in words if w not in ("*", "const")), words.count("*"), pname, "const" in words))
            assert name not in out, f"{name} declared twice"
            out[name] = plist
    return out


_prototypes = None


def parameters(name):
    global _prototypes
    if _prototypes is None:
        _prototypes = prototypes()
    return _prototypes[name]


def check_roles(module, roles):
    """The ROLES table of a placement test module against the binding table and the headers: every device pointer of a covered
    entry point is declared, by its parameter name, and "in" is exactly ``const``."""
    from onepose_amd._binding import STREAM, DevicePointer
    symbols = {**module.SYMBOLS, **getattr(module, "MORE_SYMBOLS", {})}
    for name, declared in roles.items():
        params = parameters(name)
        table = symbols[name][1]
        assert len(table) == len(params), name
        device = {p[2] for p, entry in zip(params, table) if isinstance(entry, DevicePointer) and entry is not STREAM}
        assert set(declared) == device, f"{name}: roles declared for {sorted(declared)}, the device pointers are {sorted(device)}"
        for ctype, stars, pname, const in params:
            if pname in declared:
                role = declared[pname]
                assert role in ROLE_NAMES and stars >= 1, f"{name} {pname}: {role}"
                assert (role == "in") == const, f"{name}: {'const ' if const else ''}{ctype}{'*' * stars} {pname} is declared '{role}'"


# ---- which entry points take a stream, and which of them have no captured case ----
def stream_functions():
    """the names of the functions the headers declare with a stream parameter"""
    return sorted(name for name, params in prototypes().items() if any(p[2] == "stream" for p in params))


def _stage(of, *names):
    return {n: f"stage entry for tests: enqueues a prefix or a slice of the launches of {of}, which is covered" for n in names}


# Every function of stream_functions() is a key of some placement module's ROLES (and then runs captured as well as placed) or of this
# table (tests/test_arena.py holds the two to the headers).
NOT_CAPTURED = {
    **_stage("gatsspg_forward", "gatsspg_load_state", "gatsspg_store_state", "gatsspg_gats_layer", "gatsspg_attn_layer",
             "gatsspg_final_proj_norm", "gatsspg_score_dual_softmax_match"),
    **_stage("gatsspg_forward_frames", "gatsspg_gats_layer_frames"),
    **_stage("sg_forward", "sg_keypoint_encode", "sg_layer", "sg_attention", "sg_sinkhorn", "sg_match_tail"),
    **_stage("sg_forward_ragged", "sg_attention_ragged", "sg_sinkhorn_ragged", "sg_match_tail_ragged"),
    **_stage("pnp_ransac_epnp", "pnp_epnp", "pnp_hypotheses", "pnp_score_hypotheses", "pnp_select_best", "pnp_refit"),
    **_stage("spp_dense", "spp_dense_stage"),
    **_stage("flow_track", "flow_patch_sums", "flow_mismatch_sums"),
    "gatsspg_forward_profiled": "records events by design",
    "spp_forward_profiled": "records events by design",
}


# ---- the two kinds of memory a case body runs on, and the captured mode of the plain one ----
class CaptureFailure(AssertionError):
    pass


class HostGraph:
    """The CPU stand-in of a captured graph (tests/test_arena.py): while one is capturing, ``HostGraph.enqueue(launch)`` stores
    ``launch`` -- a stand-in library function enqueues its writes this way, as a library call enqueues kernels on the stream --
    and ``replay()`` runs what was stored, in order.  Outside a capture ``enqueue`` runs the launch at once."""
    capturing = None

    def __init__(self):
        self.launches = []

    @staticmethod
    def enqueue(launch):
        if HostGraph.capturing is None:
            launch()
        else:
            HostGraph.capturing.launches.append(launch)

    def capture(self, fn):
        HostGraph.capturing = self
        try:
            fn()
        finally:
            HostGraph.capturing = None
        return len(self.launches) == 0

    def replay(self):
        for launch in self.launches:
            launch()


class DeviceGraph:
    """One ``torch.cuda.CUDAGraph`` captured under ``torch.cuda.graph``: torch's default capture error mode, on torch's own side
    stream.  ``capture(fn)`` -> whether the graph came out empty (torch warns of a graph without nodes when the capture ends)."""

    def __init__(self):
        self.graph = torch.cuda.CUDAGraph()

    def capture(self, fn):
        import warnings
        raised = []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                with torch.cuda.graph(self.graph):
                    try:
                        fn()
                    except Exception as e:      # the capture is ended before anything is raised
                        raised.append(e)
            except Exception as e:
                if raised:
                    raise RuntimeError(f"{raised[0]}; and when the capture was ended: {e}") from e
                raise
        if raised:
            raise raised[0]
        return any("graph is empty" in str(w.message).lower() for w in caught)

    def replay(self):
        self.graph.replay()


class Memory:
    """What a case body sees.  ``place`` as Arena.place; ``call(module, name, *args)`` is ``module.load().call(name, device, *args)``
    with, in an arena, a snapshot before and a check behind: writable are the pieces whose parameter is "out" or "scratch" in
    ROLES[name] -- a blob that one call packs ("scratch") is protected in the next that takes it as ``const``.

    ``captured`` (no arena): every single call is captured in a graph of its own and replayed twice, each time from the contents
    its pieces had before the call (``_replayed``); the body goes on with what the second replay left."""

    def __init__(self, device, fill, roles=None, arena=None, captured=False):
        assert not (captured and arena is not None)
        self.device, self.fill, self.roles, self.arena, self.captured = torch.device(device), fill, roles or {}, arena, captured
        self.placed = []                # plain buffers live as long as the arena's pieces do: until the body is done

    def place(self, what, role, name=None, skew=0, copy=None):
        if self.arena is not None:
            return self.arena.place(what if isinstance(what, int) else what.to(self.device), role, name, skew, copy)
        assert role in ROLE_NAMES, role
        if isinstance(what, int):
            self.placed.append(self._empty(what))
            return self.placed[-1]
        t = self._empty(what.numel() * what.element_size() + skew)[skew:].view(what.dtype).view(what.shape)
        if role == "in" if copy is None else copy:
            t.copy_(what)
        self.placed.append(t)
        return t

    def _empty(self, nbytes):
        """the ordinary way: torch.empty, holding the pattern.  On the CPU (tests/test_arena.py) 64 bytes of slack stand behind it as
        the caching allocator's rounding stands behind a small GPU tensor, so that a stand-in can read past the end."""
        slack = 64 if self.device.type == "cpu" else 0
        return torch.empty(nbytes + slack, dtype=torch.uint8, device=self.device).fill_(self.fill)[:nbytes]

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def guarded(self, fn, writable, inputs=(), name=None, empty_ok=None):
        """run ``fn()``; in an arena: between a snapshot and a check that lets it write the pieces of ``writable`` (tensors).
        Captured: ``fn`` is one library call that may write ``writable`` and reads ``inputs`` (see ``_replayed``)."""
        if self.captured:
            return self._replayed(name or getattr(fn, "__name__", "the call"), fn, [(f"writable[{i}]", t) for i, t in enumerate(writable)],
                                  [(f"inputs[{i}]", t) for i, t in enumerate(inputs)], None, empty_ok)
        if self.arena is None:
            return fn()
        self.arena.snapshot()
        result = fn()
        self.arena.check(writable)
        return result

    def _replayed(self, name, fn, writable, inputs, last_error, empty_ok):
        """The stream contract of one call: ``fn`` is captured, not run, and what it enqueued is all it does.  The pieces are cloned;
        the capture; then twice: the writable pieces are put back (a launch that ran during the capture instead of being recorded
        is wiped here, and an argument the call updates in place starts from its start value again) and the graph is replayed.
        The two replays leave the same bits and no input has changed.  ``writable`` / ``inputs``: [(parameter name, tensor)]."""
        self._sync()
        before = [(pname, t, t.clone()) for pname, t in writable]
        held = [(pname, t, t.clone()) for pname, t in inputs]
        graph = HostGraph() if self.device.type == "cpu" else DeviceGraph()
        try:
            empty = graph.capture(fn)
        except Exception as e:
            text = last_error() if last_error is not None else None
            raise CaptureFailure(f"{name} could not be captured: it allocated, synchronised or used a stream other than the one it was given"
                                 f" ({type(e).__name__}: {e}; the library's last error: {text.decode() if text else 'none'})") from e
        self._sync()
        if empty and not empty_ok:
            raise CaptureFailure(f"{name}: the captured graph is empty -- nothing was enqueued on the stream the call was given")
        if empty_ok and not empty:
            raise CaptureFailure(f"{name}: the call enqueued work, but its call site says that it enqueues nothing ({empty_ok})")
        if empty:
            return

        def replay():
            for _, t, start in before:
                t.copy_(start)
            graph.replay()
            self._sync()

        replay()
        first = [t.clone() for _, t, _ in before]
        replay()
        for pname, t, start in held:
            assert bitwise_equal(start, t), f"{name} {pname}: an input was modified ({_differing(start, t)})"
        for (pname, t, _), a in zip(before, first):
            assert bitwise_equal(a, t), f"{name} {pname}: two replays from the same contents differ in {_differing(a, t)}"

    def call(self, module, name, *args, empty_ok=None):
        """``empty_ok`` (captured runs): the header's sentence by which this call enqueues nothing for this input"""
        declared = self.roles[name]
        from onepose_amd._binding import STREAM
        symbols = {**module.SYMBOLS, **getattr(module, "MORE_SYMBOLS", {})}
        table = symbols[name][1]
        pnames = [p[2] for p, entry in zip(parameters(name), table) if entry is not STREAM]
        assert len(pnames) == len(args), f"{name}: {len(pnames)} parameters besides the stream, {len(args)} given"
        writable, inputs = [], []
        for pname, a in zip(pnames, args):
            if isinstance(a, torch.Tensor):
                role = declared[pname]                      # KeyError: a device pointer the test module did not declare
                if self.arena is not None:
                    self.arena.piece_of(a)                  # KeyError: a tensor that was not placed
                (inputs if role == "in" else writable).append((pname, a))
        lib = module.load()
        if self.captured:
            last_error = getattr(lib, next(k for k in symbols if k.endswith("_last_error")))
            self._replayed(name, lambda: lib.call(name, self.device, *args), writable, inputs, last_error, empty_ok)
            return
        self.guarded(lambda: lib.call(name, self.device, *args), [a for _, a in writable])
        if self.arena is None and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)


def run_placement(body, device, roles=None, guard=65536, capacity=64 << 20):
    """The three steps of a placement case.  ``body(mem)`` -> {name: tensor}, or ({name: tensor}, {name: tensor}): the outputs, and
    for those the header says are partly "not written" the part it says is written.  Per pattern: plain run, arena run (every
    ``mem.call`` checked), outputs bitwise equal.  Across the patterns: what was written is bitwise equal.  Returns the arena outputs
    of the first pattern."""
    return _run_twice(body, device, "arena", lambda fill: Memory(device, fill, roles, Arena(device, guard=guard, fill=fill, capacity=capacity)))


def run_captured(body, device, roles=None, guard=None, capacity=None):
    """``run_placement`` with the captured run in the arena run's place (``guard`` and ``capacity`` are taken and not used: there is
    no arena).  Per pattern: plain run -- the eager reference, which also makes the runtime load every kernel of the case before
    anything is captured --, then the body on plain buffers with every single ``mem.call`` captured in a graph and replayed
    (``Memory._replayed``); outputs bitwise equal.  Across the patterns: what was written is bitwise equal.  Returns the captured
    run's outputs of the first pattern."""
    return _run_twice(body, device, "captured", lambda fill: Memory(device, fill, roles, captured=True))


def captured_twin(test):
    """A placement test takes its runner as ``run=run_placement``; this is the same test -- parameters, marks, ids and every
    assertion behind the runner -- with ``run_captured``.  A module binds it as ``test_x_captured = captured_twin(test_x)``."""
    @functools.wraps(test)
    def twin(*args, **kwargs):
        return test(*args, run=run_captured, **kwargs)
    assert "run" in inspect.signature(test).parameters, test.__name__
    twin.__name__ = twin.__qualname__ = test.__name__ + "_captured"
    return twin


def _run_twice(body, device, kind, second):
    written = {}
    first = None
    for fill in PATTERNS:
        runs = []
        other = second(fill)
        for mem in (Memory(device, fill, other.roles), other):
            got = body(mem)
            full, part = got if isinstance(got, tuple) else (got, {})
            assert full, "a case body returns its outputs"
            runs.append((full, {k: part.get(k, v).clone() for k, v in full.items()}))
        (plain, _), (placed, part) = runs
        assert set(plain) == set(placed)
        for k in plain:
            assert bitwise_equal(plain[k], placed[k]), \
                f"{k}: the {kind} run differs from the plain run under fill {fill:#04x} in {_differing(plain[k], placed[k])}"
        written[fill] = part
        first = first or placed
    a, b = (written[f] for f in PATTERNS)
    for k in a:
        assert bitwise_equal(a[k], b[k]), (f"{k}: the result depends on the fill pattern ({_differing(a[k], b[k])}): the call read a guard, "
                                           f"an unwritten part of its workspace or the bytes behind an input")
    return first


def _differing(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / dtype {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    ne = (_bytes_of(a.contiguous()) != _bytes_of(b.contiguous())).nonzero().reshape(-1)
    return f"{ne.numel()} byte(s), the first at byte {int(ne[0])}, the last at byte {int(ne[-1])}"
