"""The database comparison of the reusing gatsspg_forward as a rider of the query window's GEMM launches.

fp32 frames of the reusing path compare the caller's database and weights with the workspace's snapshot in extra workgroups of the
first three GEMM launches of a call (qkv_kv, mlp0, mlp3 of attention layer 0 on the query window); `db_rider_share`
(onepose_amd/csrc/gatsspg_common.h) decides which launch compares which 16-byte words of which of the eight pieces.  The other
arithmetics run the same comparison as one launch of its own behind those launches.  On a miss the prepare chain then runs in the call's
own layout, behind the query-side launches of the same call, whose results must survive it.

The reference for "identical" is gatsspg_forward with GATSSPG_FLAG_NO_DB_REUSE -- the plain chain -- on the same inputs, compared bitwise.

`piece_bytes` and `rider_share` below mirror `db_piece_bytes` and `db_rider_share` of gatsspg_common.h; the CPU test at the top compiles a
plain C++ program against that header, which checks that the shares tile every piece and prints the piece sizes the mirror is held against.
The weights of the shares are read from the header.
"""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import gatsspg_oracle as orc
from onepose_amd import GATsSuperGlue, _native, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "onepose_amd", "csrc")
DEV = torch.device("cuda:0")
HP = dict(orc.DEFAULT_HPARAMS, match_threshold=0.0)
LEAF = 8
WORDS = dict(magic=0, b=1, n1p=2, n2=3, num_leaf=4, flags=5, fingerprint=6, snapshot_valid=7, miss=8, strike=9, hit=10, copy=11)
PIECES = ("desc3d_db", "desc2d_db", "GATs layer 0", "attention layer 0", "attention layer 1", "planes of attention layer 0",
          "planes of attention layer 1", "cache")

# gatsspg_common.h: floats of one attention block (AttnW::SIZE) and one GATs block (GatsW::SIZE), 16-bit elements of one block of planes
# (AttnWB::SIZE: five planes of each of the three operators), one KV partial (KVP); where the blocks start in the packed blob
BIG = 768 * 256 + 512 * 512 + 256 * 512
ATTN_W = BIG + 768 + 512 + 256 + 8
GATS_W = 512 + 256 * 256
ATTN_WB = 5 * BIG
KVP = 64 * 64 + 64 + 8
PW_GATS = 8 * ATTN_W
PW_TOTAL = PW_GATS + 4 * GATS_W + 256 * 256 + 256
FP_SAMPLES = 1024


def tiles(b, n1, n2):
    up = lambda n: (n + 127) // 128 * 128
    return b * (up(n1) + up(n2)) // 64


def piece_bytes(p, b, n2, num_leaf=LEAF):
    """db_piece_bytes."""
    plane = 4 * b * 256 * n2
    return (plane, plane * num_leaf, 4 * GATS_W, 4 * ATTN_W, 4 * ATTN_W, 2 * ATTN_WB, 2 * ATTN_WB, 2 * plane + 4 * b * 4 * KVP)[p]


@functools.lru_cache(maxsize=None)
def rider_weights():
    header = open(os.path.join(CSRC, "gatsspg_common.h")).read()
    w = re.search(r"DB_RIDER_WEIGHT\[DB_RIDER_LAUNCHES\]\s*=\s*\{([^}]*)\}", header).group(1)
    return tuple(int(x) for x in w.split(","))


def rider_share(n, k):
    """db_rider_share: words [lo, hi) of a piece of n words that riding launch k compares."""
    w = rider_weights()
    return n * sum(w[:k]) // sum(w), n * sum(w[:k + 1]) // sum(w)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the share function itself, from a plain C++ program (host compiler, address and undefined-behaviour sanitizers)
# ---------------------------------------------------------------------------------------------------------------------
SHARE_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "gatsspg_common.h"
using namespace gatsspg;
static int check(unsigned long long n) {
    unsigned long long at = 0;
    for (int k = 0; k < DB_RIDER_LAUNCHES; ++k) {
        unsigned long long lo, hi;
        db_rider_share(n, k, &lo, &hi);
        if (lo != at || hi < lo || hi > n) { std::printf("BAD n=%llu launch %d: [%llu, %llu) after %llu\n", n, k, lo, hi, at); return 1; }
        at = hi;
    }
    if (at != n) { std::printf("BAD n=%llu: the shares end at %llu\n", n, at); return 1; }
    return 0;
}
int main() {
    int bad = 0;
    const unsigned long long small[] = {0, 1, 255, 256, 257};
    for (unsigned long long n : small) bad += check(n);
    const int shapes[2][3] = {{1, 100, 4000}, {1, 1000, 7000}};
    for (auto& s : shapes)
        for (int p = 0; p < DB_PIECES; ++p) {
            const unsigned long long n = db_piece_bytes(p, s[0], s[2], 8) / 16;
            std::printf("piece %d %d %d %d %llu\n", s[0], s[1], s[2], p, n);
            bad += check(n);
        }
    for (int k = 0; k < DB_RIDER_LAUNCHES; ++k) {
        unsigned long long lo, hi;
        db_rider_share(900168, k, &lo, &hi);
        std::printf("share %d %llu %llu\n", k, lo, hi);
        if (DB_RIDER_BLOCKS[k] < 1 || DB_RIDER_BLOCKS[k] > 256) { std::printf("BAD rider count of launch %d\n", k); ++bad; }
    }
    return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
"""


def test_shares_tile_every_piece_in_a_plain_cpp_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src, exe = tmp_path / "share_main.cpp", tmp_path / "share_main"
    src.write_text(SHARE_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "BAD" not in run.stdout, run.stdout + run.stderr
    # the Python mirrors of this file against the header
    seen = [tuple(int(x) for x in line.split()[1:]) for line in run.stdout.splitlines() if line.startswith("piece")]
    assert len(seen) == 16
    for b, n1, n2, p, n in seen:
        assert piece_bytes(p, b, n2) == 16 * n, (b, n1, n2, PIECES[p])
    shares = [tuple(int(x) for x in line.split()[1:]) for line in run.stdout.splitlines() if line.startswith("share")]
    assert shares == [(k,) + rider_share(900168, k) for k in range(len(rider_weights()))]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


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
    """A workspace and its outputs for one shape, straight on the C ABI (the helper of tests/test_gats_db_reuse.py)."""

    def __init__(self, b, n1, n2, precision="fp32", extra=0):
        self.lib = _native.load()
        self.b, self.n1, self.n2 = b, n1, n2
        self.nbytes = self.lib.gatsspg_workspace_bytes(b, n1, n2, LEAF)
        self.ws = torch.zeros(self.nbytes + extra, device=DEV, dtype=torch.uint8)
        self.off = self.nbytes - 256 if tiles(b, n1, n2) > 64 else 0      # the state block: the last piece of a workspace with a reuse area
        eng = model(precision).engine
        self.packed, self.flags = eng.packed_weights(DEV), eng.flags()
        assert not self.flags & _native.FLAG_NO_DB_REUSE, "engine.flags() never sets the flag"

    def forward(self, q, d3, d2db, flags=None, packed=None, ws=None):
        b, n1, n2 = self.b, self.n1, self.n2
        out = (torch.empty(b, n1, n2, device=DEV), torch.empty(b, n1, device=DEV, dtype=torch.int64), torch.empty(b, n2, device=DEV, dtype=torch.int64),
               torch.empty(b, n1, device=DEV), torch.empty(b, n2, device=DEV))
        ws = self.ws if ws is None else ws
        _native.check(self.lib.gatsspg_forward((self.packed if packed is None else packed).data_ptr(), q.data_ptr(), d3.data_ptr(), d2db.data_ptr(), b, n1, n2,
                                               LEAF, self.flags if flags is None else flags, 0.07, 0.0, *(o.data_ptr() for o in out), ws.data_ptr(),
                                               self.nbytes, torch.cuda.current_stream(DEV).cuda_stream), "gatsspg_forward")
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

    def cache_offset(self):
        """Byte offset of the cache in the workspace, from the area's end (gatsspg_common.h: cache | snapshot pieces 0..6 | cache copy |
        state, every piece on 256 bytes), as tests/test_gats_db_reuse.py::test_overwritten_cache_alone_is_a_miss computes it."""
        up = lambda n: (n + 255) // 256 * 256
        copy = up(piece_bytes(7, self.b, self.n2))
        snapshot = sum(up(piece_bytes(p, self.b, self.n2)) for p in range(7))
        off = self.off - copy - snapshot - up(self.lib.gatsspg_db_cache_bytes(self.b, self.n2))
        assert off > 0
        return off, self.off - copy


def same(got, ref, what):
    torch.cuda.synchronize(DEV)
    for name, g, r in zip(("conf", "matches0", "matches1", "mscores0", "mscores1"), got, ref):
        g, r = (g.view(torch.int32), r.view(torch.int32)) if g.dtype == torch.float32 else (g, r)
        assert torch.equal(g, r), f"{what}: {name} differs from the plain chain in {int((g != r).sum())} entries"
    assert int((got[1] >= 0).sum()) > 0, f"{what}: no match at all"


def warm(slot, d3, d2db, q, packed=None):
    """Two misses, then a hit: the state of a workspace that has seen one database for a while."""
    for _ in range(3):
        slot.forward(q, d3, d2db, packed=packed)
    assert slot.word("hit") == 1 and slot.word("snapshot_valid") == 1


def int32_view(t):
    return t.view(-1).view(torch.int32)


def piece_ints(p, slot, d3, d2db, packed):
    """Piece p as the int32 tensor the comparison walks (a view of the caller's tensor, or of the workspace for the cache)."""
    n = piece_bytes(p, slot.b, slot.n2) // 4
    if p == 0:
        v = int32_view(d3)
    elif p == 1:
        v = int32_view(d2db)
    elif p == 7:
        off, _ = slot.cache_offset()
        v = slot.ws[off: off + 4 * n].view(torch.int32)
    else:
        blob = int32_view(packed)
        start = {2: PW_GATS, 3: 0, 4: ATTN_W, 5: PW_TOTAL, 6: PW_TOTAL + ATTN_WB // 2}[p]
        v = blob[start: start + n]
    assert v.numel() == n, PIECES[p]
    return v


def fingerprint_sample(p, slot):
    """The 4-byte words of the two database tensors that enter the fingerprint: a flip there changes it, and the call after the miss
    is then a second miss (no strike) instead of a hit."""
    if p > 1:
        return set()
    n = piece_bytes(p, slot.b, slot.n2) // 4
    return {k * n // FP_SAMPLES for k in range(FP_SAMPLES)}


def boundary_words(n):
    """First and last word of a piece of n words and the words on each side of every share boundary."""
    words = {0, n - 1}
    for k in range(len(rider_weights())):
        lo, hi = rider_share(n, k)
        words |= {w for w in (lo - 1, lo, hi - 1, hi) if 0 <= w < n}
    return sorted(words)


@gpu
def test_the_mirrored_layout_is_the_workspace_s():
    q, d3, d2db = inputs(1, 100, 4000, 7)
    slot = Slot(1, 100, 4000)
    warm(slot, d3, d2db, q)
    cache, copy = slot.cache_offset()
    n = piece_bytes(7, 1, 4000)
    assert torch.equal(slot.ws[cache: cache + n], slot.ws[copy: copy + n]), "the cache and its copy lie where the mirror says"
    assert int(slot.ws[cache: cache + n].view(torch.int32).ne(0).sum()) > n // 8


@gpu
@pytest.mark.parametrize("b,n1,n2,precision", [(1, 100, 4000, "fp32"), (2, 100, 2000, "fp32"), (1, 200, 3900, "fp32"), (1, 100, 6000, "fp16x4")])
def test_a_flipped_bit_at_every_share_boundary_is_a_miss(b, n1, n2, precision):
    """fp32: every word next to a boundary between two riding launches' shares, and the ends of every piece.  fp16x4 has no riders: the
    same words through the stand-alone launch's one bounded grid (its pieces 5 and 6, the 16-bit planes, are compared there only)."""
    assert tiles(b, n1, n2) > 64
    q, d3, d2db = (t.clone() for t in inputs(b, n1, n2, 7))
    slot = Slot(b, n1, n2, precision)
    packed = slot.packed.clone()
    warm(slot, d3, d2db, q, packed)
    flips, ref_cache = 0, None
    for p in range(8):
        if p in (5, 6) and precision == "fp32":
            continue                                  # not read by the fp32 arithmetic, not compared
        ints, sample = piece_ints(p, slot, d3, d2db, packed), fingerprint_sample(p, slot)
        for w in boundary_words(piece_bytes(p, b, n2) // 16):
            i = next(4 * w + j for j in (1, 2) if 4 * w + j not in sample)    # an int of the 16-byte word outside the fingerprint's sample
            torch.cuda.synchronize(DEV)
            ints[i] ^= 1 << 20
            what = f"{precision} {PIECES[p]}, word {w}"
            got = slot.forward(q, d3, d2db, packed=packed)
            assert (slot.word("hit"), slot.word("miss")) == (0, 0), what
            if p < 7:
                same(got, slot.reference(q, d3, d2db, packed=packed), what)
            else:                                     # the inputs no longer change: one reference for every flip inside the cache
                ref_cache = slot.reference(q, d3, d2db, packed=packed) if ref_cache is None else ref_cache
                same(got, ref_cache, what)
            slot.forward(q, d3, d2db, packed=packed)
            assert slot.word("hit") == 1, f"the call after the miss on {what}"
            flips += 1
    assert flips >= (6 if precision == "fp32" else 8) * 4


@gpu
@pytest.mark.parametrize("b,n1,n2", [(1, 100, 4000), (2, 100, 2000), (1, 200, 3900)])
def test_a_miss_after_hits_keeps_the_new_query_s_own_query_side(b, n1, n2):
    """The query-side launches of a call run BEFORE the prepare chain of the same call: on a miss their results (this call's query, not
    the previous call's) must reach the rest of the forward."""
    qs = [inputs(b, n1, n2, 100 + i)[0] for i in range(4)]
    _, d3, d2db = (t.clone() for t in inputs(b, n1, n2, 7))
    slot = Slot(b, n1, n2)
    warm(slot, d3, d2db, qs[0])
    _, d3n, d2n = inputs(b, n1, n2, 8)
    d3.copy_(d3n)
    d2db.copy_(d2n)                                   # another database in the same memory
    got = slot.forward(qs[1], d3, d2db)
    assert (slot.word("hit"), slot.word("miss"), slot.word("strike")) == (0, 0, 0)
    same(got, slot.reference(qs[1], d3, d2db), "miss after hits, new query")
    got = slot.forward(qs[2], d3, d2db)
    assert (slot.word("hit"), slot.word("strike"), slot.word("copy")) == (0, 1, 1)
    same(got, slot.reference(qs[2], d3, d2db), "second miss on the new database")
    got = slot.forward(qs[3], d3, d2db)
    assert slot.word("hit") == 1
    same(got, slot.reference(qs[3], d3, d2db), "hit on the new database")


@gpu
@pytest.mark.parametrize("b,n1,n2", [(1, 100, 4000), (1, 200, 3900)])
def test_from_a_dirty_workspace(b, n1, n2):
    qs = [inputs(b, n1, n2, 100 + i)[0] for i in range(3)]
    _, d3, d2db = inputs(b, n1, n2, 7)
    slot = Slot(b, n1, n2)
    slot.ws.fill_(0xFF)                               # every float a NaN, every word of the state -1
    for i, q in enumerate(qs):
        got = slot.forward(q, d3, d2db)
        assert slot.word("hit") == (1 if i == 2 else 0), f"call {i + 1}"
        same(got, slot.reference(q, d3, d2db), f"dirty workspace, call {i + 1}")


@gpu
def test_no_rider_runs_under_the_flag_or_below_the_threshold():
    # the flag: the state block of a workspace with an area stays what it was
    q, d3, d2db = inputs(1, 100, 4000, 7)
    slot = Slot(1, 100, 4000)
    slot.ws[slot.off: slot.off + 64].fill_(0x5A)
    before = slot.state_bytes()
    ref = slot.reference(q, d3, d2db)
    for _ in range(2):
        same(slot.forward(q, d3, d2db, flags=slot.flags | _native.FLAG_NO_DB_REUSE), ref, "with the flag")
    assert torch.equal(slot.state_bytes(), before), "a launch under the flag wrote the state block"
    # below the threshold (64 tiles): the bytes behind a plain workspace, where the area of a larger shape would lie, stay untouched
    q, d3, d2db = inputs(1, 100, 3900, 7)
    assert tiles(1, 100, 3900) == 64
    slot = Slot(1, 100, 3900, extra=Slot(1, 100, 4000).nbytes)
    assert slot.off == 0
    slot.ws[slot.nbytes:].fill_(0xA5)
    ref = slot.reference(q, d3, d2db)
    for _ in range(2):
        same(slot.forward(q, d3, d2db), ref, "64 tiles")
    assert bool((slot.ws[slot.nbytes:] == 0xA5).all()), "bytes behind the plain workspace were written"
