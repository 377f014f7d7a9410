"""Placement tests of the training-set builder (include/gatsspg_trainset.h): every entry point with its device arguments carved exactly,
back to back with 64 KiB guards, from an arena (tests/arena.py), under the fill patterns 0xFF and 0x00 -- nothing outside the outputs
and the workspace of exactly gts_workspace_bytes is written, the arena run equals the plain run bit for bit, and both patterns give the
same bits.  Every test runs a second time with each call captured in a graph and replayed (arena.run_captured).

The header names its stream parameter ``queue``, so the completeness rule of tests/test_arena.py does not see these functions; the
rule is kept here instead: ``test_every_stream_taking_function_of_the_header_has_a_case`` holds ROLES to the header.  The oracle
comparisons are in tests/test_trainset_gpu.py."""
import os
import re

import pytest
import torch

import arena
import trainset_cases as tc
import trainset_oracle as oracle
from arena import bitwise_equal, captured_twin, run_placement

BINDING = tc.BINDING
ROLES = tc.ROLES
HEADER = os.path.join(arena.ROOT, "include", "gatsspg_trainset.h")
DEV = torch.device("cuda")


def test_declared_roles_agree_with_the_const_of_the_prototypes():
    assert ROLES
    arena.check_roles(BINDING, ROLES)


def test_every_stream_taking_function_of_the_header_has_a_case():
    """every function of the header with a gts_stream_t parameter is a key of ROLES, every key is such a function, and each key is
    called by a ``run=run_placement`` test below that has a captured twin"""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    declared = re.findall(r"\b(gts_\w+)\s*\(([^()]*)\)\s*;", text)
    streams = sorted(name for name, params in declared if "gts_stream_t" in params)
    assert len(streams) == 6 and "gts_workspace_bytes" not in streams
    assert streams == sorted(ROLES)
    for name in streams:
        assert [p[2] for p in arena.parameters(name)][-1] == "queue" and BINDING.SYMBOLS[name][1][-1] is arena_stream()
    with open(os.path.join(arena.ROOT, "tests", "trainset_cases.py")) as f:
        bodies = f.read()
    for name in streams:
        assert f'mem.call(BINDING, "{name}"' in bodies, name
    tests = [n for n in globals() if n.startswith("test_") and n.endswith("_captured")]
    assert len(tests) == 6 and all(n[:-len("_captured")] in globals() for n in tests)


def arena_stream():
    from onepose_amd._binding import STREAM
    return STREAM


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 8])
def test_assign_pairs(L, run=run_placement):
    c = tc.case(L)
    got = run(tc.body_assign(c), DEV, ROLES)
    assert int(got["pair_offsets"][-1]) > 0 and int(got["ignored"]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape3d,L", tc.TILES)
def test_select_and_gather_leaves(shape3d, L, run=run_placement):
    c = tc.case(L)
    images, epochs = tc.samples(3)
    leaf = run(tc.body_select(c, images, epochs, shape3d, L), DEV, ROLES)["leaf_src"]
    got = run(tc.body_gather(c, leaf.cpu().numpy(), shape3d, L), DEV, ROLES)["descriptors2d_db"]
    assert not torch.isnan(got).any() and got.shape == (3, 256, shape3d * L)


@pytest.mark.gpu
def test_gather_into_a_destination_that_is_not_16_byte_aligned(run=run_placement):
    """264 columns, a multiple of 4: the aligned destination is written 16 bytes per lane, four bytes further 4 bytes per lane -- same bits"""
    shape3d, L = 33, 8
    c = tc.case(L)
    leaf = oracle.select_leaves(c["point_offsets"], *tc.samples(2), shape3d, L, tc.SEED)
    aligned = run(tc.body_gather(c, leaf, shape3d, L), DEV, ROLES)["descriptors2d_db"]
    skewed = run(tc.body_gather(c, leaf, shape3d, L, skew=4), DEV, ROLES)["descriptors2d_db"]
    assert bitwise_equal(aligned, skewed)


@pytest.mark.gpu
@pytest.mark.parametrize("shape2d", tc.SHAPES2D)
def test_pad_query(shape2d, run=run_placement):
    got = run(tc.body_pad_query(tc.case(8), *tc.samples(3, shape2d), shape2d), DEV, ROLES)
    assert not any(torch.isnan(v).any() for v in got.values())


@pytest.mark.gpu
@pytest.mark.parametrize("shape3d", [1, 8, 33])
def test_pad_points(shape3d, run=run_placement):
    got = run(tc.body_pad_points(tc.case(8), *tc.samples(3), shape3d), DEV, ROLES)
    assert not any(torch.isnan(v).any() for v in got.values())


@pytest.mark.gpu
@pytest.mark.parametrize("shape3d,L", tc.TILES)
def test_build_batch(shape3d, L, run=run_placement):
    shape2d = tc.SHAPES2D[tc.TILES.index((shape3d, L))]
    got = run(tc.body_build(tc.case(L), *tc.samples(3, shape3d), shape2d, shape3d, L), DEV, ROLES)
    assert not any(torch.isnan(v).any() for v in got.values())


# every case again with each library call captured in a graph and replayed (arena.run_captured): the stream contract
test_assign_pairs_captured = captured_twin(test_assign_pairs)
test_select_and_gather_leaves_captured = captured_twin(test_select_and_gather_leaves)
test_gather_into_a_destination_that_is_not_16_byte_aligned_captured = captured_twin(test_gather_into_a_destination_that_is_not_16_byte_aligned)
test_pad_query_captured = captured_twin(test_pad_query)
test_pad_points_captured = captured_twin(test_pad_points)
test_build_batch_captured = captured_twin(test_build_batch)
