"""The planning arithmetic of the host units (hpp-fcl_amd/csrc/hfcl_plan.hpp) without a GPU: the header built with g++
(tests/plan_harness).  plan_chunks, called by host_batch: the expected chunk sizes were worked out from the plan's rules and confirmed
against the lines host_batch held before they became this function.  The scene calls' chunk sizes, fold-partial bounds and list capacity
(hfcl_host_scene.hip): the expected values follow from their rules -- the option as given, or equal chunks of at most 2^21 (scene) / 2^22
(cull) queries; a scene chunk at most 2^32 - 16; pieces of 256 pairs; an eighth of the queries, at least 4096, at most all."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 4097, 65536, 65537, 98305, 200000, 1000000, 3000001]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan_harness") / "libplan_harness.so")
    src = os.path.join(ROOT, "tests", "plan_harness", "plan_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-shared", "-o", out, src])
    d = C.CDLL(out)
    for name in ("ph_plan_chunks", "ph_equal_chunks", "ph_scene_chunk_size", "ph_cull_chunk_size", "ph_scene_pieces_bound",
                 "ph_scene_listed_pieces_bound", "ph_list_capacity_guess", "ph_scene_piece_of"):
        getattr(d, name).restype = C.c_uint64

    def bounds(n, pipe_chunk=0, pipelined=True, f32=False):
        buf = np.zeros(4096, dtype=np.uint64)
        k = d.ph_plan_chunks(C.c_uint64(n), C.c_uint64(pipe_chunk), C.c_int(pipelined), C.c_int(f32), buf.ctypes.data_as(C.c_void_p), C.c_uint64(len(buf)))
        assert 2 <= k <= len(buf)
        return [int(x) for x in buf[:k]]

    bounds.dll = d
    return bounds


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pipe_chunk", [0, 50000])
@pytest.mark.parametrize("n", SIZES)
def test_bounds_cover_the_batch(plan, n, pipe_chunk, f32):
    b = plan(n, pipe_chunk, True, f32)
    assert b[0] == 0 and b[-1] == n
    assert all(hi > lo for lo, hi in zip(b, b[1:]))


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pipe_chunk", [0, 50000])
@pytest.mark.parametrize("n", SIZES)
def test_not_pipelined_is_one_chunk(plan, n, pipe_chunk, f32):
    assert plan(n, pipe_chunk, False, f32) == [0, n]


@pytest.mark.parametrize("n,f32,pipe_chunk,sizes", [
    (1000000, False, 0, [16384, 32768, 65536, 131072, 166666, 166666, 175148, 131072, 65536, 32768, 16384]),
    (1000000, True, 0, [333334, 333334, 333332]),
    (200000, False, 0, [16384, 32768, 65536, 36160, 32768, 16384]),
    (65537, False, 0, [65537]),
    (120000, False, 50000, [50000, 50000, 20000]),
])
def test_chunk_sizes(plan, n, f32, pipe_chunk, sizes):
    b = plan(n, pipe_chunk, True, f32)
    assert [hi - lo for lo, hi in zip(b, b[1:])] == sizes


# ---- the scene calls ----------------------------------------------------------------------------------------------------------------
def _u64(*xs):
    return [C.c_uint64(int(x)) for x in xs]


@pytest.mark.parametrize("total,option,auto_max,expected", [
    (1, 0, 1 << 21, 1),
    (1 << 21, 0, 1 << 21, 1 << 21),
    ((1 << 21) + 1, 0, 1 << 21, 1048577),
    (5000000, 0, 1 << 21, 1666667),
    (5000000, 0, 1 << 22, 2500000),
    (42, 200, 1 << 21, 42),
    (42, 5, 1 << 21, 5),
])
def test_equal_chunks(plan, total, option, auto_max, expected):
    d = plan.dll
    assert d.ph_equal_chunks(*_u64(total, option, auto_max)) == expected
    # the two callers: their own automatic size
    if auto_max == 1 << 21:
        assert d.ph_scene_chunk_size(*_u64(total, option)) == expected
    else:
        assert d.ph_cull_chunk_size(*_u64(total, option)) == expected


def test_scene_chunk_is_clamped_and_the_cull_chunk_is_not(plan):
    d = plan.dll
    assert d.ph_scene_chunk_size(*_u64(1 << 34, 1 << 33)) == 0xFFFFFFF0
    assert d.ph_cull_chunk_size(*_u64(1 << 34, 1 << 33)) == 1 << 33  # (kept as it is: the cull's option has no upper clamp)
    assert d.ph_equal_chunks(*_u64(1 << 34, 1 << 33, 1 << 21)) == 1 << 33


def test_pieces_bounds(plan):
    d = plan.dll
    assert d.ph_scene_pieces_bound(*_u64(600, 1000)) == 11  # 1000 // 256 + 2 + 2 * (1000 // 600 + 2)
    for m in (1, 255, 1000, 1 << 21):
        assert d.ph_scene_pieces_bound(*_u64(256, m)) == 0  # one piece: no partials
    assert d.ph_scene_listed_pieces_bound(*_u64(600, 5)) == 15
    assert d.ph_scene_listed_pieces_bound(*_u64(256, 5)) == 0


@pytest.mark.parametrize("total,expected", [(100, 100), (32768, 4096), (40000, 5000)])
def test_list_capacity_guess(plan, total, expected):
    assert plan.dll.ph_list_capacity_guess(C.c_uint64(total)) == expected


@pytest.mark.parametrize("n_pairs", [257, 600])
def test_flat_chunk_stays_within_its_pieces_bound(plan, n_pairs):
    """The pieces a chunk [q0, q0 + m) of the flat range touches -- scene_piece_of(q0 + m - 1) - scene_piece_of(q0) + 1, what the fold is
    given -- never exceed scene_pieces_bound(n_pairs, m), what the workspace holds: every q0 over three configurations."""
    d = plan.dll
    total = 3 * n_pairs
    piece = np.array([d.ph_scene_piece_of(C.c_uint64(q), C.c_uint32(n_pairs)) for q in range(total)], dtype=np.int64)
    for m in (1, 255, 256, 257, 1000):
        bound = d.ph_scene_pieces_bound(*_u64(n_pairs, m))
        q0 = np.arange(0, total - min(m, total) + 1)
        last = np.minimum(q0 + m, total) - 1
        touched = piece[last] - piece[q0] + 1
        assert touched.max() <= bound, (n_pairs, m, int(touched.max()), bound)
        assert touched.min() >= 1
