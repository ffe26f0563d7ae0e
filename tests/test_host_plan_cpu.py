"""The planning arithmetic of the host units (hpp-fcl_amd/csrc/hfcl_plan.hpp) without a GPU: the header built with g++
(tests/plan_harness).  plan_chunks, called by host_batch: the expected chunk sizes were worked out from the plan's rules and confirmed
against the lines host_batch held before they became this function.  The scene calls' chunk sizes, fold-partial bounds and list capacity
(hfcl_host_scene.hip): the expected values follow from their rules -- the option as given, or equal chunks of at most 2^21 (scene) / 2^22
(cull) queries; a scene chunk at most 2^32 - 16; pieces of 256 pairs; an eighth of the queries, at least 4096, at most all.  The plans of
the two sweeps that make lists of pairs (SelfSweep, EnvSweep): see the cases."""
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
                 "ph_scene_listed_pieces_bound", "ph_list_capacity_guess", "ph_scene_piece_of", "ph_sweep_conf_per_chunk", "ph_env_sweep_span"):
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


# ---- the sweeps that make a list of pairs --------------------------------------------------------------------------------------------
# The expected values are worked out by hand from the expressions the two users of each sweep held before they became these functions:
# rows_per_block 16 (PAIRS_ROWS) or n (small: n <= min(option, 64)); blocks_per_conf = ceil(n / rows_per_block); per = option // 16 rows in
# whole blocks, at least 1, at most n_blocks, or (0) 2^20 rows cut into equal chunks; conf_per_chunk = min(n_conf, per // blocks_per_conf
# + 2); chunk_rows = min(per * rows_per_block, n_conf * n).  Env: tiles of 256 columns, moving then environment; span from the option or
# env_auto_span (4 workgroups a compute unit); per = option // 16 or (0) 2^22 // n_spans // 16; scan_rows = chunk_rows * n_spans.
def _plan_out(d, name, n_out, *args):
    out = np.zeros(n_out, dtype=np.uint64)
    getattr(d, name).restype = None
    getattr(d, name)(*args, out.ctypes.data_as(C.c_void_p))
    return [int(x) for x in out]


@pytest.mark.parametrize("n,n_conf,small_max,option,expected", [
    # small, rows_per_block, blocks_per_conf, n_blocks, per, conf_per_chunk, chunk_rows
    (16, 64, 32, 342, [1, 16, 1, 64, 21, 23, 336]),     # a wave per configuration, rows in three chunks
    (100, 10, 32, 0, [0, 16, 7, 70, 70, 10, 1000]),     # automatic: one chunk; its rows are the table's, not 70 x 16
    (100, 10, 32, 160, [0, 16, 7, 70, 10, 3, 160]),     # per = 10 is no multiple of the 7 blocks of a configuration
    (100, 1, 32, 0, [0, 16, 7, 7, 7, 1, 100]),          # n_conf 1
    (70, 3, 100, 16, [0, 16, 5, 15, 1, 2, 16]),         # the option above PAIRS_SMALL_MAX is 64: 70 objects are not small; one block a chunk
    (2, 5, 32, 0, [1, 2, 1, 5, 5, 5, 10]),
])
def test_self_sweep_plan(plan, n, n_conf, small_max, option, expected):
    got = _plan_out(plan.dll, "ph_self_sweep_plan", 7, C.c_uint32(n), C.c_uint64(n_conf), C.c_uint32(small_max), C.c_uint64(option))
    assert got == expected


@pytest.mark.parametrize("span_option,tiles,n_blocks,n_cus,expected", [
    (3, 10, 100, 256, 3),     # the option as given
    (0, 10, 100, 256, 1),     # 1024 workgroups wanted of 100 blocks: 11 spans, 10 // 11 tiles -> at least one
    (0, 40, 1024, 256, 40),   # enough blocks: one span
    (0, 64, 128, 256, 8),     # 1151 // 128 = 8 spans of 8 tiles
    (0, 5, 1, 0, 1),          # no compute unit known counts as one: 4 spans, 5 // 4
])
def test_env_sweep_span(plan, span_option, tiles, n_blocks, n_cus, expected):
    assert plan.dll.ph_env_sweep_span(C.c_uint32(span_option), C.c_uint32(tiles), C.c_uint64(n_blocks), C.c_int(n_cus)) == expected


@pytest.mark.parametrize("nm,ne,n_conf,span_option,n_cus,option,expected", [
    # blocks_per_conf, tiles_moving, tiles, span_len, n_spans, n_blocks, per, conf_per_chunk, chunk_rows, scan_rows
    (1, 1000, 4, 0, 256, 0, [1, 1, 5, 1, 5, 4, 4, 4, 4, 20]),          # one moving object: a chunk's rows are the table's 4, not 4 x 16
    (6, 0, 64, 0, 256, 128, [1, 1, 1, 1, 1, 64, 8, 10, 128, 128]),     # no environment object: the one moving tile
    (40, 600, 5, 2, 256, 112, [3, 1, 4, 2, 2, 15, 7, 4, 112, 224]),    # per = 7 is no multiple of the 3 blocks of a configuration
    (6, 10, 1, 1, 256, 0, [1, 1, 2, 1, 2, 1, 1, 1, 6, 12]),            # n_conf 1
    (6, 10, 64, 9, 256, 0, [1, 1, 2, 2, 1, 64, 64, 64, 384, 384]),     # a span longer than the tiles is all of them
])
def test_env_sweep_plan(plan, nm, ne, n_conf, span_option, n_cus, option, expected):
    got = _plan_out(plan.dll, "ph_env_sweep_plan", 10, C.c_uint32(nm), C.c_uint32(ne), C.c_uint64(n_conf), C.c_uint32(span_option), C.c_int(n_cus),
                    C.c_uint64(option))
    assert got == expected
    assert plan.dll.ph_sweep_conf_per_chunk(C.c_uint64(n_conf), C.c_uint64(got[6]), C.c_uint32(got[0])) == got[7]
