"""The chunk plan of the host pipeline (hpp-fcl_amd/csrc/hfcl_plan.hpp: plan_chunks, called by host_batch) without a GPU: the header built
with g++ (tests/plan_harness).  The expected chunk sizes were worked out from the plan's rules and confirmed against the lines host_batch
held before they became this function."""
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
    d.ph_plan_chunks.restype = C.c_uint64

    def bounds(n, pipe_chunk=0, pipelined=True, f32=False):
        buf = np.zeros(4096, dtype=np.uint64)
        k = d.ph_plan_chunks(C.c_uint64(n), C.c_uint64(pipe_chunk), C.c_int(pipelined), C.c_int(f32), buf.ctypes.data_as(C.c_void_p), C.c_uint64(len(buf)))
        assert 2 <= k <= len(buf)
        return [int(x) for x in buf[:k]]

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
