"""The hand-out of k_epa_loop<float, 8, 17>'s blocks (hpp-fcl_amd/csrc/hfcl_epa_pool.hpp) without a GPU: the header built with g++ into a
stand-alone program (tests/epa_pool_harness) whose simulated waves draw in seeded random interleavings of their refills and atomics.
Every block of [0, cnt) must be taken exactly once; S is a multiple of the grid, and cnt (no pool: the static schedule) at share 0 and
below min_refills full refills per wave; no wave makes more than K draws that return nothing.  The expected S and range length are
written out here from the rule (tools/sched_model.py: model_epa has the same), not taken from the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "epa_pool_harness", "epa_pool_harness.cpp")
GRIDS = (1, 7, 3072)
SHARES = (0, 10, 20, 50)
KS = (1, 3, 16)
MIN_REFILLS = (0, 2)
GROUPS = 8


def _cnts(grid):
    return sorted({0, 1, max(grid - 1, 0), grid, grid + 1, 16 * grid - 1, 16 * grid, 293397})


def _build(tmp, name, extra):
    out = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", out, SRC])
    return out


def _run(exe, seed, k, share, min_refills, grid):
    p = subprocess.run([exe, str(seed), str(k), str(share), str(min_refills), str(grid)] + [str(c) for c in _cnts(grid)],
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    rows = [[int(x) for x in line.split()] for line in p.stdout.splitlines()]
    assert [r[0] for r in rows] == _cnts(grid)
    return rows


def _check(rows, k, share, min_refills, grid):
    for cnt, g, sh, kk, mr, S, length, ok, twice, never, out_of_range, max_empty, atomics in rows:
        what = "cnt %d grid %d share %d K %d min_refills %d" % (cnt, grid, share, k, min_refills)
        assert (g, sh, kk, mr) == (grid, share, k, min_refills), what
        assert ok == 1 and twice == 0 and never == 0 and out_of_range == 0, (what, twice, never, out_of_range)
        assert max_empty <= k, (what, max_empty)
        if share == 0 or cnt < grid * GROUPS * min_refills:
            want_S = cnt
        else:
            want_S = (cnt - cnt * share // 100) // grid * grid
        assert S == want_S, (what, S, want_S)
        assert S == cnt or S % grid == 0, (what, S)
        assert length == (cnt - S + k - 1) // k, (what, length)
        if S == cnt:
            assert atomics == 0, (what, atomics)  # (the pool is never touched)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("epa_pool_harness"), "epa_pool_harness", ["-O2"])


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k", KS)
def test_every_block_exactly_once(harness, grid, k):
    for share in SHARES:
        for min_refills in MIN_REFILLS:
            for seed in (1, 2):
                _check(_run(harness, seed, k, share, min_refills, grid), k, share, min_refills, grid)


def test_headline_batch_engages_the_pool(harness):
    """The headline's 293 397 polytopes on 3 072 waves: the S of profiles/r07_a section 1, and a pool that is drawn from."""
    rows = {r[0]: r for r in _run(harness, 1, 16, 10, 2, 3072)}
    assert rows[293397][5] == 261120 and rows[293397][12] > 0
    rows = {r[0]: r for r in _run(harness, 1, 16, 20, 2, 3072)}
    assert rows[293397][5] == 233472
    # the two sides of the threshold (two full refills per wave)
    assert rows[16 * 3072 - 1][5] == 16 * 3072 - 1 and rows[16 * 3072][5] < 16 * 3072


def test_harness_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined (host code only, a process of its own; the runtimes linked statically,
    so nothing has to be preloaded)."""
    exe = _build(tmp_path, "epa_pool_harness_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    for grid, k, share, min_refills in ((3072, 16, 10, 2), (3072, 16, 50, 0), (7, 3, 20, 0), (1, 1, 50, 2), (7, 16, 0, 2)):
        _check(_run(exe, 3, k, share, min_refills, grid), k, share, min_refills, grid)
