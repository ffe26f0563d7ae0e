"""The decision bands of the mesh collide() checkers, from the oracle alone (no GPU): for every batch a call site of compare.boundary_band
names (tests/boundary_batches.py: CASES; the mixed family of tests/test_options_gpu.py) the number of oracle records within 1e-9 of the
request's decision boundary d = security_margin is the `allowed` the GPU test asserts -- 0 everywhere, so those checkers excuse no record.
The 500 001-query batch of tests/test_bvh_plan_sizes_gpu.py is held the same way in that module's fixture.

Figures are printed before they are asserted (pytest -s)."""
import os

import numpy as np
import pytest

import boundary_batches
from compare import boundary_band
from test_gpu_dispatch import mixed_library  # noqa: F401  (the fixture itself: the batch of the options suite's mixed family)
from test_gpu_parity import HOST_PIPELINE_CASES, host_pipeline_batch

N_THREADS = min(16, os.cpu_count() or 1)


def _population(ref, margin, what):
    a = np.abs(ref["distance"] - margin)
    print("    %s: %d records, boundary d = %g: %d within 1e-9, %d within 1e-6, the nearest %.3g away" % (
        what, len(ref), margin, int((a < 1e-9).sum()), int((a < 1e-6).sum()), float(a.min())))
    return int((a < 1e-9).sum())


@pytest.mark.parametrize("name", sorted(boundary_batches.CASES))
def test_boundary_population_is_the_allowed_one(pkg, oracle, name):
    b, req, case = boundary_batches.make(pkg, name)
    ref = boundary_batches.oracle_records(pkg, oracle, b, req, case.kind, n_threads=N_THREADS)
    assert _population(ref, case.margin, name) == case.allowed
    assert int(boundary_band(ref, case.margin, allowed=case.allowed, name=name).sum()) == case.allowed
    if case.margin:  # (a band centred on 0 would look at other records: none of them decides anything)
        assert 0.0 < (ref["num_contacts"] > 0).mean() < 1.0


@pytest.mark.parametrize("contacts", [False, True])
def test_boundary_population_of_the_mixed_library(pkg, oracle, mixed_library, contacts):  # noqa: F811
    b = mixed_library
    req = pkg.abi.default_collision_request()
    if contacts:
        req.num_max_contacts = 10 ** 6
    ref = boundary_batches.oracle_records(pkg, oracle, b, req, "mixed", n_threads=N_THREADS)
    assert _population(ref, 0.0, "options mixed, contacts=%s" % contacts) == 0


@pytest.mark.parametrize("case", HOST_PIPELINE_CASES)
def test_boundary_population_of_the_host_pipeline_batches(pkg, oracle, case):
    """test_gpu_parity.py::test_host_pipeline_equals_device_path holds the compact-pose records to the matrix-pose ones (solids, 300 000 pairs):
    no pair of these batches within 1e-9 of touching."""
    b, req = host_pipeline_batch(pkg, case)
    fn = oracle.distance_batch if b.kind == "distance" else oracle.collide_batch
    ref = fn(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, req, n_threads=N_THREADS)
    assert _population(ref, 0.0, case) == 0


def test_boundary_population_of_the_gjk_asserts_scene(pkg, oracle):
    """tests/test_gjk_asserts_regression.py::test_kernels: a unit sphere mesh in a radius-2 one moved by unit vectors -- tangent spheres, but
    the meshes are inscribed polyhedra at eight rotations: all 48 poses are contacts, none within 1e-9 of touching."""
    import test_gjk_asserts_regression as ga
    ref = ga.oracle_records(pkg, oracle, ga.make_scene(pkg))
    assert len(ref) == 48 and _population(ref, 0.0, "gjk-asserts") == 0


def test_boundary_band_counts_and_refuses():
    """The helper itself: the mask, the count it allows, the margin it is centred on."""
    ref = np.zeros(5, dtype=[("distance", np.float64)])
    ref["distance"] = [0.05, 0.05 + 5e-10, 0.05 - 2e-9, 5e-10, -1.0]
    assert boundary_band(ref, 0.05, allowed=2).tolist() == [True, True, False, False, False]
    assert boundary_band(ref, 0.0, allowed=1).tolist() == [False, False, False, True, False]
    with pytest.raises(AssertionError):
        boundary_band(ref, 0.05, allowed=1, name="one too many")
    with pytest.raises(AssertionError):
        boundary_band(ref, 0.0, name="none allowed")
    assert not boundary_band(ref, 0.3).any()
