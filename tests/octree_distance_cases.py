"""Shared pieces of the octree distance tests (tests/test_octree_distance_cpu.py, tests/test_octree_distance_gpu.py): the host build of
the device header (tests/octree_distance_harness) and its ctypes wrapper.  Trees and queries are those of octree_cases."""
import ctypes as C
import os
import subprocess

import numpy as np

import octree_cases as oc
from octree_cases import (ROOT, FLOAT_FIELDS, HarnessTrees, block_tree, chain_tree, compare_records, empty_tree, leaf_boxes,  # noqa: F401
                          random_queries, random_rotations, random_tree, seven_solids, three_state_tree, tree_from_spec)

RESOLUTION = 0.1


def build_harness(out_dir):
    """the g++ line of octree_cases.build_harness"""
    out = os.path.join(str(out_dir), "liboctree_distance_harness.so")
    src = os.path.join(ROOT, "tests", "octree_distance_harness", "octree_distance_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-shared", "-o", out, src])
    return C.CDLL(out)


def harness_distance(pkg, ohd, ht, L, octree, shape, tft, tfs, req, swapped=None):
    """(records, n_visited) of the harness"""
    abi = pkg.abi
    shapes = np.ascontiguousarray(L.shapes_array())
    verts = np.ascontiguousarray(L.vertices_array(), dtype=np.float64)
    if len(verts) == 0:
        verts = np.zeros((1, 3))
    n = len(octree)
    octree = np.ascontiguousarray(octree, dtype=np.uint32)
    shape = np.ascontiguousarray(shape, dtype=np.uint32)
    tft = np.ascontiguousarray(tft, dtype=np.float64).reshape(-1, 12)
    tfs = np.ascontiguousarray(tfs, dtype=np.float64).reshape(-1, 12)
    out = np.zeros(n, dtype=abi.RESULT_DTYPE)
    visited = np.zeros(n, dtype=np.uint32)
    sw = None if swapped is None else np.ascontiguousarray(swapped, dtype=np.uint8)
    rc = ohd.ohd_distance(abi.ptr(shapes), C.c_uint32(len(shapes)), abi.ptr(verts), C.c_uint32(ht.n), abi.ptr(ht.table), abi.ptr(ht.params),
                          abi.ptr(ht.nodes), abi.ptr(octree), abi.ptr(shape), abi.ptr(tft), abi.ptr(tfs), C.c_size_t(n), abi.ptr(sw),
                          C.byref(req), abi.ptr(out), abi.ptr(visited))
    assert rc == 0
    return out, visited


def random_setup(pkg, rng):
    """test_octree_cpu.random_setup: three random trees of depth 3 - 5 at resolution 0.1 and the seven solids"""
    trees = [(oc.random_tree(pkg, rng, 3), RESOLUTION, 3), (oc.random_tree(pkg, rng, 4), RESOLUTION, 4),
             (oc.random_tree(pkg, rng, 5, p_child=0.35), RESOLUTION, 5, 0.75, 0.1)]
    L, solids = oc.seven_solids(pkg, rng)
    return trees, L, solids


def request(abi, signed=True):
    req = abi.default_distance_request()
    req.enable_signed_distance = 1 if signed else 0
    return req
