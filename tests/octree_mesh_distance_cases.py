"""Shared pieces of the octree x mesh distance tests (tests/test_octree_mesh_distance_cpu.py, tests/test_octree_mesh_distance_gpu.py): the
host build of the device header (tests/octree_mesh_distance_harness), its ctypes wrapper, the seeded random queries.  Trees:
tests/octree_cases.py; meshes: tests/octree_mesh_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import octree_cases as oc
import octree_mesh_cases as omc
from octree_mesh_cases import DEPTH_LIMIT, HarnessMeshes, box_mesh, chain_mesh, one_triangle, sphere_mesh, two_triangles  # noqa: F401

ROOT = oc.ROOT
RESOLUTION = 0.1
GCC_FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized"]


def build_harness(out_dir):
    """the g++ line of octree_cases.build_harness"""
    out = os.path.join(str(out_dir), "liboctree_mesh_distance_harness.so")
    src = os.path.join(ROOT, "tests", "octree_mesh_distance_harness", "octree_mesh_distance_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-fPIC"] + GCC_FLAGS + ["-shared", "-o", out, src])
    lib = C.CDLL(out)
    lib.omdh_bvh_depth.restype = C.c_uint32
    lib.omdh_depth_limit.restype = C.c_uint32
    return lib


def harness_distance(pkg, h, ht, hm, octree, mesh, tft, tfm, req, swapped=None, pairs_cap=0, expect=0):
    """(records, n_visited, pairs[n_pairs, 3]) of the harness; expect: its return code"""
    abi = pkg.abi
    n = len(octree)
    octree = np.ascontiguousarray(octree, dtype=np.uint32)
    mesh = np.ascontiguousarray(mesh, dtype=np.uint32)
    tft = np.ascontiguousarray(tft, dtype=np.float64).reshape(-1, 12)
    tfm = np.ascontiguousarray(tfm, dtype=np.float64).reshape(-1, 12)
    out = np.zeros(n, dtype=abi.RESULT_DTYPE)
    visited = np.zeros(n, dtype=np.uint32)
    pairs = np.zeros((max(pairs_cap, 1), 3), dtype=np.uint32)
    npairs = C.c_size_t(0)
    sw = None if swapped is None else np.ascontiguousarray(swapped, dtype=np.uint8)
    rc = h.omdh_distance(C.c_uint32(ht.n), abi.ptr(ht.table), abi.ptr(ht.params), abi.ptr(ht.nodes), C.c_uint32(hm.n), abi.ptr(hm.table),
                         abi.ptr(hm.nodes), C.c_size_t(len(hm.nodes)), abi.ptr(hm.verts), abi.ptr(hm.tris), abi.ptr(octree), abi.ptr(mesh),
                         abi.ptr(tft), abi.ptr(tfm), C.c_size_t(n), abi.ptr(sw), C.byref(req), abi.ptr(out), abi.ptr(visited),
                         abi.ptr(pairs) if pairs_cap else None, C.c_size_t(pairs_cap), C.byref(npairs))
    assert rc == expect, rc
    if pairs_cap:
        assert npairs.value <= pairs_cap, (npairs.value, pairs_cap)
    return out, visited, pairs[:min(npairs.value, pairs_cap)]


def request(abi, signed=True):
    req = abi.default_distance_request()
    req.enable_signed_distance = 1 if signed else 0
    return req


def random_setup(pkg, rng):
    """test_octree_mesh_cpu.random_setup plus the block: three random trees of depth 3 - 5 at resolution 0.1 and the full 8 x 8 x 8
    block; meshes of 1, 2, 12 and 288 triangles"""
    trees = [(oc.random_tree(pkg, rng, 3), RESOLUTION, 3), (oc.random_tree(pkg, rng, 4), RESOLUTION, 4),
             (oc.random_tree(pkg, rng, 5, p_child=0.35), RESOLUTION, 5, 0.75, 0.1), (oc.block_tree(pkg), RESOLUTION, 4)]
    meshes = [one_triangle(), two_triangles(), box_mesh(), sphere_mesh(pkg)]
    assert [len(m.triangles) for m in meshes] == [1, 2, 12, 288]
    return trees, meshes


def soup(mesh, shrink=0.9):
    """the same triangles, each with vertices of its own, drawn towards its centroid: no two of them share a vertex or an edge, so no
    two are equally far from a voxel but by accident"""
    v = np.concatenate([mesh.vertices[t].mean(axis=0) + shrink * (mesh.vertices[t] - mesh.vertices[t].mean(axis=0)) for t in mesh.triangles])
    return omc.omm.Mesh(v, np.arange(len(v)).reshape(-1, 3))


def soup_setup(pkg, rng):
    """random_setup with soup() of the meshes that have more than one triangle"""
    trees, meshes = random_setup(pkg, rng)
    meshes = [meshes[0]] + [soup(m) for m in meshes[1:]]
    assert [len(m.triangles) for m in meshes] == [1, 2, 12, 288]
    return trees, meshes


def mesh_ids(rng, n, big_share=0.08):
    """a mesh per query: the 288-triangle mesh (id 3) for less than a tenth of them, the three small ones for the rest"""
    ids = rng.integers(0, 3, n).astype(np.uint32)
    ids[rng.uniform(size=n) < big_share] = 3
    return ids


def random_queries(pkg, rng, trees, mesh, spread, clear=None, identity_share=1.0 / 3.0):
    """a query per entry of `mesh` (the mesh ids): trees under rotated and translated poses (a share at the identity), meshes under
    rotated poses (a share at the identity rotation, where the tree's pose is not the identity), both operand orders.
    clear is None: the mesh's origin near a reachable leaf of the tree, up to `spread` off its surface -- part of the queries penetrate.
    clear = (radius per mesh id): the mesh's origin beyond the tree's outermost reachable leaf along a random direction, by the mesh's
    radius about its origin plus up to `spread` -- the tree lies behind a plane the mesh does not reach: every query is separated."""
    geo = pkg.geometry
    n = len(mesh)
    boxes = [oc.leaf_boxes(*t[:3], *t[3:5]) for t in trees]
    octree = rng.integers(0, len(trees), n).astype(np.uint32)
    tft = geo.make_pose(quat=oc.random_rotations(rng, n), T=rng.uniform(-2.0, 2.0, (n, 3)))
    ident = rng.uniform(size=n) < identity_share
    tft[ident] = geo.make_pose()
    local = np.zeros((n, 3))
    for i in range(n):
        b = boxes[int(octree[i])]
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        if not b:
            local[i] = rng.uniform(-0.3, 0.3, 3)
        elif clear is None:
            _, lo, hi = b[int(rng.integers(0, len(b)))]
            lo, hi = np.array(lo), np.array(hi)
            local[i] = 0.5 * (lo + hi) + d * (0.5 * (hi - lo).max() + rng.uniform(0.0, spread))
        else:
            far = max(float(np.maximum(d * np.array(lo), d * np.array(hi)).sum()) for _, lo, hi in b)  # the tree's support along d
            _, lo, hi = b[int(rng.integers(0, len(b)))]
            c = 0.5 * (np.array(lo) + np.array(hi))
            local[i] = c + d * (far - float(d @ c) + clear[int(mesh[i])] + rng.uniform(0.0, spread))
    world = geo.transform_point(tft, local)
    tfm = geo.make_pose(quat=oc.random_rotations(rng, n), T=world)
    plain = (rng.uniform(size=n) < 0.35) & ~ident  # (never both: axis-aligned triangles over axis-aligned voxels are equally far from several)
    tfm[plain, :9] = geo.make_pose().reshape(-1)[:9]
    swapped = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    return octree, np.ascontiguousarray(mesh, dtype=np.uint32), tft, tfm, swapped


def mesh_radii(meshes):
    """the largest distance of a vertex from the mesh's origin, per mesh"""
    return [float(np.linalg.norm(m.vertices, axis=1).max()) for m in meshes]
