"""Shared pieces of the octree x mesh tests (tests/test_octree_mesh_cpu.py, tests/test_octree_mesh_gpu.py): the host build of the device
header (tests/octree_mesh_harness), small meshes with the oracle's BVH, seeded random queries.  Trees: tests/octree_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import octree_cases as oc
import octree_mesh_model as omm
import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH_LIMIT = 64  # HFCL_OCTREE_MESH_MAX_BVH_DEPTH


def build_harness(out_dir):
    """the g++ line of octree_cases.build_harness"""
    out = os.path.join(str(out_dir), "liboctree_mesh_harness.so")
    src = os.path.join(ROOT, "tests", "octree_mesh_harness", "octree_mesh_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-shared", "-o", out, src])
    lib = C.CDLL(out)
    lib.omh_bvh_depth.restype = C.c_uint32
    lib.omh_depth_limit.restype = C.c_uint32
    return lib


class HarnessMeshes:
    """the tables of several meshes one after the other, as the library keeps them: (node_off, vert_off, tri_off, n_nodes) a mesh"""

    def __init__(self, pkg, meshes):
        self.n = len(meshes)
        tab, no, vo, to = [], 0, 0, 0
        for m in meshes:
            tab.append((no, vo, to, len(m.nodes)))
            no, vo, to = no + len(m.nodes), vo + len(m.vertices), to + len(m.triangles)
        self.table = np.array(tab, dtype=np.uint32)
        self.nodes = np.ascontiguousarray(np.concatenate([m.nodes for m in meshes]), dtype=pkg.abi.BVH_NODE_DTYPE)
        self.verts = np.ascontiguousarray(np.concatenate([m.vertices for m in meshes]), dtype=np.float64)
        self.tris = np.ascontiguousarray(np.concatenate([m.triangles for m in meshes]), dtype=np.uint32)


def harness_collide(pkg, oh, ht, hm, octree, mesh, tft, tfm, req, swapped=None, cap=0, items_cap=0, expect=0):
    """(records, bounds, contacts, n_produced, items[n_items, 3]) of the harness; expect: its return code"""
    abi = pkg.abi
    n = len(octree)
    octree = np.ascontiguousarray(octree, dtype=np.uint32)
    mesh = np.ascontiguousarray(mesh, dtype=np.uint32)
    tft = np.ascontiguousarray(tft, dtype=np.float64).reshape(-1, 12)
    tfm = np.ascontiguousarray(tfm, dtype=np.float64).reshape(-1, 12)
    out = np.zeros(n, dtype=abi.RESULT_DTYPE)
    dlb = np.zeros(n)
    contacts = np.zeros(max(cap, 1), dtype=abi.CONTACT_DTYPE)
    items = np.zeros((max(items_cap, 1), 3), dtype=np.uint32)
    nc, ni = C.c_size_t(0), C.c_size_t(0)
    sw = None if swapped is None else np.ascontiguousarray(swapped, dtype=np.uint8)
    rc = oh.omh_collide(C.c_uint32(ht.n), abi.ptr(ht.table), abi.ptr(ht.params), abi.ptr(ht.nodes), C.c_uint32(hm.n), abi.ptr(hm.table),
                        abi.ptr(hm.nodes), C.c_size_t(len(hm.nodes)), abi.ptr(hm.verts), abi.ptr(hm.tris), abi.ptr(octree), abi.ptr(mesh),
                        abi.ptr(tft), abi.ptr(tfm), C.c_size_t(n), abi.ptr(sw), C.byref(req), abi.ptr(out), abi.ptr(dlb), abi.ptr(contacts),
                        C.c_size_t(cap), C.byref(nc), abi.ptr(items) if items_cap else None, C.c_size_t(items_cap), C.byref(ni))
    assert rc == expect, rc
    return out, dlb, contacts[:min(nc.value, cap)], int(nc.value), items[:min(ni.value, items_cap)]


# ---- meshes (octree_mesh_model.Mesh: the oracle's BVH) -------------------------------------------------------------------------------
def one_triangle(s=0.3):
    return omm.Mesh([[0.0, 0.0, 0.0], [s, 0.0, 0.0], [0.0, s, 0.05 * s]], [[0, 1, 2]])


def two_triangles(s=0.3):
    return omm.Mesh([[0.0, 0.0, 0.0], [s, 0.0, 0.0], [s, s, 0.1 * s], [0.0, s, 0.0]], [[0, 1, 2], [0, 2, 3]])


def box_mesh(hx=0.12, hy=0.08, hz=0.15):
    """the 12 triangles of a box"""
    v = np.array([[sx * hx, sy * hy, sz * hz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    t = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    return omm.Mesh(v, t)


def sphere_mesh(pkg, r=0.15, seg=12, ring=12):
    """generateBVHModel(Sphere): 2 * seg * ring triangles (288)"""
    v, t = pkg.bvh_builder.uv_sphere(seg, ring, r)
    return omm.Mesh(v, t)


def flat_mesh(n=8, side=0.8, origin=(-0.8, -0.8, -0.75)):
    """2 n^2 triangles of a square sheet (over the block of octree_cases.block_tree by default)"""
    xs = np.linspace(0.0, side, n + 1)
    v = np.array([[origin[0] + x, origin[1] + y, origin[2]] for y in xs for x in xs])
    t = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            t += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    return omm.Mesh(v, t)


def chain_mesh(levels, s=0.04):
    """`levels` small triangles along a diagonal of [-0.2, 0.2]^3 under a hand-made BVH that is a chain of `levels` levels: node 2k is the
    inner node of triangles k .., its left child the leaf of triangle k, its right child node 2k + 2; every OBB is the axis-aligned box of
    its triangles.  (BVHModel's own splitter parts a set at the mean of the centroids: it makes a chain only when every triangle lies
    farther out than the mean of all before it, which for 64 levels spreads the offsets over more than 80 orders of magnitude -- box
    tests on such a mesh are rounding noise and no walk reaches its deep end.)"""
    pkg_abi = ob._pkg().abi
    v, t = [], []
    for k in range(levels):
        x = -0.2 + 0.4 * k / max(levels - 1, 1)
        v += [[x, 0.5 * x, -x], [x + s, 0.5 * x, -x], [x, 0.5 * x + s, -x + 0.3 * s]]
        t.append([3 * k, 3 * k + 1, 3 * k + 2])
    v = np.array(v)
    nodes = np.zeros(2 * levels - 1, dtype=pkg_abi.BVH_NODE_DTYPE)
    nodes["obb_axes"][:] = nodes["rss_axes"][:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]

    def box(i, pts):
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        nodes["obb_To"][i], nodes["obb_extent"][i] = 0.5 * (lo + hi), 0.5 * (hi - lo)

    for k in range(levels):
        leaf = 2 * k + 1 if k < levels - 1 else 2 * k
        nodes["first_child"][leaf] = -(k + 1)
        nodes["first_primitive"][leaf], nodes["num_primitives"][leaf] = k, 1
        box(leaf, v[3 * k:3 * k + 3])
        if k < levels - 1:
            nodes["first_child"][2 * k] = 2 * k + 1
            nodes["first_primitive"][2 * k], nodes["num_primitives"][2 * k] = k, levels - k
            box(2 * k, v[3 * k:])
    m = omm.Mesh(v, t, nodes)
    assert m.depth() == levels, (m.depth(), levels)
    return m


# ---- seeded random queries --------------------------------------------------------------------------------------------------------
def random_queries(pkg, rng, trees, n_meshes, n, spread=0.35, identity_share=1.0 / 3.0):
    """octree_cases.random_queries with meshes in the place of the solids: (octree, mesh, tf_octree, tf_mesh, swapped); a share of the
    mesh poses at the identity rotation too"""
    ot, me, tft, tfm, sw = oc.random_queries(pkg, rng, trees, np.arange(n_meshes, dtype=np.uint32), n, spread, identity_share)
    plain = rng.uniform(size=n) < 0.25
    tfm[plain, :9] = pkg.geometry.make_pose().reshape(-1)[:9]
    return ot, me, tft, tfm, sw
