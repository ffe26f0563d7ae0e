"""Shared pieces of the octree tests (tests/test_octree_cpu.py, tests/test_octree_gpu.py): the host build of the device header
(tests/octree_harness), hand-made and seeded random trees as node arrays, seeded random queries."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_FIELDS = ("distance", "normal", "p1", "p2")
FREE, UNCERTAIN, OCCUPIED = 0.0, 0.3, 0.8  # against the default thresholds 0 / 0.5


# ---- the host build of the device header ---------------------------------------------------------------------------------------
def build_harness(out_dir):
    """the g++ line of hfield_cases.build_harness"""
    out = os.path.join(str(out_dir), "liboctree_harness.so")
    src = os.path.join(ROOT, "tests", "octree_harness", "octree_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-shared", "-o", out, src])
    return C.CDLL(out)


class HarnessTrees:
    """the tables of several trees one after the other, as the library keeps them.  trees: [(nodes, resolution, depth, occupancy_threshold,
    free_threshold)]"""

    def __init__(self, pkg, trees):
        self.n = len(trees)
        off, table, params, nodes = 0, [], [], []
        for t in trees:
            n, res, depth = t[0], t[1], t[2]
            occ, free = (t[3], t[4]) if len(t) > 3 else (0.5, 0.0)
            table.append([off, len(n)])
            params.append([res, float(depth), occ, free])
            nodes.append(np.ascontiguousarray(n, dtype=pkg.abi.OCTREE_NODE_DTYPE))
            off += len(n)
        self.table = np.array(table, dtype=np.uint64)
        self.params = np.array(params, dtype=np.float64)
        self.nodes = np.concatenate(nodes + [np.zeros(1, dtype=pkg.abi.OCTREE_NODE_DTYPE)])  # (never empty: a pointer to pass)


def harness_collide(pkg, oh, ht, L, octree, shape, tft, tfs, req, swapped=None, cap=0):
    """(records, bounds, contacts, n_produced, n_items) of the harness"""
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
    dlb = np.zeros(n)
    contacts = np.zeros(max(cap, 1), dtype=abi.CONTACT_DTYPE)
    nc, ni = C.c_size_t(0), C.c_size_t(0)
    sw = None if swapped is None else np.ascontiguousarray(swapped, dtype=np.uint8)
    rc = oh.oh_collide(abi.ptr(shapes), C.c_uint32(len(shapes)), abi.ptr(verts), C.c_uint32(ht.n), abi.ptr(ht.table), abi.ptr(ht.params),
                       abi.ptr(ht.nodes), abi.ptr(octree), abi.ptr(shape), abi.ptr(tft), abi.ptr(tfs), C.c_size_t(n), abi.ptr(sw),
                       C.byref(req), abi.ptr(out), abi.ptr(dlb), abi.ptr(contacts), C.c_size_t(cap), C.byref(nc), None, C.c_size_t(0),
                       C.byref(ni))
    assert rc == 0
    return out, dlb, contacts[:min(nc.value, cap)], int(nc.value), int(ni.value)


def compare_records(got, want, fields=FLOAT_FIELDS + ("b1", "b2", "status", "num_contacts")):
    """names of the fields in which two record arrays differ in any byte"""
    return [k for k in fields if got[k].tobytes() != want[k].tobytes()]


# ---- trees as node arrays ----------------------------------------------------------------------------------------------------------
def tree_from_spec(pkg, spec):
    """spec: a float (a leaf of that occupancy) or (occupancy, {child index: spec}); nodes in depth-first preorder"""
    rows = []

    def rec(s):
        i = len(rows)
        rows.append(None)
        if isinstance(s, tuple):
            occ, kids = s
            child = [0] * 8
            for k in sorted(kids):
                child[k] = rec(kids[k])
        else:
            occ, child = s, [0] * 8
        rows[i] = (child, occ)
        return i

    rec(spec)
    return np.array(rows, dtype=pkg.abi.OCTREE_NODE_DTYPE)


def empty_tree(pkg):
    return np.zeros(0, dtype=pkg.abi.OCTREE_NODE_DTYPE)


def three_state_tree(pkg):
    """depth 2: under the root a free, an uncertain and an occupied leaf, an occupied inner node with two occupied leaves, and an inner
    node BELOW the threshold whose children are occupied (never reached)"""
    return tree_from_spec(pkg, (OCCUPIED, {0: FREE, 1: UNCERTAIN, 2: OCCUPIED, 5: (OCCUPIED, {0: OCCUPIED, 7: 0.9}),
                                           6: (UNCERTAIN, {1: OCCUPIED, 2: OCCUPIED})}))


def random_tree(pkg, rng, depth, p_child=0.45, p_leaf=0.35, states=(OCCUPIED, OCCUPIED, OCCUPIED, 0.97, UNCERTAIN, FREE)):
    """leaves at mixed levels: below the root a child exists with probability p_child and, above the last level, is a leaf with
    probability p_leaf; a leaf draws its occupancy from `states`, an inner node takes the maximum of its children (as octomap's
    updateInnerOccupancy)"""
    def rec(level):
        if level == depth or (level > 0 and rng.uniform() < p_leaf):
            return float(states[rng.integers(0, len(states))])
        kids = {k: rec(level + 1) for k in range(8) if rng.uniform() < p_child}
        if not kids:
            kids = {int(rng.integers(0, 8)): rec(level + 1)}
        return (max(v[0] if isinstance(v, tuple) else v for v in kids.values()), kids)

    return tree_from_spec(pkg, rec(0))


def chain_tree(pkg, depth=16):
    """one chain of child 7, 0, 7, 0 ... down to a single voxel at level `depth`, with an occupied sibling leaf at a few levels"""
    spec = OCCUPIED
    for level in range(depth - 1, -1, -1):
        k = 7 if level % 2 == 0 else 0
        kids = {k: spec}
        if level in (1, 6, 15):
            kids[3] = OCCUPIED
        spec = (OCCUPIED, kids)
    return tree_from_spec(pkg, spec)


def block_tree(pkg):
    """depth 4: a full 8 x 8 x 8 block of occupied voxels in the octant of child 0 (three full levels under it)"""
    def full(levels):
        return OCCUPIED if levels == 0 else (OCCUPIED, {k: full(levels - 1) for k in range(8)})

    return tree_from_spec(pkg, (OCCUPIED, {0: full(3)}))


def leaf_boxes(nodes, resolution, depth, occupancy_threshold=0.5, free_threshold=0.0):
    """(node, lo, hi) of the leaves a walk can reach (every node of the path occupied), boxes by halving from the root"""
    out = []
    if len(nodes) == 0:
        return out
    d = (1 << depth) * resolution / 2

    def rec(i, lo, hi):
        occ = float(nodes[i]["occupancy"])
        if occ <= free_threshold or not occ >= occupancy_threshold:
            return
        kids = [int(c) for c in nodes[i]["child"]]
        if not any(kids):
            out.append((i, lo, hi))
            return
        for k in range(8):
            if kids[k]:
                clo, chi = list(lo), list(hi)
                for a in range(3):
                    if k & (1 << a):
                        clo[a] = (lo[a] + hi[a]) * 0.5
                    else:
                        chi[a] = (lo[a] + hi[a]) * 0.5
                rec(kids[k], clo, chi)

    rec(0, [-d] * 3, [d] * 3)
    return out


# ---- seeded random queries --------------------------------------------------------------------------------------------------------
def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def seven_solids(pkg, rng, scale=1.0):
    """a shape library with one solid of each kind an octree collides with (the box carries a swept-sphere radius)"""
    L = pkg.geometry.ShapeLibrary()
    s = scale
    pts = rng.normal(size=(14, 3))
    pts = 0.12 * s * pts / np.linalg.norm(pts, axis=1, keepdims=True) * rng.uniform(0.7, 1.0, (14, 1))
    ids = [L.add_box(0.16 * s, 0.12 * s, 0.2 * s, 0.01 * s), L.add_sphere(0.1 * s), L.add_capsule(0.06 * s, 0.16 * s), L.add_cone(0.08 * s, 0.2 * s),
           L.add_cylinder(0.08 * s, 0.16 * s), L.add_ellipsoid(0.12 * s, 0.08 * s, 0.06 * s), L.add_convex(pts)]
    return L, np.array(ids, dtype=np.uint32)


def random_queries(pkg, rng, trees, solid_ids, n, spread=0.7, identity_share=1.0 / 3.0):
    """n queries: solids near a reachable leaf of a tree (about half in contact), trees under rotated and translated poses (a share at the
    identity), both operand orders.  trees: [(nodes, resolution, depth, ...)]; a tree without a reachable leaf gets solids near its
    origin"""
    geo = pkg.geometry
    boxes = [leaf_boxes(*t[:3], *t[3:5]) for t in trees]
    octree = rng.integers(0, len(trees), n).astype(np.uint32)
    shape = solid_ids[rng.integers(0, len(solid_ids), n)]
    tft = geo.make_pose(quat=random_rotations(rng, n), T=rng.uniform(-2.0, 2.0, (n, 3)))
    ident = rng.uniform(size=n) < identity_share
    tft[ident] = geo.make_pose()
    local = np.zeros((n, 3))
    for i in range(n):
        b = boxes[int(octree[i])]
        if b:
            _, lo, hi = b[int(rng.integers(0, len(b)))]
            lo, hi = np.array(lo), np.array(hi)
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            local[i] = 0.5 * (lo + hi) + d * (0.5 * (hi - lo).max() + rng.uniform(0.0, spread))
        else:
            local[i] = rng.uniform(-0.3, 0.3, 3)
    world = geo.transform_point(tft, local)
    tfs = geo.make_pose(quat=random_rotations(rng, n), T=world)
    swapped = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    return octree, shape, tft, tfs, swapped
