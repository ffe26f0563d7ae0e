"""fp64 model of OcTree x convex solid distance(): a restatement of the reference in plain Python, the yardstick of
tests/test_octree_distance_cpu.py.  It shares no code with hpp-fcl_amd/csrc/hfcl_octree_distance.hpp.

  the entry        OcTreeShapeDistance / ShapeOcTreeDistance                 internal/traversal_node_octree.h:216-244
  the walk         OcTreeShapeDistanceRecurse                                internal/traversal_node_octree.h:246-297
  the solid's box  computeBV<AABB, S>(solid, tf_solid)                       hfield_model.solid_world_box (the Ellipsoid's R * radii as it is)
  a child's box    computeChildBV, Converter<AABB, AABB>::convert            include/hpp/fcl/octree.h:299-324, BV/BV.h:66-73
  the box distance AABB::distance                                            src/BV/AABB.cpp:115-133
  a leaf           constructBox, ShapeShapeDistance<Box, S>                  src/shape/geometric_shapes_utility.cpp:1052-1056
  the result       DistanceResult::update, DistanceRequest::isSatisfied      collision_data.h:1111-1124

The oracle is used for one thing: the Box x solid distance of every reachable occupied leaf of a call (oracle_binding.distance_batch on
Box shapes built per leaf, ONE oracle call; no leaf depends on another under DefaultGuess).  The recursion is then replayed with those
distances: which leaves it solves hangs on the running minimum, so the answer is the ordered walk's, not the minimum over the leaves.
Vectors are tuples of Python floats and every sum of products is written left to right."""
import math

import numpy as np

import oracle_binding as ob
from hfield_model import solid_world_box
from octree_model import BOX, DBL_MAX, NAN3, Tree, add, child_bv, pose, pose_row, rot, sub  # noqa: F401

NEAR = 1e-9


def convert_aabb(lo, hi, tf):
    """Converter<AABB, AABB>::convert(bv, tf)"""
    R, T = tf
    center = ((lo[0] + hi[0]) * 0.5, (lo[1] + hi[1]) * 0.5, (lo[2] + hi[2]) * 0.5)
    e = sub(hi, lo)
    r = math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) * 0.5
    c2 = add(rot(R, center), T)
    return (c2[0] - r, c2[1] - r, c2[2] - r), (c2[0] + r, c2[1] + r, c2[2] + r)


def aabb_distance(a, b):
    """AABB::distance"""
    result = 0.0
    for i in range(3):
        amin, amax, bmin, bmax = a[0][i], a[1][i], b[0][i], b[1][i]
        if amin > bmax:
            delta = bmax - amin
            result += delta * delta
        elif bmin > amax:
            delta = amax - bmin
            result += delta * delta
    return math.sqrt(result)


def reachable_leaves(tree):
    """(node, lo, hi) of the occupied leaves below occupied nodes only, depth first with the children in index order"""
    out = []
    if not tree.children:
        return out

    def rec(i, lo, hi):
        if not tree.is_occupied(i):
            return
        if not tree.has_children(i):
            out.append((i, lo, hi))
            return
        for k in range(8):
            if tree.children[i][k]:
                rec(tree.children[i][k], *child_bv(lo, hi, k))

    rec(0, *tree.root_bv())
    return out


def replay(tree, tft, aabb2, leaf):
    """OcTreeShapeDistanceRecurse with the leaves' answers given: leaf[node] = (distance, p1, p2, normal).
    Returns (min_distance, p1, p2, normal, b1, visited, near)"""
    st = dict(min=DBL_MAX, p1=NAN3, p2=NAN3, normal=NAN3, b1=-1, visited=0, near=False)
    if not tree.children:  # a choice: the untouched DistanceResult (the reference dereferences a null root)
        return st

    def rec(i, lo, hi):
        if not tree.has_children(i):
            if tree.is_occupied(i):
                d, p1, p2, n = leaf[i]
                st["visited"] += 1
                if abs(d - st["min"]) < NEAR:
                    st["near"] = True
                if st["min"] > d:  # DistanceResult::update
                    st.update(min=d, p1=p1, p2=p2, normal=n, b1=i)
                return st["min"] <= 0  # isSatisfied
            return False
        if not tree.is_occupied(i):
            return False
        for k in range(8):
            c = tree.children[i][k]
            if c:
                clo, chi = child_bv(lo, hi, k)
                d = aabb_distance(convert_aabb(clo, chi, tft), aabb2)
                if abs(d - st["min"]) < NEAR:
                    st["near"] = True
                if d < st["min"]:
                    if rec(c, clo, chi):
                        return True
        return False

    rec(0, *tree.root_bv())
    return st


def distance(trees, octree, shapes, verts, shape, tf_octree, tf_shape, req, swapped=None):
    """trees: list of Tree; octree / shape: ids per query; tf_*: (n, 12) pose rows; req: abi.DistanceRequest (DefaultGuess).
    Returns (records, visited, near, leaves): a dict per query, the number of leaves the walk solved, the `near` flag (a tested box
    distance or a solved leaf's distance lay within 1e-9 of the running minimum at that moment), and per query the (node, distance) of
    every reachable occupied leaf in depth-first order (what a brute-force minimum runs over)."""
    abi = ob._pkg().abi
    n = len(shape)
    verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
    cache = {}
    jobs, box_rows, box_tfs = [], [], []
    for i in range(n):
        t = int(octree[i])
        if t not in cache:
            cache[t] = reachable_leaves(trees[t])
        R, T = pose(tf_octree[i])
        for node, lo, hi in cache[t]:
            side = sub(hi, lo)  # Box(bv.max_ - bv.min_): halfSide = side / 2
            center = ((lo[0] + hi[0]) * 0.5, (lo[1] + hi[1]) * 0.5, (lo[2] + hi[2]) * 0.5)
            box_rows.append((side[0] / 2, side[1] / 2, side[2] / 2))
            box_tfs.append(pose_row(R, add(rot(R, center), T)))  # tf * Transform3f(center)
            jobs.append((i, node))
    per_query = [dict() for _ in range(n)]
    if jobs:
        # one Box shape per distinct half side (the boxes of a level are the same numbers more often than not)
        sides = {}
        for h in box_rows:
            sides.setdefault(h, len(sides))
        all_shapes = np.zeros(len(shapes) + len(sides), dtype=abi.SHAPE_DTYPE)
        all_shapes[:len(shapes)] = shapes
        for h, k in sides.items():
            row = all_shapes[len(shapes) + k]
            row["type"] = BOX
            row["params"][:3] = h
        s1 = np.array([len(shapes) + sides[h] for h in box_rows], dtype=np.uint32)
        s2 = np.array([int(shape[j[0]]) for j in jobs], dtype=np.uint32)
        q = np.array([j[0] for j in jobs])
        res = ob.distance_batch(all_shapes, verts if len(verts) else np.zeros((1, 3)), s1, s2, np.asarray(box_tfs, dtype=np.float64),
                                np.asarray(tf_shape, dtype=np.float64).reshape(-1, 12)[q], req, n_threads=8)
        dist, p1, p2, nrm = res["distance"].tolist(), res["p1"].tolist(), res["p2"].tolist(), res["normal"].tolist()
        for k, (i, node) in enumerate(jobs):
            per_query[i][node] = (dist[k], tuple(p1[k]), tuple(p2[k]), tuple(nrm[k]))
    records, visited, near, leaves = [], [], [], []
    for i in range(n):
        tree = trees[int(octree[i])]
        tft, tfs = pose(tf_octree[i]), pose(tf_shape[i])
        aabb2 = solid_world_box(shapes[int(shape[i])], verts, tfs)
        st = replay(tree, tft, aabb2, per_query[i])
        sw = bool(swapped[i]) if swapped is not None else False
        records.append(dict(distance=st["min"], p1=st["p1"], p2=st["p2"], normal=st["normal"], b1=st["b1"], b2=-1, swapped=sw,
                            contact=st["min"] <= 0))
        visited.append(st["visited"])
        near.append(st["near"])
        leaves.append([(node, per_query[i][node][0]) for node, _, _ in cache[int(octree[i])]])
    return records, visited, near, leaves
