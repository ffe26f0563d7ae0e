"""fp64 model of OcTree x convex solid collide(): a restatement of the reference in plain Python, the yardstick of
tests/test_octree_cpu.py.  It shares no code with hpp-fcl_amd/csrc/hfcl_octree.hpp.

  the entry       OctreeCollide                                          src/collision_func_matrix.cpp:52-75
  the set-up      OcTreeShapeIntersect, convertBV<AABB, OBB>             internal/traversal_node_octree.h:183-197, BV/BV.h:79-84
  the walk        OcTreeShapeIntersectRecurse                            internal/traversal_node_octree.h:299-369
  the boxes       getRootBV, computeChildBV                              include/hpp/fcl/octree.h:139-144, 299-324
  the box test    OBB::overlap(other, request, sqr),
                  obbDisjointAndLowerBoundDistance                       src/BV/OBB.cpp:290-392, 405-423
  a leaf          constructBox, ShapeShapeCollider<Box, S>::run          src/shape/geometric_shapes_utility.cpp:1052-1056,
                                                                         internal/shape_shape_func.h:132-164
  the contact     Contact(o1, o2, b1, b2, pos, normal, depth)            collision_data.h:126-148
  the bounds      updateDistanceLowerBoundFromBV / FromLeaf              collision_data.h:1177-1197

The tree is a node array (abi.OCTREE_NODE_DTYPE): the reference reaches octomap through getRoot, nodeHasChildren, nodeChildExists /
getNodeChild and getOccupancy only.  The oracle is used for one thing: the Box x solid collide of every reached leaf
(oracle_binding.collide_batch on Box shapes built per leaf; the leaves of a call go into ONE oracle call, no leaf depends on another
under DefaultGuess).  Vectors are tuples of Python floats and every sum of products is written left to right, in the reference's
order.  A reported node is its index in the array (the reference's pointer difference cannot be reproduced)."""
import math

import numpy as np

import oracle_binding as ob

DBL_MAX = float(np.finfo(np.float64).max)
NAN = float("nan")
NAN3 = (NAN, NAN, NAN)
BOX, SPHERE, CAPSULE, CONE, CYLINDER, CONVEX, ELLIPSOID = 9, 10, 11, 12, 13, 14, 19


# ---- vectors -------------------------------------------------------------------------------------------------------------------
def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def pose(row):
    """12 doubles (column-major R, then T) -> (rows of R, T)"""
    p = [float(x) for x in row]
    return ((p[0], p[3], p[6]), (p[1], p[4], p[7]), (p[2], p[5], p[8])), (p[9], p[10], p[11])


def pose_row(R, T):
    return [R[0][0], R[1][0], R[2][0], R[0][1], R[1][1], R[2][1], R[0][2], R[1][2], R[2][2], T[0], T[1], T[2]]


def rot(R, v):
    return (dot(R[0], v), dot(R[1], v), dot(R[2], v))


def col(R, j):
    return (R[0][j], R[1][j], R[2][j])


def rot_t(R, v):
    return (dot(col(R, 0), v), dot(col(R, 1), v), dot(col(R, 2), v))


def mat_t_mat(A, B):
    """A^T B"""
    return tuple(tuple(dot(col(A, i), col(B, j)) for j in range(3)) for i in range(3))


# ---- the tree ------------------------------------------------------------------------------------------------------------------
class Tree:
    def __init__(self, nodes, resolution, depth, occupancy_threshold=0.5, free_threshold=0.0):
        self.children = [[int(c) for c in n["child"]] for n in nodes]
        self.occupancy = [float(n["occupancy"]) for n in nodes]
        self.resolution, self.depth = float(resolution), int(depth)
        self.occupancy_threshold, self.free_threshold = float(occupancy_threshold), float(free_threshold)

    def root_bv(self):
        delta = (1 << self.depth) * self.resolution / 2
        return (-delta, -delta, -delta), (delta, delta, delta)

    def is_occupied(self, i):
        return self.occupancy[i] >= self.occupancy_threshold

    def is_free(self, i):
        return self.occupancy[i] <= self.free_threshold

    def is_uncertain(self, i):
        return (not self.is_occupied(i)) and (not self.is_free(i))

    def has_children(self, i):
        return any(self.children[i])

    def to_boxes(self):
        """toBoxes(): (x, y, z, size, occupancy, threshold) of the occupied leaves, in the order of a depth-first walk with the children
        in index order; centre and size from the halved boxes (size: along x)"""
        out = []
        if not self.children:
            return out

        def rec(i, lo, hi):
            if not self.has_children(i):
                if self.is_occupied(i):
                    out.append(((lo[0] + hi[0]) * 0.5, (lo[1] + hi[1]) * 0.5, (lo[2] + hi[2]) * 0.5, hi[0] - lo[0], self.occupancy[i],
                                self.occupancy_threshold, i, lo, hi))
                return
            for k in range(8):
                if self.children[i][k]:
                    clo, chi = child_bv(lo, hi, k)
                    rec(self.children[i][k], clo, chi)

        rec(0, *self.root_bv())
        return out


def child_bv(lo, hi, i):
    """computeChildBV"""
    clo, chi = list(lo), list(hi)
    for axis in range(3):
        if i & (1 << axis):
            clo[axis] = (lo[axis] + hi[axis]) * 0.5
        else:
            chi[axis] = (lo[axis] + hi[axis]) * 0.5
    return tuple(clo), tuple(chi)


# ---- the solid's local box: computeBV<AABB, S>(s, Transform3f()) ---------------------------------------------------------------------
def solid_local_box(srow, verts):
    """src/shape/geometric_shapes_utility.cpp:292-382 at the identity pose (the signs of zero aside); a swept-sphere radius widens
    it, as computeLocalAABB does"""
    k = int(srow["type"])
    p = [float(x) for x in srow["params"]]
    if k in (BOX, ELLIPSOID):
        h = (p[0], p[1], p[2])
    elif k == SPHERE:
        h = (p[0], p[0], p[0])
    elif k == CAPSULE:
        h = (p[0], p[0], p[1] + p[0])
    elif k in (CONE, CYLINDER):
        h = (abs(p[0]), abs(p[0]), abs(p[1]))
    elif k == CONVEX:
        v = verts[int(srow["vertex_offset"]):int(srow["vertex_offset"]) + int(srow["num_points"])]
        lo, hi = tuple(float(x) for x in v.min(axis=0)), tuple(float(x) for x in v.max(axis=0))
        h = None
    else:
        raise ValueError("no octree row for node type %d" % k)
    if h is not None:
        lo, hi = (-h[0], -h[1], -h[2]), h
    r = float(srow["swept_sphere_radius"])
    if r > 0:
        lo, hi = (lo[0] - r, lo[1] - r, lo[2] - r), (hi[0] + r, hi[1] + r, hi[2] + r)
    return lo, hi


def convert_bv(lo, hi, tf):
    """Converter<AABB, OBB>: (To, extent, axes)"""
    R, T = tf
    center = ((lo[0] + hi[0]) * 0.5, (lo[1] + hi[1]) * 0.5, (lo[2] + hi[2]) * 0.5)
    To = add(rot(R, center), T)
    extent = ((hi[0] - lo[0]) * 0.5, (hi[1] - lo[1]) * 0.5, (hi[2] - lo[2]) * 0.5)
    return To, extent, R


# ---- obbDisjointAndLowerBoundDistance ----------------------------------------------------------------------------------------------
def obb_disjoint_lb(B, T, a_, b_, margin, bd2):
    """(disjoint, squaredLowerBoundDistance)"""
    Bf = tuple(tuple(abs(x) for x in row) for row in B)
    a = tuple(max(x + margin / 2, 0.0) for x in a_)
    b = tuple(max(x + margin / 2, 0.0) for x in b_)
    # obbDisjoint_check_A_axis: (|T| - a) - Bf b, clamped at 0, squared norm
    c = [abs(T[i]) - a[i] for i in range(3)]
    Bfb = rot(Bf, b)
    c = [max(c[i] - Bfb[i], 0.0) for i in range(3)]
    sq = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
    if sq > bd2:
        return True, sq
    # obbDisjoint_check_B_axis
    t = 0.0
    for j in range(3):
        s = abs(dot(col(B, j), T)) - dot(col(Bf, j), a) - b[j]
        if s > 0:
            t += s * s
    sq = t
    if sq > bd2:
        return True, sq
    ja, ka = 1, 2
    for ia in range(3):
        for ib in range(3):
            jb, kb = (ib + 1) % 3, (ib + 2) % 3
            sinus2 = 1 - Bf[ia][ib] * Bf[ia][ib]
            if sinus2 < 1e-6:
                continue
            s = T[ka] * B[ja][ib] - T[ja] * B[ka][ib]
            diff = abs(s) - (a[ja] * Bf[ka][ib] + a[ka] * Bf[ja][ib] + b[jb] * Bf[ia][kb] + b[kb] * Bf[ia][jb])
            if diff > 0:
                sq = diff * diff / sinus2
                if sq > bd2:
                    return True, sq
        ja, ka = ka, ia
    return False, sq


def obb_overlap(obb1, obb2, margin, bd2):
    """OBB::overlap(other, request, sqrDistLowerBound) of obb1: (overlap, sqr)"""
    To1, ext1, ax1 = obb1
    To2, ext2, ax2 = obb2
    T = rot_t(ax1, sub(To2, To1))
    R = mat_t_mat(ax1, ax2)
    disjoint, sq = obb_disjoint_lb(R, T, ext1, ext2, margin, bd2)
    return not disjoint, sq


# ---- the walk ------------------------------------------------------------------------------------------------------------------
def walk(tree, tf_tree, obb2, margin, bd2):
    """OcTreeShapeIntersectRecurse without the leaves' solves (the box tests do not depend on them): the events in order,
    ("box", bound) for a disjoint node and ("leaf", node, lo, hi) for a leaf that is reached"""
    events = []
    if not tree.children:  # `if (!root1) return false`
        return events

    def rec(i, lo, hi):
        if tree.is_free(i):
            return
        if tree.is_uncertain(i):
            return
        obb1 = convert_bv(lo, hi, tf_tree)
        overlap, sq = obb_overlap(obb1, obb2, margin, bd2)
        if not overlap:
            events.append(("box", math.sqrt(sq)))
            return
        if not tree.has_children(i):
            events.append(("leaf", i, lo, hi))
            return
        for k in range(8):
            if tree.children[i][k]:
                clo, chi = child_bv(lo, hi, k)
                rec(tree.children[i][k], clo, chi)

    rec(0, *tree.root_bv())
    return events


# ---- collide() -----------------------------------------------------------------------------------------------------------------
def collide(trees, octree, shapes, verts, shape, tf_octree, tf_shape, req, swapped=None, near=1e-9):
    """trees: list of Tree; octree / shape: ids per query; tf_*: (n, 12) pose rows; req: abi.CollisionRequest.
    Returns (records, bounds, contacts, near_threshold): dicts per query, the distance_lower_bound per query, the contact list (dicts, in
    query order and within a query in walk order), and per query whether a leaf's distance - margin lay within `near` of the
    threshold.  swapped[i]: the caller's order was (solid, octree) -- the reference answers with the octree-first result, so it only
    marks the record."""
    pkg_abi = ob._pkg().abi
    n = len(shape)
    margin, thr = float(req.security_margin), float(req.q.collision_distance_threshold)
    if req.num_max_contacts == 0:
        raise ValueError("Invalid number of max contacts (current value is 0).")
    skip_all = margin == -math.inf
    if margin < 0 and not skip_all:
        raise ValueError("Negative security margin are not handled yet for Octree")
    bd2 = float(req.break_distance) * float(req.break_distance)
    nmax = int(req.num_max_contacts)
    verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
    walks, jobs, box_rows, box_tfs = [], [], [], []
    for i in range(n):
        if skip_all:
            walks.append(None)
            continue
        tree = trees[int(octree[i])]
        tft, tfs = pose(tf_octree[i]), pose(tf_shape[i])
        lo, hi = solid_local_box(shapes[int(shape[i])], verts)
        obb2 = convert_bv(lo, hi, tfs)
        ev = walk(tree, tft, obb2, margin, bd2)
        walks.append(ev)
        for e in ev:
            if e[0] != "leaf":
                continue
            _, node, blo, bhi = e
            side = sub(bhi, blo)  # Box(bv.max_ - bv.min_): halfSide = side / 2
            center = ((blo[0] + bhi[0]) * 0.5, (blo[1] + bhi[1]) * 0.5, (blo[2] + bhi[2]) * 0.5)
            R, T = tft
            box_rows.append((side[0] / 2, side[1] / 2, side[2] / 2))
            box_tfs.append(pose_row(R, add(rot(R, center), T)))  # tf * Transform3f(center)
            jobs.append((i, node))
    leaf = {}
    if jobs:
        all_shapes = np.zeros(len(shapes) + len(box_rows), dtype=pkg_abi.SHAPE_DTYPE)
        all_shapes[:len(shapes)] = shapes
        for k, h in enumerate(box_rows):
            row = all_shapes[len(shapes) + k]
            row["type"] = BOX
            row["params"][:3] = h
        one = pkg_abi.CollisionRequest.from_buffer_copy(bytes(req))
        one.num_max_contacts = 1
        s1 = np.arange(len(shapes), len(shapes) + len(jobs), dtype=np.uint32)
        s2 = np.array([int(shape[j[0]]) for j in jobs], dtype=np.uint32)
        q = np.array([j[0] for j in jobs])
        res = ob.collide_batch(all_shapes, verts if len(verts) else np.zeros((1, 3)), s1, s2, np.asarray(box_tfs, dtype=np.float64),
                               np.asarray(tf_shape, dtype=np.float64).reshape(-1, 12)[q], one, n_threads=8)
        for (i, node), r in zip(jobs, res):
            leaf[(i, node)] = r
    records, bounds, contacts, near_flags = [], [], [], []
    for i in range(n):
        sw = bool(swapped[i]) if swapped is not None else False
        if skip_all:
            records.append(dict(skipped=True, swapped=sw))
            bounds.append(DBL_MAX)
            near_flags.append(False)
            continue
        dlb, np1, np2, nn = DBL_MAX, NAN3, NAN3, NAN3
        mine = []
        flag = False
        for e in walks[i]:
            if e[0] == "box":  # updateDistanceLowerBoundFromBV
                if dlb <= 0:
                    continue
                if e[1] < dlb:
                    dlb = e[1]
                continue
            node = e[1]
            r = leaf[(i, node)]
            distance = float(r["distance"])
            p1, p2, normal = (tuple(float(x) for x in r[k]) for k in ("p1", "p2", "normal"))
            dtc = distance - margin
            if abs(dtc - thr) < near:
                flag = True
            if dtc < dlb:  # updateDistanceLowerBoundFromLeaf
                dlb, np1, np2, nn = dtc, p1, p2, normal
            if dtc <= thr and len(mine) < nmax:
                pos = ((p1[0] + p2[0]) / 2, (p1[1] + p2[1]) / 2, (p1[2] + p2[2]) / 2)  # Contact(o1, o2, NONE, NONE, p1, p2, normal, distance)
                h = (distance * normal[0] / 2, distance * normal[1] / 2, distance * normal[2] / 2)  # ... rebuilt with b1 = the node
                mine.append(dict(pair=i, node=node, b1=node, b2=-1, depth=distance, normal=normal, p1=sub(pos, h), p2=add(pos, h)))
            if len(mine) >= nmax:  # isSatisfied()
                break
        if mine:
            f = mine[0]
            rec = dict(distance=f["depth"], normal=f["normal"], p1=f["p1"], p2=f["p2"], b1=f["b1"], b2=f["b2"])
        else:
            rec = dict(distance=dlb, normal=nn, p1=np1, p2=np2, b1=-1, b2=-1)
        rec.update(num_contacts=len(mine), skipped=False, swapped=sw)
        records.append(rec)
        bounds.append(dlb)
        contacts.extend(mine)
        near_flags.append(flag)
    return records, bounds, contacts, near_flags
