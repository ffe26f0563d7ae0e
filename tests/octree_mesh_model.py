"""fp64 model of OcTree x BVHModel<OBBRSS> collide(): a restatement of the reference in plain Python, the yardstick of
tests/test_octree_mesh_cpu.py.  It shares no code with hpp-fcl_amd/csrc/hfcl_octree_mesh.hpp; of tests/octree_model.py it takes the
tree, computeChildBV, Converter<AABB, OBB> and OBB::overlap.

  the entry       OctreeCollide                                          src/collision_func_matrix.cpp:52-75
  the set-up      OcTreeMeshIntersect / MeshOcTreeIntersect              internal/traversal_node_octree.h:100-139
  the walk        OcTreeMeshIntersectRecurse                             internal/traversal_node_octree.h:462-563
  the mesh's box  Converter<OBBRSS, OBB>                                 BV/BV.h:94-113
  the sizes       AABB::size() (the FULL diagonal squared), OBBRSS::size() (the HALF extents squared)
                                                                         BV/AABB.h:162, BV/OBB.h:110, BV/OBBRSS.h:114
  a leaf          constructBox, ShapeShapeDistance<Box, TriangleP>       src/shape/geometric_shapes_utility.cpp:1052-1056
  the contact     Contact(o1, o2, b1, b2, c1, c2, normal, distance)      collision_data.h:138-148
  the bounds      updateDistanceLowerBoundFromBV / FromLeaf              collision_data.h:1177-1197

The mesh is the oracle's (oracle_binding.bvh_build).  The oracle is used for one more thing: the Box x TriangleP solve of every reached
(leaf, triangle) pair -- all of a call in ONE oracle_binding.collide_batch on Box rows and GEOM_TRIANGLE rows with num_max_contacts = 1,
whose record is ShapeShapeDistance<Box, TriangleP>'s distance, points and normal.  No leaf depends on another under DefaultGuess."""
import math

import numpy as np

import octree_model as om
import oracle_binding as ob

DBL_MAX, NAN3 = om.DBL_MAX, om.NAN3
BOX, TRIANGLE = 9, 17


class Mesh:
    """vertices, triangles and the node array of BVHModel<OBBRSS>::endModel() as the oracle builds it"""

    def __init__(self, vertices, triangles, nodes=None):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.triangles = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        self.nodes = ob.bvh_build(self.vertices, self.triangles)[0] if nodes is None else nodes
        self.first_child = [int(x) for x in self.nodes["first_child"]]
        self.To = [tuple(float(x) for x in r) for r in self.nodes["obb_To"]]
        self.extent = [tuple(float(x) for x in r) for r in self.nodes["obb_extent"]]
        # obb_axes: column-major; kept as rows
        self.axes = [tuple(tuple(float(r[3 * c + k]) for c in range(3)) for k in range(3)) for r in self.nodes["obb_axes"]]

    def depth(self):
        """levels of the BVH, the root being level 1"""
        best, todo = 0, [(0, 1)]
        while todo:
            i, d = todo.pop()
            best = max(best, d)
            if self.first_child[i] > 0:
                todo += [(self.first_child[i], d + 1), (self.first_child[i] + 1, d + 1)]
        return best


def mat_mat(A, B):
    """A B, every entry summed left to right"""
    return tuple(tuple(A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)) for i in range(3))


def convert_obbrss(mesh, node, tf):
    """Converter<OBBRSS, OBB>: (To, extent, axes) -- the RSS half is not read"""
    R, T = tf
    return om.add(om.rot(R, mesh.To[node]), T), mesh.extent[node], mat_mat(R, mesh.axes[node])


def sq_norm(v):
    return v[0] * v[0] + v[1] * v[1] + v[2] * v[2]


def walk(tree, tf_tree, mesh, tf_mesh, margin, bd2, same_quantity=False):
    """OcTreeMeshIntersectRecurse without the leaves' solves (the box tests do not depend on them): the events in order, ("box", bound)
    for a disjoint pair of nodes and ("leaf", node, lo, hi, triangle) for a reached pair of leaves.  same_quantity: NOT the reference --
    the descent rule with the octree box's half extents squared, for the test that pins the reference's rule"""
    events = []
    if not tree.children:  # `if (!root1) return false`
        return events

    def rec(i, lo, hi, j):
        if tree.is_free(i):
            return
        if tree.is_uncertain(i):  # (tree2->isUncertain() is false for a mesh)
            return
        overlap, sq = om.obb_overlap(om.convert_bv(lo, hi, tf_tree), convert_obbrss(mesh, j, tf_mesh), margin, bd2)
        if not overlap:
            events.append(("box", math.sqrt(sq)))
            return
        fc = mesh.first_child[j]
        if not tree.has_children(i) and fc < 0:
            events.append(("leaf", i, lo, hi, -(fc + 1)))
            return
        size1 = sq_norm(om.sub(hi, lo))  # AABB::size()
        if same_quantity:
            size1 = sq_norm(om.scale(om.sub(hi, lo), 0.5))
        if fc < 0 or (tree.has_children(i) and size1 > sq_norm(mesh.extent[j])):
            for k in range(8):
                if tree.children[i][k]:
                    clo, chi = om.child_bv(lo, hi, k)
                    rec(tree.children[i][k], clo, chi, j)
        else:
            rec(i, lo, hi, fc)
            rec(i, lo, hi, fc + 1)

    rec(0, *tree.root_bv(), 0)
    return events


def collide(trees, octree, meshes, mesh, tf_octree, tf_mesh, req, swapped=None, near=1e-9):
    """trees: list of octree_model.Tree; meshes: list of Mesh; octree / mesh: ids per query; tf_*: (n, 12) pose rows; req:
    abi.CollisionRequest.  Returns (records, bounds, contacts, near_threshold, items): dicts per query, the distance_lower_bound per
    query at the moment the walk stops, the contact list (dicts, in query order and within a query in walk order), per query whether a
    leaf's distance - margin lay within `near` of the threshold, and the listed (query, node, triangle) of every query in walk order.
    swapped[i]: the caller's order was (mesh, octree) -- the reference answers with the octree-first result, so it only marks the
    record."""
    pkg_abi = ob._pkg().abi
    n = len(mesh)
    margin, thr = float(req.security_margin), float(req.q.collision_distance_threshold)
    if req.num_max_contacts == 0:
        raise ValueError("Invalid number of max contacts (current value is 0).")
    skip_all = margin == -math.inf
    if margin < 0 and not skip_all:
        raise ValueError("Negative security margin are not handled yet for Octree")
    bd2 = float(req.break_distance) * float(req.break_distance)
    nmax = int(req.num_max_contacts)
    walks, jobs, box_rows, box_tfs, tri_pts, items = [], [], [], [], [], []
    for i in range(n):
        if skip_all:
            walks.append(None)
            continue
        tree, me = trees[int(octree[i])], meshes[int(mesh[i])]
        tft, tfm = om.pose(tf_octree[i]), om.pose(tf_mesh[i])
        ev = walk(tree, tft, me, tfm, margin, bd2)
        walks.append(ev)
        for e in ev:
            if e[0] != "leaf":
                continue
            _, node, blo, bhi, prim = e
            side = om.sub(bhi, blo)  # Box(bv.max_ - bv.min_): halfSide = side / 2
            center = ((blo[0] + bhi[0]) * 0.5, (blo[1] + bhi[1]) * 0.5, (blo[2] + bhi[2]) * 0.5)
            R, T = tft
            box_rows.append((side[0] / 2, side[1] / 2, side[2] / 2))
            box_tfs.append(om.pose_row(R, om.add(om.rot(R, center), T)))  # tf * Transform3f(center)
            tri_pts.append(me.vertices[me.triangles[prim]])
            jobs.append((i, node, prim))
            items.append((i, node, prim))
    leaf = {}
    if jobs:
        m = len(jobs)
        shapes = np.zeros(2 * m, dtype=pkg_abi.SHAPE_DTYPE)
        shapes["type"][:m] = BOX
        shapes["params"][:m, :3] = np.asarray(box_rows)
        shapes["type"][m:] = TRIANGLE
        shapes["num_points"][m:] = 3
        shapes["vertex_offset"][m:] = 3 * np.arange(m)
        verts = np.ascontiguousarray(np.concatenate(tri_pts), dtype=np.float64)
        one = pkg_abi.CollisionRequest.from_buffer_copy(bytes(req))
        one.num_max_contacts = 1
        q = np.array([j[0] for j in jobs])
        res = ob.collide_batch(shapes, verts, np.arange(m, dtype=np.uint32), np.arange(m, 2 * m, dtype=np.uint32),
                               np.asarray(box_tfs, dtype=np.float64), np.asarray(tf_mesh, dtype=np.float64).reshape(-1, 12)[q], one, n_threads=8)
        for j, r in zip(jobs, res):
            leaf[j] = r
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
            node, prim = e[1], e[4]
            r = leaf[(i, node, prim)]
            distance = float(r["distance"])
            c1, c2, normal = (tuple(float(x) for x in r[k]) for k in ("p1", "p2", "normal"))
            dtc = distance - margin
            if abs(dtc - thr) < near:
                flag = True
            if dtc < dlb:  # updateDistanceLowerBoundFromLeaf
                dlb, np1, np2, nn = dtc, c1, c2, normal
            if len(mine) < nmax and dtc <= thr:  # the eight-argument Contact: nearest_points = {c1, c2}
                mine.append(dict(pair=i, node=node, b1=node, b2=prim, depth=distance, normal=normal, p1=c1, p2=c2))
            if len(mine) >= nmax:  # isSatisfied(): `true` ends the whole walk
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
    return records, bounds, contacts, near_flags, items
