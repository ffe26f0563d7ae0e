"""fp64 model of HeightField<AABB> x convex solid collide(): a restatement of the reference in plain Python, the yardstick of
tests/test_hfield_cpu.py.  It shares no code with hpp-fcl_amd/csrc/hfcl_hfield.hpp.

  the tree        HeightField::init / recursiveBuildTree                 include/hpp/fcl/hfield.h:308-479
  the walk        collisionRecurse                                       src/traversal/traversal_recurse.cpp:44-85
                  BVDisjoints / leafCollides                             internal/traversal_node_hfield_shape.h:560-642
  the box test    overlap(R, T, b1, b2, request, sqr), rotate, translate  src/BV/AABB.cpp:51-73, 141-146; BV/AABB.h:234-253
  the solid's box computeBV<AABB, S>                                     src/shape/geometric_shapes_utility.cpp:292-382
  a leaf          buildConvexTriangles, binCorrection, shapeDistance     internal/traversal_node_hfield_shape.h:121-509
  the bounds      updateDistanceLowerBoundFromBV / FromLeaf              collision_data.h:1177-1197
  the swap        collide(), CollisionResult::swapObjects                src/collision.cpp:52-129

The oracle is used for two things only: the prism x solid distance (oracle_binding.distance_batch on a 6-vertex Convex with signed
distance; every prism of a call goes into ONE oracle call, no leaf depends on another under DefaultGuess) and the solid's support
(oracle_binding.shape_support is getSupport<NoSweptSphere>; the swept sphere is added here as getSupport<WithSweptSphere> does).
Vectors are tuples of Python floats and every sum of three products is written left to right, in the reference's order."""
import math

import numpy as np

import oracle_binding as ob

DBL_MAX = float(np.finfo(np.float64).max)
NAN = float("nan")
NAN3 = (NAN, NAN, NAN)
TOP, BOTTOM, NORTH, EAST, SOUTH, WEST = 1, 1, 2, 4, 8, 16
BOX, SPHERE, CAPSULE, CONE, CYLINDER, CONVEX, ELLIPSOID = 9, 10, 11, 12, 13, 14, 19

# the face tables of buildConvexTriangles
TRIANGLES = (((0, 2, 1), (3, 4, 5), (0, 1, 3), (3, 1, 4), (1, 2, 5), (1, 5, 4), (0, 5, 2), (5, 0, 3)),
             ((2, 1, 0), (3, 4, 5), (0, 1, 3), (3, 1, 4), (0, 5, 2), (0, 3, 5), (1, 2, 5), (4, 1, 2)))


# ---- vectors -------------------------------------------------------------------------------------------------------------------
def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def neg(a):
    return (-a[0], -a[1], -a[2])


def scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def sqnorm(a):
    return dot(a, a)


def norm(a):
    return math.sqrt(sqnorm(a))


def normalized(a):
    z = sqnorm(a)
    if z > 0:
        s = math.sqrt(z)
        return (a[0] / s, a[1] / s, a[2] / s)
    return a


def pose(row):
    """12 doubles (column-major R, then T) -> (rows of R, T)"""
    p = [float(x) for x in row]
    return ((p[0], p[3], p[6]), (p[1], p[4], p[7]), (p[2], p[5], p[8])), (p[9], p[10], p[11])


def rot(R, v):
    return (dot(R[0], v), dot(R[1], v), dot(R[2], v))


def rot_t(R, v):
    return (R[0][0] * v[0] + R[1][0] * v[1] + R[2][0] * v[2], R[0][1] * v[0] + R[1][1] * v[1] + R[2][1] * v[2],
            R[0][2] * v[0] + R[1][2] * v[1] + R[2][2] * v[2])


# ---- the tree ------------------------------------------------------------------------------------------------------------------
def linspaced(n, low, high):
    step = (high - low) / float(n - 1)
    return [high if i == n - 1 else low + float(i) * step for i in range(n)]


class Field:
    def __init__(self, x_dim, y_dim, heights, min_height=0.0):
        h = np.asarray(heights, dtype=np.float64)
        assert h.ndim == 2 and h.shape[0] >= 2 and h.shape[1] >= 2
        self.x_dim, self.y_dim, self.min_height = float(x_dim), float(y_dim), float(min_height)
        self.ny, self.nx = h.shape
        self.heights = [[max(float(v), self.min_height) for v in row] for row in h]
        self.x_grid = linspaced(self.nx, -0.5 * self.x_dim, 0.5 * self.x_dim)
        self.y_grid = linspaced(self.ny, 0.5 * self.y_dim, -0.5 * self.y_dim)
        self.nodes = [None] * (2 * (self.nx - 1) * (self.ny - 1) - 1)
        self.num = 1
        self.max_height = self._build(0, 0, self.nx - 1, 0, self.ny - 1)
        assert self.num == len(self.nodes)

    def _build(self, bv, x_id, x_size, y_id, y_size):
        first_child = 0
        if x_size == 1 and y_size == 1:
            H = self.heights
            mh = max(H[y_id][x_id], H[y_id + 1][x_id], H[y_id][x_id + 1], H[y_id + 1][x_id + 1])
            assert mh > self.min_height, "max_height is lower than min_height"
        else:
            first_child = self.num
            self.num += 2
            if x_size >= y_size:
                half = 1 if x_size == 1 else x_size // 2
                ml = self._build(first_child, x_id, half, y_id, y_size)
                mr = self._build(first_child + 1, x_id + half, x_size - half, y_id, y_size)
            else:
                half = 1 if y_size == 1 else y_size // 2
                ml = self._build(first_child, x_id, x_size, y_id, half)
                mr = self._build(first_child + 1, x_id, x_size, y_id + half, y_size - half)
            mh = max(ml, mr)
        a = (self.x_grid[x_id], self.y_grid[y_id], self.min_height)
        b = (self.x_grid[x_id + x_size], self.y_grid[y_id + y_size], mh)
        faces = 0
        if x_size == 1 and y_size == 1:
            faces = TOP | BOTTOM
            if x_id == 0:
                faces |= WEST
            if y_id == 0:
                faces |= NORTH
            if x_id + 1 == self.nx - 1:
                faces |= EAST
            if y_id + 1 == self.ny - 1:
                faces |= SOUTH
        self.nodes[bv] = dict(first_child=first_child, x_id=x_id, x_size=x_size, y_id=y_id, y_size=y_size, max_height=mh,
                              contact_active_faces=faces, aabb_min=tuple(min(p, q) for p, q in zip(a, b)),
                              aabb_max=tuple(max(p, q) for p, q in zip(a, b)))
        return mh

    def local_aabb(self):
        a = (self.x_grid[0], self.y_grid[0], self.min_height)
        b = (self.x_grid[-1], self.y_grid[-1], self.max_height)
        return tuple(min(p, q) for p, q in zip(a, b)) + tuple(max(p, q) for p, q in zip(a, b))

    def prisms(self, node):
        x0, x1 = self.x_grid[node["x_id"]], self.x_grid[node["x_id"] + 1]
        y0, y1 = self.y_grid[node["y_id"]], self.y_grid[node["y_id"] + 1]
        H, r, c, mh = self.heights, node["y_id"], node["x_id"], self.min_height
        c00, c01, c10, c11 = H[r][c], H[r][c + 1], H[r + 1][c], H[r + 1][c + 1]
        f = node["contact_active_faces"]
        a1 = (f & 1) | (2 if f & WEST else 0) | (8 if f & NORTH else 0)
        a2 = (f & 1) | (8 if f & EAST else 0) | (2 if f & SOUTH else 0)
        p1 = ((x0, y0, mh), (x0, y1, mh), (x1, y0, mh), (x0, y0, c00), (x0, y1, c10), (x1, y0, c01))
        p2 = ((x0, y1, mh), (x1, y1, mh), (x1, y0, mh), (x0, y1, c10), (x1, y1, c11), (x1, y0, c01))
        return (p1, a1), (p2, a2)


# ---- the solid's world box and the box test ------------------------------------------------------------------------------------------
def solid_world_box(shape, verts, tf):
    R, T = tf
    k = int(shape["type"])
    p = [float(x) for x in shape["params"]]
    if k == CONVEX:
        lo, hi = [DBL_MAX] * 3, [-DBL_MAX] * 3
        off, n = int(shape["vertex_offset"]), int(shape["num_points"])
        for i in range(n):
            q = add(rot(R, tuple(float(x) for x in verts[off + i])), T)
            lo = [min(a, b) for a, b in zip(lo, q)]
            hi = [max(a, b) for a, b in zip(hi, q)]
        return tuple(lo), tuple(hi)
    if k == BOX:
        d = tuple(abs(R[i][0]) * p[0] + abs(R[i][1]) * p[1] + abs(R[i][2]) * p[2] for i in range(3))
    elif k == SPHERE:
        d = (p[0], p[0], p[0])
    elif k == ELLIPSOID:
        d = rot(R, (p[0], p[1], p[2]))
    elif k == CAPSULE:
        d = tuple(abs(R[i][2]) * p[1] + p[0] for i in range(3))
    elif k in (CONE, CYLINDER):
        d = tuple(abs(R[i][0] * p[0]) + abs(R[i][1] * p[0]) + abs(R[i][2] * p[1]) for i in range(3))
    else:
        raise ValueError("no height-field row for node type %d" % k)
    return sub(T, d), add(T, d)


def node_disjoint(tfh, node, blo, bhi, margin, bd2):
    R, T = tfh
    mn, mx = node["aabb_min"], node["aabb_max"]
    lo = hi = rot(R, mn)
    for ic in range(1, 8):
        c = rot(R, tuple(mx[i] if ic & (1 << i) else mn[i] for i in range(3)))
        lo = tuple(min(a, b) for a, b in zip(lo, c))
        hi = tuple(max(a, b) for a, b in zip(hi, c))
    lo, hi = add(lo, T), add(hi, T)
    g = tuple(max(lo[i] - bhi[i] - margin, 0.0) for i in range(3))
    sq = sqnorm(g)
    if sq > bd2:
        return True, sq
    g = tuple(max(blo[i] - hi[i] - margin, 0.0) for i in range(3))
    sq = sqnorm(g)
    if sq > bd2:
        return True, sq
    return False, sq


def walk(field, tfh, blo, bhi, margin, bd2):
    """The events of collisionRecurse in order, as far as they do not depend on the leaves: ('box', bound) / ('leaf', node id)."""
    events = []

    def recurse(b):
        node = field.nodes[b]
        if node["x_size"] == 1 and node["y_size"] == 1:
            events.append(("leaf", b))
            return
        disjoint, sq = node_disjoint(tfh, node, blo, bhi, margin, bd2)
        if disjoint:
            events.append(("box", math.sqrt(sq)))
            return
        recurse(node["first_child"])
        recurse(node["first_child"] + 1)

    recurse(0)
    return events


# ---- Project::projectTriangle and binCorrection -------------------------------------------------------------------------------------
def project_line(a, b, p):
    d = sub(b, a)
    l = sqnorm(d)
    assert l > 0
    t = dot(sub(p, a), d)
    p1 = 1.0 if t >= l else (0.0 if t <= 0 else t / l)
    p0 = 1.0 - p1
    if t >= l:
        sq = sqnorm(sub(p, b))
    elif t <= 0:
        sq = sqnorm(sub(p, a))
    else:
        sq = sqnorm(sub(add(a, scale(d, p1)), p))
    return p0, p1, sq


def project_on_triangle(a, b, c, p):
    """the point Project::projectTriangle parameterises, or None for a degenerate triangle (the reference reads uninitialised memory)"""
    vt = (a, b, c)
    dl = (sub(a, b), sub(b, c), sub(c, a))
    n = cross(dl[0], dl[1])
    l = sqnorm(n)
    if not l > 0:
        return None
    par = [0.0, 0.0, 0.0]
    mind = -1.0
    for i in range(3):
        if dot(sub(vt[i], p), cross(dl[i], n)) > 0:
            j = (i + 1) % 3
            p0, p1, sq = project_line(vt[i], vt[j], p)
            if mind < 0 or sq < mind:
                mind = sq
                par[i], par[j], par[(j + 1) % 3] = p0, p1, 0.0
    if mind < 0:
        d = dot(sub(a, p), n)
        s = math.sqrt(l)
        ptp = scale(n, d / l)
        par[0] = norm(cross(dl[1], sub(sub(b, p), ptp))) / s
        par[1] = norm(cross(dl[2], sub(sub(c, p), ptp))) / s
        par[2] = 1.0 - par[0] - par[1]
    return add(add(scale(a, par[0]), scale(b, par[1])), scale(c, par[2]))


def support_with_swept_sphere(shape, verts, direction):
    """getSupport<WithSweptSphere> in the solid's frame: the oracle's NoSweptSphere support plus the swept sphere"""
    k, p0, ssr = int(shape["type"]), float(shape["params"][0]), float(shape["swept_sphere_radius"])
    u = normalized(direction)
    if k == SPHERE:
        return scale(u, p0 + ssr)
    s, _ = ob.shape_support(np.asarray(shape).reshape(1), verts, direction)
    return add(tuple(float(x) for x in s), scale(u, p0 + ssr if k == CAPSULE else ssr))


def bin_correction(pts, part, active, shape, verts, tfs, distance, c1, c2, normal, is_collision, near=None):
    prec = 1e-12
    on_bin_side = True
    face_tri = None
    shortest = DBL_MAX
    face_normal = normal
    faces = [0, 1] + ([2] if active & 2 else []) + ([4] if active & 4 else []) + ([6] if active & 8 else [])

    def tri_distance(t):
        a, b, c = (pts[i] for i in TRIANGLES[part][t])
        q = project_on_triangle(a, b, c, c1)
        return DBL_MAX if q is None else norm(sub(q, c1))

    for f in faces:
        closest, d = f, tri_distance(f)
        if f > 1:
            d2 = tri_distance(f + 1)
            if d > d2:
                closest, d = f + 1, d2
        if near is not None and abs(d - prec) < near[0]:
            near[1] = True
        if d <= prec:
            on_bin_side, face_tri, shortest = False, closest, d
            break
        elif d < shortest:
            face_tri, shortest = closest, d
    if is_collision:
        if face_tri is None:
            return on_bin_side, NAN, NAN3, NAN3, NAN3, NAN3
        a, b, c = (pts[i] for i in TRIANGLES[part][face_tri])
        face_normal = normalized(cross(sub(b, a), sub(c, a)))
        R, T = tfs
        sl = support_with_swept_sphere(shape, verts, neg(rot_t(R, face_normal)))
        support = add(rot(R, sl), T)
        offset = dot(face_normal, a)
        pn, pd = (1.0, 0.0, 0.0), 0.0
        l = norm(face_normal)  # Plane(face_normal, offset): unitNormalTest
        if l > 0:
            inv = 1.0 / l
            pn, pd = scale(face_normal, inv), offset * inv
        dsp = dot(pn, support) - pd
        projected = sub(support, scale(face_normal, dsp))
        c1 = project_on_triangle(a, b, c, projected)
        if c1 is None:
            c1 = (0.0, 0.0, 0.0)
        c2 = add(c1, scale(face_normal, dsp))
        normal = face_normal
        distance = -abs(dsp)
    return on_bin_side, distance, c1, c2, normal, face_normal


def is_approx(a, b):
    return sqnorm(sub(a, b)) <= 1e-12 * 1e-12 * min(sqnorm(a), sqnorm(b))


# ---- collide() -----------------------------------------------------------------------------------------------------------------
def collide(fields, hfield, shapes, verts, shape, tf_hfield, tf_shape, req, swapped=None, near=1e-9):
    """fields: list of Field; hfield / shape: ids per query; tf_*: (n, 12) pose rows; req: abi.CollisionRequest.
    Returns (records, bounds, contacts, near_threshold): dicts per query, the distance_lower_bound per query, the contact list (dicts, in
    query order and within a query in the reference's order), and per query whether a decision quantity of the model lay within `near`
    of its threshold (leaf distance against margin + threshold; a face distance within 5e-13 of the 1e-12 on-face test)."""
    pkg_abi = ob._pkg().abi
    n = len(shape)
    margin, thr = float(req.security_margin), float(req.q.collision_distance_threshold)
    bd2 = float(req.break_distance) * float(req.break_distance)
    nmax = int(req.num_max_contacts)
    verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
    skip_all = margin == -math.inf
    # the walks, and the prisms of every visited leaf as convex shapes of one oracle call
    walks, jobs, extra_shapes, extra_verts = [], [], [], []
    cell_shape = {}
    nverts = len(verts)
    for i in range(n):
        if skip_all:
            walks.append(None)
            continue
        F = fields[int(hfield[i])]
        tfh, tfs = pose(tf_hfield[i]), pose(tf_shape[i])
        blo, bhi = solid_world_box(shapes[int(shape[i])], verts, tfs)
        ev = walk(F, tfh, blo, bhi, margin, bd2)
        walks.append(ev)
        for kind, b in ev:
            if kind != "leaf":
                continue
            key = (int(hfield[i]), b)
            if key not in cell_shape:
                ids = []
                for pts, _ in F.prisms(F.nodes[b]):
                    ids.append(len(shapes) + len(extra_shapes))
                    extra_shapes.append((nverts + 6 * len(extra_verts)))
                    extra_verts.append(pts)
                cell_shape[key] = ids
            for part in range(2):
                jobs.append((cell_shape[key][part], int(shape[i]), i))
    dist = {}
    if jobs:
        all_shapes = np.zeros(len(shapes) + len(extra_shapes), dtype=pkg_abi.SHAPE_DTYPE)
        all_shapes[:len(shapes)] = shapes
        for k, off in enumerate(extra_shapes):
            row = all_shapes[len(shapes) + k]
            row["type"], row["num_points"], row["vertex_offset"] = CONVEX, 6, off
        all_verts = np.concatenate([verts, np.asarray(extra_verts, dtype=np.float64).reshape(-1, 3)]) if extra_verts else verts
        dreq = pkg_abi.default_distance_request()
        for f in ("gjk_variant", "gjk_convergence_criterion", "gjk_convergence_criterion_type", "gjk_max_iterations", "epa_max_iterations",
                  "gjk_tolerance", "epa_tolerance"):
            setattr(dreq.q, f, getattr(req.q, f))
        s1 = np.array([j[0] for j in jobs], dtype=np.uint32)
        s2 = np.array([j[1] for j in jobs], dtype=np.uint32)
        q = np.array([j[2] for j in jobs])
        res = ob.distance_batch(all_shapes, all_verts, s1, s2, np.asarray(tf_hfield)[q], np.asarray(tf_shape)[q], dreq, n_threads=8)
        for (ps, _, i), r in zip(jobs, res):
            dist[(i, ps)] = r
    records, bounds, contacts, near_flags = [], [], [], []
    for i in range(n):
        sw = bool(swapped[i]) if swapped is not None else False
        if skip_all:
            records.append(dict(skipped=True, swapped=sw))
            bounds.append(DBL_MAX)
            near_flags.append(False)
            continue
        F = fields[int(hfield[i])]
        tfs = pose(tf_shape[i])
        srow = shapes[int(shape[i])]
        dlb, np1, np2, nn = DBL_MAX, NAN3, NAN3, NAN3
        mine = []
        flag = [5e-13, False]
        for kind, b in walks[i]:
            if kind == "box":  # updateDistanceLowerBoundFromBV
                if dlb <= 0:
                    continue
                if b < dlb:
                    dlb = b
                continue
            node = F.nodes[b]
            outs = []
            for part, (pts, active) in enumerate(F.prisms(node)):
                r = dist[(i, cell_shape[(int(hfield[i]), b)][part])]
                d = float(r["distance"])
                coll = d - margin <= thr
                if abs(d - margin - thr) < near:
                    flag[1] = True
                c1, c2, nrm = (tuple(float(x) for x in r[k]) for k in ("p1", "p2", "normal"))
                if coll:
                    side, d, c1, c2, nrm, ntop = bin_correction(pts, part, active, srow, verts, tfs, d, c1, c2, nrm, True, flag)
                else:  # binCorrection changes nothing but the side flag, which only the gate of a leaf in collision reads: on demand
                    side, ntop = None, nrm
                outs.append((coll, d, c1, c2, nrm, ntop, side))
            (k1, d1), (k2, d2) = (outs[0][0], outs[0][1]), (outs[1][0], outs[1][1])
            if k1 and k2:
                pick = 1 if d1 > d2 else 0
            elif k1:
                pick = 0
            elif k2:
                pick = 1
            else:
                pick = 1 if d1 > d2 else 0
            collision = k1 or k2
            _, distance, c1, c2, nrm, ntop, side = outs[pick]
            dtc = distance - margin
            if dtc <= thr:
                if side is None:
                    pts, active = F.prisms(node)[pick]
                    side = bin_correction(pts, pick, active, srow, verts, tfs, distance, c1, c2, nrm, False, flag)[0]
                if len(mine) < nmax:
                    if is_approx(ntop, nrm) and (collision or not side):
                        mine.append(dict(pair=i, node=b, depth=distance, normal=nrm, p1=c1, p2=c2))
            if dtc < dlb:  # updateDistanceLowerBoundFromLeaf
                dlb, np1, np2, nn = dtc, c1, c2, nrm
            if len(mine) >= nmax:  # canStop()
                break
        if sw:
            np1, np2, nn = np2, np1, neg(nn)
            for c in mine:
                c["p1"], c["p2"], c["normal"] = c["p2"], c["p1"], neg(c["normal"])
        for c in mine:
            c["b1"], c["b2"] = (-1, c["node"]) if sw else (c["node"], -1)
        if mine:
            f = mine[0]
            rec = dict(distance=f["depth"], normal=f["normal"], p1=f["p1"], p2=f["p2"], b1=f["b1"], b2=f["b2"])
        else:
            rec = dict(distance=dlb, normal=nn, p1=np1, p2=np2, b1=-1, b2=-1)
        rec.update(num_contacts=len(mine), skipped=False, swapped=sw)
        records.append(rec)
        bounds.append(dlb)
        contacts.extend(mine)
        near_flags.append(flag[1])
    return records, bounds, contacts, near_flags
