"""`hppfcl`-named Python surface over the C ABI: the names, argument meaning and error behaviour of the
reference's Python module (python/collision.cc:257-266, python/distance.cc:150-159, python/collision-geometries.cc,
python/math.cc) for the path in scope, so that code written against `import hppfcl` -- e.g. the reference's
test/python_unit/api.py, collision.py, collision_manager.py -- runs on `import hppfcl_amd.compat as hppfcl`.

Plumbing only: every query is a batch of one (or, through `collide_pairs` / the collision manager, one batch)
on the HIP library.  No CPU fallback."""
import functools
import os

import numpy as np

from . import abi, bvh_builder, engine, geometry


class NODE_TYPE:  # include/hpp/fcl/collision_object.h:65-89
    BV_OBBRSS = abi.BV_OBBRSS
    GEOM_BOX, GEOM_SPHERE, GEOM_CAPSULE, GEOM_CONE = abi.GEOM_BOX, abi.GEOM_SPHERE, abi.GEOM_CAPSULE, abi.GEOM_CONE
    GEOM_CYLINDER, GEOM_CONVEX, GEOM_PLANE = abi.GEOM_CYLINDER, abi.GEOM_CONVEX, abi.GEOM_PLANE
    GEOM_HALFSPACE, GEOM_TRIANGLE, GEOM_ELLIPSOID = abi.GEOM_HALFSPACE, abi.GEOM_TRIANGLE, abi.GEOM_ELLIPSOID
    HF_AABB, HF_OBBRSS = abi.HF_GEOM_AABB, abi.HF_GEOM_OBBRSS
    GEOM_OCTREE = abi.GEOM_OCTREE


class GJKInitialGuess:
    DefaultGuess, CachedGuess, BoundingVolumeGuess = abi.DefaultGuess, abi.CachedGuess, abi.BoundingVolumeGuess


class GJKVariant:
    DefaultGJK, PolyakAcceleration, NesterovAcceleration = abi.DefaultGJK, abi.PolyakAcceleration, abi.NesterovAcceleration


class GJKConvergenceCriterion:
    Default, DualityGap, Hybrid = abi.Default, abi.DualityGap, abi.Hybrid


class GJKConvergenceCriterionType:
    Relative, Absolute = abi.Relative, abi.Absolute


def _v3(v):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.shape != (3,):
        raise ValueError("expected a 3-vector")
    return a.copy()


class Transform3f:  # include/hpp/fcl/math/transform.h:56-218
    def __init__(self, R=None, T=None):
        self._R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3).copy()
        self._T = np.zeros(3) if T is None else _v3(T)

    @staticmethod
    def Identity():
        return Transform3f()

    def getRotation(self):
        return self._R

    def getTranslation(self):
        return self._T

    def setRotation(self, R):
        self._R = np.asarray(R, dtype=np.float64).reshape(3, 3).copy()

    def setTranslation(self, T):
        self._T = _v3(T)

    def setTransform(self, R, T):
        self.setRotation(R)
        self.setTranslation(T)

    def transform(self, v):
        return self._R @ _v3(v) + self._T

    def inverse(self):
        return Transform3f(self._R.T, -self._R.T @ self._T)

    def __mul__(self, other):  # transform.h:187-190
        return Transform3f(self._R @ other._R, self._R @ other._T + self._T)

    def _abi(self):
        return geometry.make_pose(R=self._R, T=self._T)


class CollisionGeometry:
    def getNodeType(self):
        return self._node_type


class ShapeBase(CollisionGeometry):
    _swept = 0.0

    def getSweptSphereRadius(self):
        return self._swept

    def setSweptSphereRadius(self, r):
        if r < 0:
            raise ValueError("Swept-sphere radius must be positive.")  # geometric_shapes.h:74-80
        self._swept = float(r)


class Box(ShapeBase):
    _node_type = NODE_TYPE.GEOM_BOX

    def __init__(self, x, y=None, z=None):
        side = _v3(x) if y is None else np.array([x, y, z], dtype=np.float64)
        self.halfSide = side / 2.0

    def _register(self, L):
        return L.add_box(*(2.0 * np.asarray(self.halfSide, dtype=np.float64)), swept_sphere_radius=self._swept)


class Sphere(ShapeBase):
    _node_type = NODE_TYPE.GEOM_SPHERE

    def __init__(self, radius):
        self.radius = float(radius)

    def _register(self, L):
        return L.add_sphere(self.radius, self._swept)


class Ellipsoid(ShapeBase):
    _node_type = NODE_TYPE.GEOM_ELLIPSOID

    def __init__(self, rx, ry=None, rz=None):
        self.radii = _v3(rx) if ry is None else np.array([rx, ry, rz], dtype=np.float64)

    def _register(self, L):
        return L.add_ellipsoid(*map(float, self.radii), swept_sphere_radius=self._swept)


class _RadiusHalfLength(ShapeBase):
    def __init__(self, radius, lz):
        self.radius = float(radius)
        self.halfLength = float(lz) / 2.0  # geometric_shapes.h:386-387


class Capsule(_RadiusHalfLength):
    _node_type = NODE_TYPE.GEOM_CAPSULE

    def _register(self, L):
        return L.add_capsule(self.radius, 2.0 * self.halfLength, self._swept)


class Cone(_RadiusHalfLength):
    _node_type = NODE_TYPE.GEOM_CONE

    def _register(self, L):
        return L.add_cone(self.radius, 2.0 * self.halfLength, self._swept)


class Cylinder(_RadiusHalfLength):
    _node_type = NODE_TYPE.GEOM_CYLINDER

    def _register(self, L):
        return L.add_cylinder(self.radius, 2.0 * self.halfLength, self._swept)


class _Flat(ShapeBase):
    def __init__(self, n=(1.0, 0.0, 0.0), d=0.0, *rest):
        if rest:  # (a, b, c, d)
            n, d = (n, d, rest[0]), rest[1]
        self.n, self.d = _v3(n), float(d)
        l = np.linalg.norm(self.n)  # unitNormalTest, geometric_shapes.cpp:121-143
        if l > 0:
            self.n, self.d = self.n / l, self.d / l
        else:
            self.n, self.d = np.array([1.0, 0.0, 0.0]), 0.0


class Halfspace(_Flat):
    _node_type = NODE_TYPE.GEOM_HALFSPACE

    def _register(self, L):
        return L.add_halfspace(self.n, self.d, self._swept)


class Plane(_Flat):
    _node_type = NODE_TYPE.GEOM_PLANE

    def _register(self, L):
        return L.add_plane(self.n, self.d, self._swept)


class TriangleP(ShapeBase):
    _node_type = NODE_TYPE.GEOM_TRIANGLE

    def __init__(self, a, b, c):
        self.a, self.b, self.c = _v3(a), _v3(b), _v3(c)

    def _register(self, L):
        return L.add_triangle(self.a, self.b, self.c, self._swept)


class Triangle:  # include/hpp/fcl/data_types.h:101-144
    def __init__(self, p1=0, p2=0, p3=0):
        self.vids = [int(p1), int(p2), int(p3)]

    def __getitem__(self, i):
        return self.vids[i]


class StdVec_Vec3f(list):
    pass


class StdVec_Triangle(list):
    pass


class Convex(ShapeBase):
    """Convex<Triangle>(points, triangles).  Up to 32 vertices the narrow phase scans the points in registers, above it
    scans them from memory; with facets given, hulls of HFCL_CLIMB_MIN (512) vertices and more climb the vertex adjacency
    the facets define, as the reference does (fillNeighbors, shape/details/convex.hxx:231-280; getShapeSupportLog)."""
    _node_type = NODE_TYPE.GEOM_CONVEX

    def __init__(self, points, polygons=None):
        self.points = np.array([_v3(p) for p in points], dtype=np.float64)
        self.num_points = len(self.points)
        self.polygons = list(polygons) if polygons is not None else []

    def neighbors(self):
        """ConvexBase::neighbors as CSR (offsets[num_points + 1], ids), or None without facets.  Cached per object, keyed on the facets' indices."""
        if not self.polygons:
            return None
        polys = [tuple(int(poly[k]) for k in range(3)) if isinstance(poly, Triangle) else tuple(int(k) for k in poly) for poly in self.polygons]
        key = (len(self.points), hash(tuple(polys)))  # the facets themselves: an edit in place must not leave a stale adjacency behind
        if getattr(self, "_nb_cache", None) is not None and self._nb_cache[0] == key:
            return self._nb_cache[1]
        npts = len(self.points)
        nb = [set() for _ in range(npts)]
        for idx in polys:
            n = len(idx)
            for j in range(n):
                nb[idx[j]].add(idx[j - 1])
                nb[idx[j]].add(idx[(j + 1) % n])
        offs = np.zeros(npts + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(x) for x in nb])
        out = (offs, np.array([v for x in nb for v in sorted(x)], dtype=np.uint32))
        self._nb_cache = (key, out)
        return out

    def _register(self, L):
        return L.add_convex(self.points, self._swept)


class BVHModelOBBRSS(CollisionGeometry):  # BVHModel<OBBRSS>, src/BVH/BVH_model.cpp:264-576
    _node_type = NODE_TYPE.BV_OBBRSS

    def __init__(self):
        self._v, self._t, self._mesh = [], [], None

    def beginModel(self, num_tris=0, num_vertices=0):
        self._v, self._t, self._mesh = [], [], None
        return 0

    def addVertex(self, p):
        self._v.append(_v3(p))
        return 0

    def addTriangle(self, p1, p2, p3):
        base = len(self._v)
        self._v += [_v3(p1), _v3(p2), _v3(p3)]
        self._t.append((base, base + 1, base + 2))
        return 0

    def addSubModel(self, vertices, triangles=None):
        base = len(self._v)
        self._v += [_v3(p) for p in vertices]
        for t in ([] if triangles is None else triangles):
            self._t.append((base + int(t[0]), base + int(t[1]), base + int(t[2])))
        return 0

    def endModel(self):
        if not self._t:
            return -3  # BVH_ERR_BUILD_EMPTY_MODEL
        self._mesh = bvh_builder.Mesh(np.array(self._v), np.array(self._t, dtype=np.uint32))
        return 0

    @property
    def num_vertices(self):
        return len(self._v)

    @property
    def num_tris(self):
        return len(self._t)


class HeightFieldAABB(CollisionGeometry):  # HeightField<AABB>, include/hpp/fcl/hfield.h:202-520
    """heights: (ny, nx), row 0 = the north edge (+y_dim/2).  The tree is built by the library's host builder (hfcl_hfield_build);
    collide() against a convex solid, in either operand order, goes to hfcl_hfield_collide_batch."""
    _node_type = NODE_TYPE.HF_AABB

    def __init__(self, x_dim, y_dim, heights, min_height=0.0):
        self._x_dim, self._y_dim, self._min = float(x_dim), float(y_dim), float(min_height)
        self._version = 0
        self.aabb_local = None
        self._set(np.array(heights, dtype=np.float64))

    def _set(self, heights):
        if heights.ndim != 2:
            raise ValueError("heights: a (ny, nx) matrix")
        try:
            self._nodes, self._xg, self._yg = engine.hfield_build(self._x_dim, self._y_dim, heights, self._min)
        except engine.EngineError as e:
            raise ValueError(str(e))
        self._heights = np.maximum(heights, self._min)
        self._max = float(self._nodes[0]["max_height"])
        self._version += 1  # (the next collide() registers the field again)

    def getXDim(self):
        return self._x_dim

    def getYDim(self):
        return self._y_dim

    def getXGrid(self):
        return self._xg

    def getYGrid(self):
        return self._yg

    def getHeights(self):
        return self._heights

    def getMinHeight(self):
        return self._min

    def getMaxHeight(self):
        return self._max

    def getNodes(self):
        return self._nodes

    def computeLocalAABB(self):  # hfield.h:278-287
        a = np.array([self._xg[0], self._yg[0], self._min])
        b = np.array([self._xg[-1], self._yg[-1], self._max])
        self.aabb_local = np.concatenate([np.minimum(a, b), np.maximum(a, b)])
        self.aabb_radius = float(np.sqrt(((a - b) ** 2).sum())) / 2.0
        self.aabb_center = (self.aabb_local[:3] + self.aabb_local[3:]) * 0.5

    def updateHeights(self, new_heights):  # hfield.h:290-305: same size; the tree is rebuilt and uploaded again by the next call
        h = np.array(new_heights, dtype=np.float64)
        if h.shape != self._heights.shape:
            raise ValueError("The matrix containing the new heights values does not have the same matrix size as the original one.")
        self._set(h)


class OcTree(CollisionGeometry):  # include/hpp/fcl/octree.h:53-296, over a node array instead of an octomap tree
    """nodes: abi.OCTREE_NODE_DTYPE (node 0 the root, child[i] = index of child i, 0 = none; engine.octree_from_points / makeOctree
    make one).  Every box is halved down from getRootBV, as the reference computes them.  collide() against a convex solid, in either
    operand order, goes to hfcl_octree_collide_batch."""
    _node_type = NODE_TYPE.GEOM_OCTREE

    def __init__(self, nodes, resolution, depth=abi.OCTREE_MAX_DEPTH, occupancy_threshold=0.5, free_threshold=0.0):
        self._nodes = np.ascontiguousarray(nodes, dtype=abi.OCTREE_NODE_DTYPE).copy()
        self._resolution, self._depth = float(resolution), int(depth)
        try:
            engine.octree_validate(self._nodes, self._depth)
        except engine.EngineError as e:
            raise ValueError(str(e))
        self._occ, self._free = float(occupancy_threshold), float(free_threshold)
        self._version = 1

    def getTreeDepth(self):
        return self._depth

    def getResolution(self):
        return self._resolution

    def size(self):
        return len(self._nodes)

    def getNodes(self):
        return self._nodes

    def getRootBV(self):  # octree.h:139-144: (min xyz, max xyz)
        delta = (1 << self._depth) * self._resolution / 2
        return np.array([-delta, -delta, -delta, delta, delta, delta])

    def getOccupancyThres(self):
        return self._occ

    def getFreeThres(self):
        return self._free

    def setOccupancyThres(self, d):
        self._occ = float(d)
        self._version += 1  # (the next collide() sets the thresholds on the library)

    def setFreeThres(self, d):
        self._free = float(d)
        self._version += 1

    def _leaves(self):
        """(node, min, max) of every node without children, depth-first with the children in index order"""
        out = []
        if len(self._nodes) == 0:
            return out
        child = self._nodes["child"]
        b = self.getRootBV()
        stack = [(0, b[:3].copy(), b[3:].copy())]
        while stack:
            i, lo, hi = stack.pop()
            kids = child[i]
            if not kids.any():
                out.append((i, lo, hi))
                continue
            for k in range(7, -1, -1):  # (popped in index order)
                if kids[k]:
                    clo, chi = lo.copy(), hi.copy()
                    for a in range(3):  # computeChildBV, octree.h:299-324
                        if k & (1 << a):
                            clo[a] = (lo[a] + hi[a]) * 0.5
                        else:
                            chi[a] = (lo[a] + hi[a]) * 0.5
                    stack.append((int(kids[k]), clo, chi))
        return out

    def toBoxes(self):  # octree.h:178-200: (x, y, z, size, occupancy, threshold) of the occupied leaves, from the halved boxes
        rows = [[(lo[0] + hi[0]) * 0.5, (lo[1] + hi[1]) * 0.5, (lo[2] + hi[2]) * 0.5, hi[0] - lo[0], float(self._nodes[i]["occupancy"]), self._occ]
                for i, lo, hi in self._leaves() if self._nodes[i]["occupancy"] >= self._occ]
        return np.array(rows, dtype=np.float64).reshape(-1, 6)


def makeOctree(points, resolution):  # src/octree.cpp:188-202 (octomap's tree depth: 16)
    try:
        return OcTree(engine.octree_from_points(points, resolution, abi.OCTREE_MAX_DEPTH), resolution, abi.OCTREE_MAX_DEPTH)
    except engine.EngineError as e:
        raise ValueError(str(e))


class _Query:
    def __init__(self):
        self.gjk_initial_guess = GJKInitialGuess.DefaultGuess
        self.cached_gjk_guess = np.array([1.0, 0.0, 0.0])
        self.cached_support_func_guess = np.zeros(2, dtype=np.int32)
        self.gjk_max_iterations, self.gjk_tolerance = 128, 1e-6
        self.gjk_variant = GJKVariant.DefaultGJK
        self.gjk_convergence_criterion = GJKConvergenceCriterion.Default
        self.gjk_convergence_criterion_type = GJKConvergenceCriterionType.Relative
        self.epa_max_iterations, self.epa_tolerance = 64, 1e-6
        self.enable_timings = False
        self.collision_distance_threshold = 1e-12

    def _fill(self, q):
        q.gjk_initial_guess, q.gjk_variant = int(self.gjk_initial_guess), int(self.gjk_variant)
        q.gjk_convergence_criterion = int(self.gjk_convergence_criterion)
        q.gjk_convergence_criterion_type = int(self.gjk_convergence_criterion_type)
        q.gjk_max_iterations, q.epa_max_iterations = int(self.gjk_max_iterations), int(self.epa_max_iterations)
        q.gjk_tolerance, q.epa_tolerance = float(self.gjk_tolerance), float(self.epa_tolerance)
        q.collision_distance_threshold = float(self.collision_distance_threshold)
        for k in range(3):
            q.cached_gjk_guess[k] = float(self.cached_gjk_guess[k])
        for k in range(2):
            q.cached_support_func_guess[k] = int(self.cached_support_func_guess[k])

    def updateGuess(self, result):  # collision_data.h:258-265
        if self.gjk_initial_guess == GJKInitialGuess.CachedGuess:
            self.cached_gjk_guess = np.array(result.cached_gjk_guess)
            self.cached_support_func_guess = np.array(result.cached_support_func_guess)


class CollisionRequest(_Query):  # collision_data.h:312-366
    def __init__(self, flag=None, num_max_contacts=1):
        super().__init__()
        self.num_max_contacts, self.enable_contact = int(num_max_contacts), True
        self.security_margin, self.break_distance = 0.0, 1e-3
        self.distance_upper_bound = np.finfo(np.float64).max

    def _abi(self):
        r = abi.default_collision_request()
        self._fill(r.q)
        r.num_max_contacts, r.enable_contact = int(self.num_max_contacts), int(bool(self.enable_contact))
        r.security_margin, r.break_distance = float(self.security_margin), float(self.break_distance)
        r.distance_upper_bound = float(self.distance_upper_bound)
        return r


class DistanceRequest(_Query):  # collision_data.h:987-1031
    def __init__(self, enable_nearest_points=True, enable_signed_distance=True, rel_err=0.0, abs_err=0.0):
        super().__init__()
        self.enable_nearest_points, self.enable_signed_distance = enable_nearest_points, enable_signed_distance
        self.rel_err, self.abs_err = rel_err, abs_err

    def _abi(self):
        r = abi.default_distance_request()
        self._fill(r.q)
        r.enable_nearest_points, r.enable_signed_distance = int(bool(self.enable_nearest_points)), int(bool(self.enable_signed_distance))
        r.rel_err, r.abs_err = float(self.rel_err), float(self.abs_err)
        return r


_NAN3 = np.full(3, np.nan)


class Contact:  # collision_data.h:59-166
    NONE = -1

    def __init__(self, o1=None, o2=None, b1=-1, b2=-1, p1=_NAN3, p2=_NAN3, normal=_NAN3, depth=np.finfo(np.float64).max):
        self.o1, self.o2, self.b1, self.b2 = o1, o2, int(b1), int(b2)
        self.nearest_points = [np.array(p1), np.array(p2)]
        self.normal = np.array(normal)
        self.pos = (self.nearest_points[0] + self.nearest_points[1]) / 2.0
        self.penetration_depth = float(depth)

    def getNearestPoint1(self):
        return self.nearest_points[0]

    def getNearestPoint2(self):
        return self.nearest_points[1]


class CollisionResult:  # collision_data.h:391-494
    def __init__(self):
        self.clear()

    def clear(self):
        self._contacts = []
        self.distance_lower_bound = np.finfo(np.float64).max
        self.normal = _NAN3.copy()
        self.nearest_points = [_NAN3.copy(), _NAN3.copy()]
        self.cached_gjk_guess = np.array([1.0, 0.0, 0.0])
        self.cached_support_func_guess = np.zeros(2, dtype=np.int32)

    def isCollision(self):
        return len(self._contacts) > 0

    def numContacts(self):
        return len(self._contacts)

    def getContact(self, i):
        if not self._contacts:
            raise RuntimeError("The number of contacts is zero. No Contact can be returned.")  # :449-456
        return self._contacts[min(i, len(self._contacts) - 1)]

    def getContacts(self):
        return list(self._contacts)

    def addContact(self, c):
        self._contacts.append(c)

    def getNearestPoint1(self):
        return self.nearest_points[0]

    def getNearestPoint2(self):
        return self.nearest_points[1]


class DistanceResult:  # collision_data.h:1053-1174
    def __init__(self):
        self.clear()

    def clear(self):
        self.min_distance = np.finfo(np.float64).max
        self.normal = _NAN3.copy()
        self.nearest_points = [_NAN3.copy(), _NAN3.copy()]
        self.o1 = self.o2 = None
        self.b1 = self.b2 = -1
        self.cached_gjk_guess = np.array([1.0, 0.0, 0.0])
        self.cached_support_func_guess = np.zeros(2, dtype=np.int32)

    def getNearestPoint1(self):
        return self.nearest_points[0]

    def getNearestPoint2(self):
        return self.nearest_points[1]


class _Context:
    """Shape table of every geometry seen so far + the device library built from it (rebuilt when it grows)."""

    def __init__(self, device=0):
        self.device, self.L, self.lib = device, geometry.ShapeLibrary(), None
        self.ids, self.keep, self.meshes = {}, [], []
        self.built = 0
        self.hfields, self.hfield_ids = [], {}  # registered (field, heights, ...) in index order; (id(field), version) -> index
        self.octrees, self.octree_ids = [], {}  # the same for OcTree objects (a version: the thresholds as they were)

    @staticmethod
    def _signature(g):
        if isinstance(g, BVHModelOBBRSS):
            return ("bvh", id(g._mesh))
        vals = []
        for k, v in sorted(vars(g).items()):
            if k not in ("polygons", "_nb_cache"):  # (the cached adjacency is derived from the polygons)
                vals.append((k, np.asarray(v, dtype=np.float64).tobytes() if not isinstance(v, list) else None))
        return (type(g).__name__, tuple(vals))

    def add(self, g):
        sig = self._signature(g)
        hit = self.ids.get(id(g))
        if hit and hit[1] == sig:
            return hit[0]
        if isinstance(g, BVHModelOBBRSS):
            if g._mesh is None:
                raise ValueError("BVHModel: endModel() has not been called")
            self.meshes.append(g._mesh)
            sid = self.L.add_bvh(len(self.meshes) - 1, g.num_vertices)
        elif isinstance(g, CollisionGeometry) and hasattr(g, "_register"):
            sid = g._register(self.L)
        else:
            raise ValueError("unsupported collision geometry")
        self.ids[id(g)] = (sid, sig)
        self.keep.append(g)  # ids stay valid while the context lives
        return sid

    HFIELDS_MAX = 16  # registered (field, version) entries the context keeps before it clears them and the library's tables

    def add_hfield(self, g):
        """the index of a HeightFieldAABB on the library (a field whose heights were updated is registered again; at most HFIELDS_MAX
        registrations are kept, so a caller that updates heights every step does not grow host or device memory)"""
        key = (id(g), g._version)
        if key not in self.hfield_ids:
            if len(self.hfields) >= self.HFIELDS_MAX:  # versions of updated fields, fields that came and went: start over, here and on the library
                self.hfields, self.hfield_ids = [], {}
                if self.lib is not None:
                    self.lib.clear_hfields()
            self.hfield_ids[key] = len(self.hfields)
            self.hfields.append((g, g._x_dim, g._y_dim, g._heights.copy(), g._min))  # (g is kept: its id stays its own while it is listed)
        return self.hfield_ids[key]

    OCTREES_MAX = 16  # the same for (octree, version) entries

    def add_octree(self, g):
        """the index of an OcTree on the library (one whose thresholds were set is registered again; at most OCTREES_MAX registrations)"""
        key = (id(g), g._version)
        if key not in self.octree_ids:
            if len(self.octrees) >= self.OCTREES_MAX:
                self.octrees, self.octree_ids = [], {}
                if self.lib is not None:
                    self.lib.clear_octrees()
            self.octree_ids[key] = len(self.octrees)
            self.octrees.append((g, g._nodes, g._resolution, g._depth, g._occ, g._free))
        return self.octree_ids[key]

    def library(self):
        lib = self._library()
        for _, x_dim, y_dim, h, mh in self.hfields[lib.hfield_count():]:  # (all of them on a library that was just rebuilt)
            lib.add_hfield(x_dim, y_dim, h, mh)
        for _, nodes, res, depth, occ, free in self.octrees[lib.octree_count():]:
            lib.add_octree(nodes, res, depth, occ, free)
        return lib

    def _library(self):
        if self.lib is None or self.built != len(self.L):
            if self.lib is not None:
                self.lib.close()
            self.lib = engine.Library(self.L, device=self.device)
            for m in self.meshes:
                self.lib.add_bvh(m)
            # large hulls with facets: the adjacency the device climbs.  Only hulls the engine will climb (its own threshold,
            # hfcl_lib_climb_min: below that the scan is faster) pay the host loop and the device copy.
            climb_min = self.lib.climb_min()
            for g in self.keep:
                if isinstance(g, Convex) and g.num_points >= max(33, climb_min):
                    nb = g.neighbors()
                    if nb is not None:
                        self.lib.set_convex_neighbors(self.ids[id(g)][0], *nb)
            self.built = len(self.L)
        return self.lib


_ctx = None


def _context():
    global _ctx
    if _ctx is None:
        _ctx = _Context()
    return _ctx


def _check_pair(o1, o2, for_distance):
    t1, t2 = isinstance(o1, OcTree), isinstance(o2, OcTree)
    if (t1 or t2) and not for_distance:
        other = int((o2 if t1 else o1).getNodeType())
        if t1 != t2 and (engine.octree_pair_supported(other) or engine.octree_mesh_pair_supported(other)):  # a solid, or a BVHModel<OBBRSS>
            return
        raise ValueError("Collision function between node type %d and node type %d is not yet supported." % (o1.getNodeType(), o2.getNodeType()))
    if t1 or t2:  # distance(): an octree against one of the seven convex solids, either order (hppfcl_amd_octree_distance.h)
        if t1 != t2 and engine.octree_distance_pair_supported(int((o2 if t1 else o1).getNodeType())):
            return
        raise ValueError("Distance function between node type %d and node type %d is not yet supported." % (o1.getNodeType(), o2.getNodeType()))
    h1, h2 = isinstance(o1, HeightFieldAABB), isinstance(o2, HeightFieldAABB)
    if (h1 or h2) and not for_distance:
        if h1 != h2 and engine.hfield_pair_supported(int((o2 if h1 else o1).getNodeType())):
            return
        raise ValueError("Collision function between node type %d and node type %d is not yet supported." % (o1.getNodeType(), o2.getNodeType()))
    if not engine.dll().hfcl_pair_supported(int(o1.getNodeType()), int(o2.getNodeType()), int(for_distance)):
        raise ValueError("%s function between node type %d and node type %d is not yet supported." %
                         ("Distance" if for_distance else "Collision", o1.getNodeType(), o2.getNodeType()))


def _run(kind, pairs, request):
    """pairs: list of (o1, tf1, o2, tf2) -> (records, guesses, contacts or None)"""
    ctx = _context()
    ids = [(ctx.add(o1), ctx.add(o2)) for o1, _, o2, _ in pairs]
    lib = ctx.library()
    s1 = np.array([a for a, _ in ids], dtype=np.uint32)
    s2 = np.array([b for _, b in ids], dtype=np.uint32)
    tf1 = np.concatenate([p[1]._abi().reshape(1, 12) for p in pairs])
    tf2 = np.concatenate([p[3]._abi().reshape(1, 12) for p in pairs])
    req = request._abi()
    try:
        if kind == "distance":
            rec, g = lib.distance(s1, s2, tf1, tf2, req, want_guess=True)
            return rec, g, None
        if request.num_max_contacts > 1 and any(isinstance(p[0], BVHModelOBBRSS) or isinstance(p[2], BVHModelOBBRSS) for p in pairs):
            cap = int(min(request.num_max_contacts, 1 << 16)) * len(pairs)
            rec, contacts, _ = lib.collide_contacts(s1, s2, tf1, tf2, req, cap)
            return rec, None, contacts
        rec, g = lib.collide(s1, s2, tf1, tf2, req, want_guess=True)
        return rec, g, None
    except engine.EngineError as e:
        if e.code in (abi.ERR_INVALID_ARGUMENT, abi.ERR_UNSUPPORTED_PAIR):
            raise ValueError(str(e))  # std::invalid_argument in the reference
        raise


def _fill_collision(result, o1, o2, request, rec, guess, contacts, pair_index=0):
    if abi.status_skipped(rec["status"]):
        return
    d = float(rec["distance"])
    dtc = d - request.security_margin
    if dtc < result.distance_lower_bound:  # updateDistanceLowerBoundFromLeaf, collision_data.h:1186-1197
        result.distance_lower_bound = dtc
        result.normal = np.array(rec["normal"])
        result.nearest_points = [np.array(rec["p1"]), np.array(rec["p2"])]
    if contacts is not None:
        for c in contacts[contacts["pair"] == pair_index]:
            if result.numContacts() < request.num_max_contacts:
                result.addContact(Contact(o1, o2, c["b1"], c["b2"], c["p1"], c["p2"], c["normal"], c["penetration_depth"]))
    elif rec["num_contacts"] > 0 and result.numContacts() < request.num_max_contacts:
        result.addContact(Contact(o1, o2, rec["b1"], rec["b2"], rec["p1"], rec["p2"], rec["normal"], d))
    if guess is not None:
        result.cached_gjk_guess = np.array(guess["gjk_guess"])
        result.cached_support_func_guess = np.array(guess["support_guess"])
        request.updateGuess(result)


def _one_listed_query(call, container, shape, tf_container, tf_shape, request, swapped, **kw):
    """One query through a height-field / octree batch call of the library; what the engine refuses of it is the reference's
    std::invalid_argument."""
    try:
        return call([container], [shape], tf_container._abi().reshape(1, 12), tf_shape._abi().reshape(1, 12), request._abi(),
                    swapped=[1 if swapped else 0], **kw)
    except engine.EngineError as e:
        if e.code in (abi.ERR_INVALID_ARGUMENT, abi.ERR_UNSUPPORTED_PAIR, abi.ERR_LIMIT):
            raise ValueError(str(e))
        raise


def _collide_hfield(o1, tf1, o2, tf2, request, result):
    """(HeightFieldAABB, solid) or (solid, HeightFieldAABB) through hfcl_hfield_collide_batch.  The result gets every contact and the
    call's distance_lower_bound; its nearest_points / normal are the record's: the first contact's when there is one."""
    swapped = not isinstance(o1, HeightFieldAABB)
    field, tfh, solid, tfs = (o2, tf2, o1, tf1) if swapped else (o1, tf1, o2, tf2)
    ctx = _context()
    sid, hid = ctx.add(solid), ctx.add_hfield(field)
    rec, dlb, contacts, _ = _one_listed_query(ctx.library().hfield_collide, hid, sid, tfh, tfs, request, swapped,
                                              max_contacts=int(min(request.num_max_contacts, 1 << 16)))
    if abi.status_skipped(rec[0]["status"]):
        return result.numContacts()
    if dlb[0] < result.distance_lower_bound:
        result.distance_lower_bound = float(dlb[0])
        result.normal = np.array(rec[0]["normal"])
        result.nearest_points = [np.array(rec[0]["p1"]), np.array(rec[0]["p2"])]
    for c in contacts:
        if result.numContacts() < request.num_max_contacts:
            result.addContact(Contact(o1, o2, c["b1"], c["b2"], c["p1"], c["p2"], c["normal"], c["penetration_depth"]))
    return result.numContacts()


def _collide_octree(o1, tf1, o2, tf2, request, result):
    """(OcTree, solid or mesh) or (solid or mesh, OcTree) through hfcl_octree_collide_batch / hfcl_octree_mesh_collide_batch.  Either order gets the octree-first result (the reference
    does not swap it back: src/collision.cpp:92-108 has no octree branch): the tree is o1 of every contact, its node b1."""
    swapped = not isinstance(o1, OcTree)
    tree, tft, solid, tfs = (o2, tf2, o1, tf1) if swapped else (o1, tf1, o2, tf2)
    ctx = _context()
    sid, tid = ctx.add(solid), ctx.add_octree(tree)
    lib = ctx.library()
    # a BVHModel<OBBRSS> goes through hfcl_octree_mesh_collide_batch (hppfcl_amd_octree_mesh.h): the same record conventions, the
    # triangle in b2, the solver's own points in the contacts
    call = lib.octree_mesh_collide if isinstance(solid, BVHModelOBBRSS) else lib.octree_collide
    rec, dlb, contacts, _ = _one_listed_query(call, tid, sid, tft, tfs, request, swapped, max_contacts=int(min(request.num_max_contacts, 1 << 16)))
    if abi.status_skipped(rec[0]["status"]):
        return result.numContacts()
    if dlb[0] < result.distance_lower_bound:
        result.distance_lower_bound = float(dlb[0])
        if rec[0]["num_contacts"] == 0:  # (a record with a contact carries the contact's points, not the result's)
            result.normal = np.array(rec[0]["normal"])
            result.nearest_points = [np.array(rec[0]["p1"]), np.array(rec[0]["p2"])]
    for c in contacts:
        if result.numContacts() < request.num_max_contacts:
            result.addContact(Contact(tree, solid, c["b1"], c["b2"], c["p1"], c["p2"], c["normal"], c["penetration_depth"]))
    return result.numContacts()


def _distance_octree_through(call, o1, tf1, o2, tf2, request, result):
    """distance() of a checked (OcTree, other) / (other, OcTree) pair through `call`, a batch method of engine.Library: the walk starts
    fresh and the result is merged by DistanceResult::update -- o1 the tree and b1 its node, whichever the caller's order."""
    swapped = not isinstance(o1, OcTree)
    tree, tft, other, tfo = (o2, tf2, o1, tf1) if swapped else (o1, tf1, o2, tf2)
    ctx = _context()
    sid, tid = ctx.add(other), ctx.add_octree(tree)
    r = _one_listed_query(functools.partial(call, ctx.library()), tid, sid, tft, tfo, request, swapped)[0]
    d = float(r["distance"])
    if result.min_distance > d:  # DistanceResult::update
        result.min_distance, result.o1, result.o2 = d, tree, other
        result.b1, result.b2 = int(r["b1"]), int(r["b2"])
        result.normal = np.array(r["normal"])
        result.nearest_points = [np.array(r["p1"]), np.array(r["p2"])]
    return d


def _distance_octree(o1, tf1, o2, tf2, request, result):
    """(OcTree, solid) or (solid, OcTree) through hfcl_octree_distance_batch: the reference's ordered walk.  Either order gets the
    octree-first result (src/distance.cpp swaps back only for BVH and height fields): result.o1 is the tree, b1 its node.  The walk of
    the reference runs on the caller's DistanceResult, so a minimum it already holds would prune this walk too; here the walk starts
    fresh and the result is merged by DistanceResult::update."""
    return _distance_octree_through(engine.Library.octree_distance, o1, tf1, o2, tf2, request, result)


def distance_octree_mesh(o1, tf1, o2, tf2, request, result):
    """distance() between an OcTree and a BVHModel<OBBRSS>, either operand order, through hfcl_octree_mesh_distance_batch
    (hppfcl_amd_octree_mesh_distance.h): the reference's ordered dual walk.  A call of its own BESIDE the dispatch: distance() and
    ComputeDistance keep refusing the pair (taking it there is the follow-up; two tests hold the refusal).  Either order gets the
    octree-first result: result.o1 is the tree and result.o2 the mesh, b1 the node and b2 the triangle, nearest_points and normal the
    record's.  The walk starts fresh and the result is merged by DistanceResult::update, as distance() does for an octree."""
    t1, t2 = isinstance(o1, OcTree), isinstance(o2, OcTree)
    if t1 == t2 or not engine.octree_mesh_distance_pair_supported(int((o2 if t1 else o1).getNodeType())):
        raise ValueError("Distance function between node type %d and node type %d is not yet supported." % (o1.getNodeType(), o2.getNodeType()))
    if result.min_distance <= 0:  # DistanceRequest::isSatisfied
        return result.min_distance
    return _distance_octree_through(engine.Library.octree_mesh_distance, o1, tf1, o2, tf2, request, result)


def collide(*args):
    """collide(o1, tf1, o2, tf2, request, result) or collide(obj1, obj2, request, result)  (python/collision.cc:257-266)"""
    if len(args) == 4:
        a, b, request, result = args
        o1, tf1, o2, tf2 = a.collisionGeometry(), a.getTransform(), b.collisionGeometry(), b.getTransform()
    else:
        o1, tf1, o2, tf2, request, result = args
    if request.security_margin == -np.inf:  # src/collision.cpp:73-76
        result.clear()
        return 0
    if request.num_max_contacts == 0:
        raise ValueError("Invalid number of max contacts (current value is 0).")
    _check_pair(o1, o2, False)
    if result.isCollision() and request.num_max_contacts <= result.numContacts():
        return result.numContacts()
    if isinstance(o1, HeightFieldAABB) or isinstance(o2, HeightFieldAABB):
        return _collide_hfield(o1, tf1, o2, tf2, request, result)
    if isinstance(o1, OcTree) or isinstance(o2, OcTree):
        return _collide_octree(o1, tf1, o2, tf2, request, result)
    rec, g, contacts = _run("collide", [(o1, tf1, o2, tf2)], request)
    _fill_collision(result, o1, o2, request, rec[0], g[0] if g is not None else None, contacts)
    return result.numContacts()


def distance(*args):
    """distance(o1, tf1, o2, tf2, request, result) or distance(obj1, obj2, request, result)  (python/distance.cc:150-159)"""
    if len(args) == 4:
        a, b, request, result = args
        o1, tf1, o2, tf2 = a.collisionGeometry(), a.getTransform(), b.collisionGeometry(), b.getTransform()
    else:
        o1, tf1, o2, tf2, request, result = args
    _check_pair(o1, o2, True)
    if result.min_distance <= 0:  # DistanceRequest::isSatisfied
        return result.min_distance
    if isinstance(o1, OcTree) or isinstance(o2, OcTree):
        return _distance_octree(o1, tf1, o2, tf2, request, result)
    rec, g, _ = _run("distance", [(o1, tf1, o2, tf2)], request)
    r = rec[0]
    d = float(r["distance"])
    if result.min_distance > d:  # DistanceResult::update
        result.min_distance, result.o1, result.o2 = d, o1, o2
        result.b1, result.b2 = int(r["b1"]), int(r["b2"])
        result.normal = np.array(r["normal"])
        result.nearest_points = [np.array(r["p1"]), np.array(r["p2"])]
    result.cached_gjk_guess = np.array(g[0]["gjk_guess"])
    result.cached_support_func_guess = np.array(g[0]["support_guess"])
    request.updateGuess(result)
    return d


class ComputeCollision:  # collision.h:79-117
    def __init__(self, o1, o2):
        _check_pair(o1, o2, False)
        self.o1, self.o2 = o1, o2

    def __call__(self, tf1, tf2, request, result):
        return collide(self.o1, tf1, self.o2, tf2, request, result)


class ComputeDistance:  # distance.h:74-112
    def __init__(self, o1, o2):
        _check_pair(o1, o2, True)
        self.o1, self.o2 = o1, o2

    def __call__(self, tf1, tf2, request, result):
        return distance(self.o1, tf1, self.o2, tf2, request, result)


# ---- broadphase hand-off (collision_object.h:215-357, broadphase_callbacks.h, default_broadphase_callbacks.h) ----
class CollisionObject:
    def __init__(self, cgeom, tf=None):
        self._g, self._tf = cgeom, tf if tf is not None else Transform3f()

    def collisionGeometry(self):
        return self._g

    def getTransform(self):
        return self._tf

    def setTransform(self, tf):
        self._tf = tf

    def getTranslation(self):
        return self._tf.getTranslation()

    def setTranslation(self, T):
        self._tf.setTranslation(T)


class CollisionCallBackCollect:  # default_broadphase_callbacks.h:200-230
    def __init__(self, max_size):
        self.max_size, self._pairs = int(max_size), []

    def collide(self, o1, o2):
        if len(self._pairs) < self.max_size:
            self._pairs.append((o1, o2))
        return False

    def numCollisionPairs(self):
        return len(self._pairs)

    def getCollisionPairs(self):
        return list(self._pairs)

    def init(self):
        self._pairs = []


class _CollisionData:
    def __init__(self):
        self.request, self.result, self.done = CollisionRequest(), CollisionResult(), False


class CollisionCallBackDefault:  # default_broadphase_callbacks.h:129-145: one shared, accumulating CollisionResult
    def __init__(self):
        self.data = _CollisionData()

    def init(self):
        self.data.result.clear()
        self.data.done = False


def collide_pairs(pairs, request):
    """Batched narrow phase on collected (CollisionObject, CollisionObject) pairs: ONE device call; one fresh
    CollisionResult per pair."""
    if not pairs:
        return []
    for a, b in pairs:
        _check_pair(a.collisionGeometry(), b.collisionGeometry(), False)
    quad = [(a.collisionGeometry(), a.getTransform(), b.collisionGeometry(), b.getTransform()) for a, b in pairs]
    rec, g, contacts = _run("collide", quad, request)
    out = []
    for i, (a, b) in enumerate(pairs):
        r = CollisionResult()
        _fill_collision(r, a.collisionGeometry(), b.collisionGeometry(), request, rec[i], g[i] if g is not None else None,
                        contacts, i)
        out.append(r)
    return out


def _scene_run(kind, objects, pair_indices, request, transforms, broadphase=False, inflate=0.0, nearest_bound=None, groups=None, n_moving=None):
    """The pair list `pair_indices` ((n_pairs, 2) indices into `objects`) for every configuration: ONE scene call.  broadphase: the
    list is culled per configuration on the device first (boxes grown by `inflate`); rec / g then hold the surviving queries only and
    the last two items are their ids q = c * n_pairs + p and conf_begin (None without broadphase).  nearest_bound (distance only): the
    pruned minimum (engine.Scene.nearest; with broadphase="self" engine.Scene.nearest_self, with broadphase="env" engine.Scene.nearest_env,
    the summaries then being its clearances) with
    that upper bound; rec then holds one min record per configuration and g is None.
    groups (broadphase="self" or "env"): (object_group, collides) for engine.Scene.set_groups.
    broadphase="env", n_moving=K: as "self" for a scene whose objects[K:] stand still at their own transforms (engine.Scene.set_environment);
    `transforms` then holds the K moving objects' alone, and no pair of two environment objects is listed."""
    ctx = _context()
    geoms = [o.collisionGeometry() for o in objects]
    ids = np.array([ctx.add(g) for g in geoms], dtype=np.uint32)
    env = isinstance(broadphase, str) and broadphase == "env"
    self_pairs = isinstance(broadphase, str) and broadphase == "self" or env
    if isinstance(broadphase, str) and not self_pairs:
        raise ValueError('broadphase: False, True, "self" or "env"')
    if groups is not None and not self_pairs:
        raise ValueError('groups filter the pairs the device finds itself: they need broadphase="self" or "env" (a pair list already says which pairs)')
    if env != (n_moving is not None):
        raise ValueError('broadphase="env" and n_moving go together')
    if env and not 0 <= int(n_moving) <= len(objects):
        raise ValueError("n_moving outside the objects")
    n_table = int(n_moving) if env else len(objects)  # objects a configuration of `transforms` holds
    pr = np.ascontiguousarray([] if self_pairs or pair_indices is None else pair_indices, dtype=np.uint32).reshape(-1, 2)
    if len(pr) and int(pr.max()) >= len(objects):
        raise ValueError("pair index outside the objects")
    types = np.array([g.getNodeType() for g in geoms], dtype=np.int64)
    if self_pairs:  # (any two objects can meet: kinds (a, b) with an object of kind a in front of one of kind b)
        first = {int(t): int(np.flatnonzero(types == t)[0]) for t in np.unique(types)}
        last = {int(t): int(np.flatnonzero(types == t)[-1]) for t in np.unique(types)}
        kinds = [(a, b) for a in first for b in first if first[a] < last[b]]
    else:
        kinds = np.unique(types[pr], axis=0) if len(pr) else ()
    for t1, t2 in kinds:  # (the distinct kind pairs: a few, whatever the list's length)
        if not engine.dll().hfcl_pair_supported(int(t1), int(t2), int(kind == "distance")):
            raise ValueError("%s function between node type %d and node type %d is not yet supported." %
                             ("Distance" if kind == "distance" else "Collision", t1, t2))
    own = lambda objs: np.concatenate([o.getTransform()._abi().reshape(1, 12) for o in objs] + [np.zeros((0, 12))])  # noqa: E731
    if transforms is None:
        table = own(objects[:n_table]).reshape(1, n_table, 12)
    elif isinstance(transforms, np.ndarray):
        table = np.ascontiguousarray(transforms, dtype=np.float64)
        table = table.reshape(-1, n_table, 12) if n_table else table.reshape(len(table) if table.ndim == 3 else 0, 0, 12)
    else:
        table = np.stack([np.concatenate([t._abi().reshape(1, 12) for t in conf]) for conf in transforms])
    lib = ctx.library()
    sc = lib.scene(ids, pr)
    try:
        ids = conf_begin = None
        if groups is not None:
            sc.set_groups(*groups)
        if env:
            sc.set_environment(n_table, own(objects[n_table:]))
        if env and nearest_bound is not None:  # (summ: the clearances, hfcl_scene_clearance)
            summ, rec, _ = sc.nearest_env(table, request._abi(), float(nearest_bound))
            g = None
        elif env:
            fn = sc.distance_env if kind == "distance" else sc.collide_env
            rec, ids, conf_begin, summ, g = fn(table, request._abi(), float(inflate), records=True, want_guess=True)
        elif nearest_bound is not None and self_pairs:  # (summ: the clearances, hfcl_scene_clearance)
            summ, rec, _ = sc.nearest_self(table, request._abi(), float(nearest_bound))
            g = None
        elif nearest_bound is not None:
            summ, rec, _ = sc.nearest(table, request._abi(), float(nearest_bound))
            g = None
        elif self_pairs:  # (ids: the listed pairs (i, j) themselves)
            fn = sc.distance_self if kind == "distance" else sc.collide_self
            rec, ids, conf_begin, summ, g = fn(table, request._abi(), float(inflate), records=True, want_guess=True)
        elif broadphase:
            fn = sc.distance_culled if kind == "distance" else sc.collide_culled
            rec, ids, conf_begin, summ, g = fn(table, float(inflate), request._abi(), records=True, summary=True, want_guess=True)
        else:
            fn = sc.distance if kind == "distance" else sc.collide
            rec, summ, g = fn(table, request._abi(), records=True, summary=True, want_guess=True)
    except engine.EngineError as e:
        if e.code in (abi.ERR_INVALID_ARGUMENT, abi.ERR_UNSUPPORTED_PAIR):
            raise ValueError(str(e))  # std::invalid_argument in the reference
        raise
    finally:
        sc.close()
    return geoms, pr, len(table), rec, summ, g, ids, conf_begin


def collide_scene(objects, pair_indices, request, transforms=None, broadphase=False, inflate=0.0, groups=None, n_moving=None):
    """collide() on the listed pairs of `objects` (CollisionObjects) through a scene: each object's pose goes to the device
    once per configuration, not once per pair.  transforms: None -- one configuration, the objects' own transforms --, an
    array (n_conf, n_objects, 12) of Transform3f images, or n_conf lists of Transform3f.  Returns (results, summaries):
    results[c][p] is the CollisionResult collide_pairs gives for pair p under configuration c (a flat list of n_pairs when
    transforms is None), summaries the abi.SCENE_SUMMARY_DTYPE record of every configuration (n_contacts > 0: what
    CollisionCallBackDefault's result.isCollision() says after manager.collide).  The results are Python objects, filled one by
    one: for lists of 10^5 pairs and more that loop costs far more than the device call -- take the summaries, or the records of
    engine.Scene.collide, there.
    broadphase=True: per configuration only the listed pairs whose world AABBs (each grown by `inflate` >= 0 on every side) overlap
    are evaluated -- with inflate = 0 the pairs DynamicAABBTreeCollisionManager::collide passes to its callback; the test runs on the
    device (engine.Scene.collide_culled).  results[c] is then a list of (p, CollisionResult) for the surviving pairs, p ascending, and
    the summaries are folds over those (n_contacts and first_contact as without the broadphase).
    broadphase="self": no list at all -- `pair_indices` is ignored (None will do): per configuration the device finds every pair (i < j)
    of `objects` whose grown world AABBs overlap (engine.Scene.collide_self) and evaluates those.  results[c] is a list of
    ((i, j), CollisionResult), i then j ascending; min_pair / first_contact of a summary are positions in that list.
    groups=(object_group, collides), with broadphase="self" only: a group per object and the symmetric group matrix ((G, G) bools or G
    uint64 words, G <= 64) -- only pairs whose groups may pair are found (engine.Scene.set_groups; engine.groups_between gives
    collide(otherManager, callback), engine.groups_excluding an allowed-collision matrix).
    broadphase="env", n_moving=K: a robot among a static environment.  objects[K:] keep their own transforms as the environment, which goes
    to the device once with its boxes (engine.Scene.set_environment; put the robot first and the obstacles in engine.spatial_order);
    `transforms` is (n_conf, K, 12) -- the moving objects' poses alone (None: their own).  The results are those of broadphase="self"
    on the full transforms less every pair of two environment objects; `groups` works as with "self"."""
    if request.num_max_contacts == 0:
        raise ValueError("Invalid number of max contacts (current value is 0).")
    if request.num_max_contacts > 1 and any(isinstance(o.collisionGeometry(), BVHModelOBBRSS) for o in objects):
        raise ValueError("collide_scene: contact lists of mesh pairs (num_max_contacts > 1) go through collide_pairs")
    geoms, pr, n_conf, rec, summ, g, ids, conf_begin = _scene_run("collide", objects, pair_indices, request, transforms, broadphase, inflate,
                                                                    groups=groups, n_moving=n_moving)
    out = []
    for c in range(n_conf):
        row = []
        if broadphase in ("self", "env"):  # ((i, j), result) of configuration c's touching pairs
            for k in range(int(conf_begin[c]), int(conf_begin[c + 1])):
                i, j = int(ids[k][0]), int(ids[k][1])
                r = CollisionResult()
                _fill_collision(r, geoms[i], geoms[j], request, rec[k], g[k], None, k - int(conf_begin[c]))
                row.append(((i, j), r))
        elif broadphase:  # (p, result) of configuration c's surviving pairs
            for k in range(int(conf_begin[c]), int(conf_begin[c + 1])):
                p = int(ids[k]) - c * len(pr)
                r = CollisionResult()
                _fill_collision(r, geoms[pr[p][0]], geoms[pr[p][1]], request, rec[k], g[k], None, p)
                row.append((p, r))
        else:
            for p, (i, j) in enumerate(pr):
                r = CollisionResult()
                q = c * len(pr) + p
                _fill_collision(r, geoms[i], geoms[j], request, rec[q], g[q], None, p)
                row.append(r)
        out.append(row)
    return (out[0] if transforms is None and out else out), summ


def distance_scene(objects, pair_indices, request, transforms=None, broadphase=False, inflate=0.0, nearest=False, upper_bound=float("inf"),
                   groups=None, n_moving=None):
    """distance() on the listed pairs of `objects`: (min_distance array (n_conf, n_pairs), records, summaries); the
    summaries' min_distance is DistanceCallBackDefault's answer per configuration.
    broadphase=True: only the pairs whose world AABBs, each grown by `inflate`, overlap are evaluated (inflate = D / 2 keeps every pair
    whose boxes are within D along each axis: a box-shaped filter, not the manager's traversal with its shrinking bound).  Returns
    (distances, pair indices, summaries): per configuration the array of the surviving pairs' distances and the array of their p.
    broadphase="self": `pair_indices` is ignored; the device finds every pair (i < j) whose grown boxes overlap (engine.Scene.distance_self);
    the second item is then per configuration the (k, 2) array of those pairs.  groups=(object_group, collides), with broadphase="self"
    only: as in collide_scene.
    nearest=True: the clearance alone -- one DistanceResult per configuration, what DistanceCallBackDefault leaves behind after
    DynamicAABBTreeCollisionManager::distance: the closest listed pair's min_distance, o1 / o2, nearest points, normal, b1 / b2.  The pairs
    are pruned on the device by a bound from their world boxes (engine.Scene.nearest); a configuration whose closest pair is farther than
    `upper_bound` keeps a default DistanceResult.  With broadphase="self" there is no list and no inflate: the clearance over every
    pair (i < j) the `groups` allow, the pairs made and pruned on the device (engine.Scene.nearest_self) --
    DynamicAABBTreeCollisionManager::distance(otherManager, DistanceCallBackDefault) with two groups.
    broadphase="env", n_moving=K: as in collide_scene -- objects[K:] are the environment, `transforms` is (n_conf, K, 12); the items are
    those of "self".  With nearest=True: the clearance of the K moving objects among themselves and against the environment
    (engine.Scene.nearest_env), never a pair of two environment objects."""
    self_pairs = isinstance(broadphase, str) and broadphase in ("self", "env")
    if nearest and groups is not None and not self_pairs:
        raise ValueError('groups need broadphase="self" or "env": the pruned minimum (nearest=True) runs on the pair list')
    if nearest:
        geoms, pr, n_conf, rec, summ, _, _, _ = _scene_run("distance", objects, pair_indices, request, transforms, broadphase if self_pairs else False,
                                                           nearest_bound=upper_bound, groups=groups, n_moving=n_moving)
        out = []
        for c in range(n_conf):
            res = DistanceResult()
            r = rec[c]
            if self_pairs:
                i, j = int(summ["min_i"][c]), int(summ["min_j"][c])
            else:
                p = int(summ["min_pair"][c])
                i, j = (int(pr[p][0]), int(pr[p][1])) if p != abi.SCENE_NONE else (abi.SCENE_NONE, abi.SCENE_NONE)
            if i != abi.SCENE_NONE and float(summ["min_distance"][c]) <= upper_bound:
                res.min_distance, res.o1, res.o2 = float(r["distance"]), geoms[i], geoms[j]
                res.b1, res.b2 = int(r["b1"]), int(r["b2"])
                res.normal = np.array(r["normal"])
                res.nearest_points = [np.array(r["p1"]), np.array(r["p2"])]
            out.append(res)
        return out
    geoms, pr, n_conf, rec, summ, g, ids, conf_begin = _scene_run("distance", objects, pair_indices, request, transforms, broadphase, inflate,
                                                                    groups=groups, n_moving=n_moving)
    if broadphase in ("self", "env"):  # (distances, (i, j) arrays, summaries): no list; the device finds the pairs whose grown boxes overlap
        cb = conf_begin.astype(np.int64)
        return [rec["distance"][cb[c]:cb[c + 1]] for c in range(n_conf)], [ids[cb[c]:cb[c + 1]] for c in range(n_conf)], summ
    if broadphase:
        cb = conf_begin.astype(np.int64)
        return ([rec["distance"][cb[c]:cb[c + 1]] for c in range(n_conf)],
                [ids[cb[c]:cb[c + 1]].astype(np.int64) - c * len(pr) for c in range(n_conf)], summ)
    return rec["distance"].reshape(n_conf, len(pr)), rec, summ


def collide_terrain(objects, field, field_tf, request, transforms=None, object_indices=None):
    """A HeightFieldAABB under `objects` (CollisionObjects): DynamicAABBTreeCollisionManager::collide(terrain, CollisionCallBackDefault), or
    the loop of collide(field, field_tf, o, tf_o) over a robot's links, for every configuration in ONE scene call
    (engine.Scene.collide_terrain).  object_indices: the strictly ascending indices of the objects tested against the ground; None: every
    object whose geometry has an evaluator against a height field.  transforms: as collide_scene -- None (one configuration, the objects'
    own), an array (n_conf, n_objects, 12), or n_conf lists of Transform3f.  Returns (results, summaries): results[c][k] is the
    CollisionResult collide(field, field_tf, objects[object_indices[k]], ...) gives under configuration c (a flat list when transforms
    is None); summaries the abi.SCENE_SUMMARY_DTYPE record of every configuration -- min_distance the smallest
    distance_lower_bound, min_pair / first_contact indices into `objects`, n_contacts > 0: isCollision() of the default callback."""
    if request.num_max_contacts == 0:
        raise ValueError("Invalid number of max contacts (current value is 0).")
    if not isinstance(field, HeightFieldAABB):
        raise ValueError("collide_terrain: the terrain is a HeightFieldAABB")
    ctx = _context()
    geoms = [o.collisionGeometry() for o in objects]
    if object_indices is None:
        listed = [i for i, g in enumerate(geoms) if engine.hfield_pair_supported(int(g.getNodeType()))]
    else:
        listed = [int(i) for i in object_indices]
        if any(i < 0 or i >= len(objects) for i in listed):
            raise ValueError("object index outside the objects")
    ids = np.array([ctx.add(g) for g in geoms], dtype=np.uint32)
    hid = ctx.add_hfield(field)
    n = len(objects)
    if transforms is None:
        table = np.concatenate([o.getTransform()._abi().reshape(1, 12) for o in objects] + [np.zeros((0, 12))]).reshape(1, n, 12)
    elif isinstance(transforms, np.ndarray):
        table = np.ascontiguousarray(transforms, dtype=np.float64)
        table = table.reshape(-1, n, 12) if n else table.reshape(len(table) if table.ndim == 3 else 0, 0, 12)
    else:
        table = np.stack([np.concatenate([t._abi().reshape(1, 12) for t in conf]) for conf in transforms])
    lib = ctx.library()
    sc = lib.scene(ids, np.zeros((0, 2), dtype=np.uint32))
    try:
        sc.set_terrain(hid, field_tf._abi().reshape(12), np.array(listed, dtype=np.uint32))
        cap = int(min(request.num_max_contacts, 1 << 16)) * len(table) * len(listed)
        rec, dlb, summ, contacts, _ = sc.collide_terrain(table, request._abi(), max_contacts=cap)
    except engine.EngineError as e:
        if e.code in (abi.ERR_INVALID_ARGUMENT, abi.ERR_UNSUPPORTED_PAIR, abi.ERR_LIMIT):
            raise ValueError(str(e))  # std::invalid_argument in the reference
        raise
    finally:
        sc.close()
    starts = np.searchsorted(contacts["pair"], np.arange(len(rec) + 1))  # (the contacts come in query order)
    out = []
    for c in range(len(table)):
        row = []
        for k, i in enumerate(listed):
            q = c * len(listed) + k
            r = CollisionResult()
            if not abi.status_skipped(rec[q]["status"]):
                if dlb[q] < r.distance_lower_bound:
                    r.distance_lower_bound = float(dlb[q])
                    r.normal = np.array(rec[q]["normal"])
                    r.nearest_points = [np.array(rec[q]["p1"]), np.array(rec[q]["p2"])]
                for h in contacts[starts[q]:starts[q + 1]]:
                    if r.numContacts() < request.num_max_contacts:
                        r.addContact(Contact(field, geoms[i], h["b1"], h["b2"], h["p1"], h["p2"], h["normal"], h["penetration_depth"]))
            row.append(r)
        out.append(row)
    return (out[0] if transforms is None else out), summ


class DynamicAABBTreeCollisionManager:  # broadphase_dynamic_AABB_tree.h (candidate set = all AABB-overlapping pairs)
    def __init__(self):
        self._objs, self._aabbs = [], None

    def registerObject(self, obj):
        self._objs.append(obj)
        self._aabbs = None

    def registerObjects(self, objs):
        for o in objs:
            self.registerObject(o)

    def unregisterObject(self, obj):
        self._objs = [o for o in self._objs if o is not obj]
        self._aabbs = None

    def size(self):
        return len(self._objs)

    def empty(self):
        return not self._objs

    def clear(self):
        self._objs, self._aabbs = [], None

    def update(self, *_):
        self._aabbs = None

    def _world_aabbs(self, objs):
        L = geometry.ShapeLibrary()
        ids = np.array([o.collisionGeometry()._register(L) for o in objs], dtype=np.uint32)
        tf = np.concatenate([o.getTransform()._abi().reshape(1, 12) for o in objs])
        return engine.world_aabbs(L, ids, tf)

    def setup(self):
        self._aabbs = self._world_aabbs(self._objs) if self._objs else np.zeros((0, 6))

    def _candidates(self, other=None):
        if self._aabbs is None:
            self.setup()
        if other is None:
            idx = engine.broadphase_self_pairs(self._aabbs) if len(self._objs) > 1 else np.zeros((0, 2), dtype=np.uint32)
            return [(self._objs[i], self._objs[j]) for i, j in idx]
        box = self._world_aabbs([other])
        idx = engine.broadphase_pairs_between(box, self._aabbs) if self._objs else np.zeros((0, 2), dtype=np.uint32)
        return [(other, self._objs[j]) for _, j in idx]

    def collide(self, *args):
        """collide(callback): self pairs; collide(obj, callback): obj against the managed objects."""
        other, callback = (None, args[0]) if len(args) == 1 else args
        cand = self._candidates(other)
        if isinstance(callback, CollisionCallBackDefault):
            d = callback.data
            for (a, b), r in zip(cand, collide_pairs(cand, d.request)):
                for c in r.getContacts():  # the default callback accumulates into one result
                    if d.result.numContacts() < d.request.num_max_contacts:
                        d.result.addContact(c)
                d.result.distance_lower_bound = min(d.result.distance_lower_bound, r.distance_lower_bound)
                if d.result.isCollision() and d.result.numContacts() >= d.request.num_max_contacts:
                    d.done = True
                    break
            return
        for a, b in cand:
            if callback.collide(a, b):
                break


# ---- contact patches: hpp::fcl::computeContactPatch (src/contact_patch.cpp:48-120, collision_data.h:519-980) -------------
class ContactPatchRequest:  # collision_data.h:726-823
    def __init__(self, max_num_patch=1, num_samples_curved_shapes=12, patch_tolerance=1e-3):
        if isinstance(max_num_patch, CollisionRequest):
            max_num_patch = max_num_patch.num_max_contacts
        self.max_num_patch = int(max_num_patch)
        self.setNumSamplesCurvedShapes(num_samples_curved_shapes)
        self.setPatchTolerance(patch_tolerance)

    def setNumSamplesCurvedShapes(self, n):
        self._ns = 3 if n < 3 else int(n)

    def getNumSamplesCurvedShapes(self):
        return self._ns

    def setPatchTolerance(self, tol):
        self._tol = 1e-12 if tol < 0 else float(tol)

    def getPatchTolerance(self):
        return self._tol

    def _abi(self):
        return abi.default_patch_request(self.max_num_patch, self._ns, self._tol)


class ContactPatch:  # collision_data.h:519-717 (the patch frame's z axis is the normal; points are 2-D in that frame)
    DEFAULT, INVERTED = 0, 1

    def __init__(self, preallocated_size=12):
        self.tf = Transform3f()
        self.direction = ContactPatch.DEFAULT
        self.penetration_depth = 0.0
        self._points = []

    def size(self):
        return len(self._points)

    def getNormal(self):
        n = self.tf.getRotation()[:, 2].copy()
        return -n if self.direction == ContactPatch.INVERTED else n

    def addPoint(self, p3):
        q = self.tf.getRotation().T @ (_v3(p3) - self.tf.getTranslation())
        self._points.append(q[:2].copy())

    def point(self, i):
        if not self._points:
            raise RuntimeError("Patch is empty.")
        return self._points[min(i, len(self._points) - 1)]

    def points(self):
        return list(self._points)

    def getPoint(self, i):
        p = self.point(i)
        return self.tf.transform(np.array([p[0], p[1], 0.0]))

    def getPointShape1(self, i):
        return self.getPoint(i) - (self.penetration_depth / 2) * self.getNormal()

    def getPointShape2(self, i):
        return self.getPoint(i) + (self.penetration_depth / 2) * self.getNormal()

    def clear(self):
        self._points = []
        self.tf = Transform3f()
        self.penetration_depth = 0.0

    def isSame(self, other, tol=1e-12):  # collision_data.h:660-704
        def approx(a, b):
            return np.linalg.norm(a - b) <= tol * min(np.linalg.norm(a), np.linalg.norm(b))
        if not approx(self.getNormal(), other.getNormal()):
            return False
        if abs(self.penetration_depth - other.penetration_depth) > tol or self.direction != other.direction:
            return False
        if self.size() != other.size():
            return False
        theirs = [other.getPoint(j) for j in range(other.size())]
        return all(any(approx(self.getPoint(i), q) for q in theirs) for i in range(self.size()))


def constructContactPatchFrameFromContact(contact, patch):  # collision_data.h:706-713 (numpy arithmetic: for building expected patches)
    n = np.asarray(contact.normal, dtype=np.float64)
    x, y, z = n
    if not (abs(x) <= abs(z) * 1e-12) or not (abs(y) <= abs(z) * 1e-12):
        inv = 1.0 / np.sqrt(x * x + y * y)
        u = np.array([-y * inv, x * inv, 0.0])
    else:
        inv = 1.0 / np.sqrt(y * y + z * z)
        u = np.array([0.0, -z * inv, y * inv])
    R = np.zeros((3, 3))
    R[:, 2] = n / np.sqrt(n @ n) if n @ n > 0 else n
    R[:, 1] = -u
    R[:, 0] = np.cross(R[:, 1], n)
    patch.penetration_depth = contact.penetration_depth
    patch.tf = Transform3f(R, contact.pos)
    patch.direction = ContactPatch.DEFAULT


class ContactPatchResult:  # collision_data.h:826-981
    def __init__(self, request=None):
        self._patches = []

    def numContactPatches(self):
        return len(self._patches)

    def getContactPatch(self, i):
        if not self._patches:
            raise ValueError("The number of contact patches is zero. No ContactPatch can be returned.")
        return self._patches[min(i, len(self._patches) - 1)]

    def contactPatch(self, i):
        return self.getContactPatch(i)

    def clear(self):
        self._patches = []

    def set(self, request):
        self.clear()


def computeContactPatch(*args):
    """computeContactPatch(o1, tf1, o2, tf2, collision_result, request, result) or (obj1, obj2, collision_result, request, result):
    one patch per contact of the collision result, at most request.max_num_patch, computed on the device from the contacts."""
    if len(args) == 5:
        a, b, col_res, request, result = args
        o1, tf1, o2, tf2 = a.collisionGeometry(), a.getTransform(), b.collisionGeometry(), b.getTransform()
    else:
        o1, tf1, o2, tf2, col_res, request, result = args
    if not col_res.isCollision() or request.max_num_patch == 0:  # src/contact_patch.cpp:54-57
        return
    result.set(request)
    if not engine.patch_supported(int(o1.getNodeType()), int(o2.getNodeType())):
        raise ValueError("Contact patch computation between node type %d and node type %d is not yet supported." %
                         (o1.getNodeType(), o2.getNodeType()))
    ctx = _context()
    i1, i2 = ctx.add(o1), ctx.add(o2)
    lib = ctx.library()
    contacts = col_res.getContacts()[:request.max_num_patch]
    n = len(contacts)
    rec = np.zeros(n, dtype=abi.RESULT_DTYPE)
    for k, c in enumerate(contacts):
        rec[k]["distance"] = c.penetration_depth
        rec[k]["normal"] = c.normal
        rec[k]["p1"], rec[k]["p2"] = c.nearest_points
        rec[k]["b1"], rec[k]["b2"] = c.b1, c.b2
        rec[k]["num_contacts"] = 1
    guess = np.zeros(n, dtype=abi.GUESS_DTYPE)
    guess["support_guess"] = np.asarray(col_res.cached_support_func_guess, dtype=np.int32)
    tfa = np.repeat(tf1._abi().reshape(1, 12), n, axis=0)
    tfb = np.repeat(tf2._abi().reshape(1, 12), n, axis=0)
    out, pts = lib.contact_patch(np.full(n, i1, np.uint32), np.full(n, i2, np.uint32), tfa, tfb, rec, guess, request._abi())
    for k in range(n):
        p = ContactPatch()
        tf = out["tf"][k]
        p.tf = Transform3f(tf[:9].reshape(3, 3).T, tf[9:12])
        p.penetration_depth = float(out["penetration_depth"][k])
        p._points = [pts[k, j].copy() for j in range(int(out["num_points"][k]))]
        result._patches.append(p)


class ComputeContactPatch:  # contact_patch.h:80-120
    def __init__(self, o1, o2):
        if not engine.patch_supported(int(o1.getNodeType()), int(o2.getNodeType())):
            raise ValueError("Contact patch computation between node type %d and node type %d is not yet supported." %
                             (o1.getNodeType(), o2.getNodeType()))
        self.o1, self.o2 = o1, o2

    def __call__(self, tf1, tf2, collision_result, request, result):
        return computeContactPatch(self.o1, tf1, self.o2, tf2, collision_result, request, result)
