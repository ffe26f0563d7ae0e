"""Synthetic workloads of BASELINE.json's configs.  Plumbing: numpy only.

All randomness comes from a counter-based generator (Philox) keyed by (seed, stream) so the
same batch can be regenerated anywhere (host, GPU box, any rank) without shipping data.
Default seed = 1, echoing the reference's unseeded rand() (test/utility.cpp:93-96)."""
import numpy as np

from . import geometry


def _rng(seed, stream):
    return np.random.Generator(np.random.Philox(key=[int(seed), int(stream)]))


def uniform_quaternions(rng, n):
    """uniformRandomQuaternion, include/hpp/fcl/math/transform.h:228-249 -> (w,x,y,z)."""
    u1, u2, u3 = rng.random(n), rng.random(n), rng.random(n)
    m1, m2 = np.sqrt(1.0 - u1), np.sqrt(u1)
    q = np.empty((n, 4))
    q[:, 0] = m1 * np.sin(2 * np.pi * u2)
    q[:, 1] = m1 * np.cos(2 * np.pi * u2)
    q[:, 2] = m2 * np.sin(2 * np.pi * u3)
    q[:, 3] = m2 * np.cos(2 * np.pi * u3)
    return q


def fibonacci_sphere(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    theta = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)


class Batch:
    """One batch of queries: shape library + pair list + poses (both precisions)."""

    def __init__(self, name, lib, s1, s2, quat1, T1, quat2, T2, kind, request_overrides=None):
        self.name = name
        self.lib = lib
        self.shapes = lib.shapes_array()
        self.verts = lib.vertices_array()
        self.s1 = np.ascontiguousarray(s1, dtype=np.uint32)
        self.s2 = np.ascontiguousarray(s2, dtype=np.uint32)
        self.quat1, self.T1, self.quat2, self.T2 = quat1, T1, quat2, T2
        self.kind = kind  # "distance" | "collide"
        self.request_overrides = request_overrides or {}
        self.meshes = None

    def __len__(self):
        return len(self.s1)

    @property
    def tf1(self):
        return geometry.make_pose(quat=self.quat1, T=self.T1)

    @property
    def tf2(self):
        return geometry.make_pose(quat=self.quat2, T=self.T2)

    @property
    def pose1_f32(self):
        return geometry.pose_f32_from_quat(self.quat1, self.T1)

    @property
    def pose2_f32(self):
        return geometry.pose_f32_from_quat(self.quat2, self.T2)

    @property
    def pose1_qt(self):
        """(n, 7) float64 compact host poses (quaternion w, x, y, z + translation) for the *_qt entry points."""
        return np.concatenate([np.asarray(self.quat1, dtype=np.float64), np.asarray(self.T1, dtype=np.float64)], axis=-1)

    @property
    def pose2_qt(self):
        return np.concatenate([np.asarray(self.quat2, dtype=np.float64), np.asarray(self.T2, dtype=np.float64)], axis=-1)

    def tf_from_f32(self):
        """fp64 poses built from the *rounded* fp32 quaternion/translation (what the fp32 path sees)."""
        p1, p2 = self.pose1_f32.astype(np.float64), self.pose2_f32.astype(np.float64)

        def mk(p):
            q = p[:, :4] / np.linalg.norm(p[:, :4], axis=1, keepdims=True)
            return geometry.make_pose(quat=q, T=p[:, 4:7])

        return mk(p1), mk(p2)

    def slice(self, lo, hi):
        b = Batch.__new__(Batch)
        b.__dict__.update(self.__dict__)
        b.s1, b.s2 = self.s1[lo:hi], self.s2[lo:hi]
        b.quat1, b.T1, b.quat2, b.T2 = self.quat1[lo:hi], self.T1[lo:hi], self.quat2[lo:hi], self.T2[lo:hi]
        return b


def _poses(rng, n, half_width):
    q1, q2 = uniform_quaternions(rng, n), uniform_quaternions(rng, n)
    T1 = rng.uniform(-half_width, half_width, (n, 3))
    T2 = rng.uniform(-half_width, half_width, (n, 3))
    return q1, T1, q2, T2


def cfg1_sphere_sphere(n=1000, seed=1):
    """cfg1: Sphere-Sphere distance(), radii U[0.1,1] (test/utility.cpp:565-567)."""
    rng = _rng(seed, 1)
    lib = geometry.ShapeLibrary()
    nlib = 256
    for r in rng.uniform(0.1, 1.0, nlib):
        lib.add_sphere(float(r))
    s1, s2 = rng.integers(0, nlib, n), rng.integers(0, nlib, n)
    q1, T1, q2, T2 = _poses(rng, n, 0.9)
    return Batch("cfg1_sphere_sphere_distance", lib, s1, s2, q1, T1, q2, T2, "distance")


def cfg2_box_capsule(n=1_000_000, seed=1, nlib=1024, half_width=0.92):
    """cfg2: Box-Capsule collide(), default request.  Box side U[0.1,1]^3 (makeRandomBox,
    test/utility.cpp:559-563), Capsule r U[0.1,0.8], lz U[0.2,1.0] (:575-579).  The translation cube is
    sized so ~30 % of the pairs penetrate (the reference's GJK benchmark had 28 % colliding,
    test/benchmark/test_fcl_gjk.output:3)."""
    rng = _rng(seed, 2)
    lib = geometry.ShapeLibrary()
    for s in rng.uniform(0.1, 1.0, (nlib, 3)):
        lib.add_box(*map(float, s))
    for r, lz in zip(rng.uniform(0.1, 0.8, nlib), rng.uniform(0.2, 1.0, nlib)):
        lib.add_capsule(float(r), float(lz))
    s1 = rng.integers(0, nlib, n)
    s2 = nlib + rng.integers(0, nlib, n)
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    return Batch("cfg2_box_capsule_collide", lib, s1, s2, q1, T1, q2, T2, "collide")


def convex_hull_library(rng, nlib, nverts=32):
    lib = geometry.ShapeLibrary()
    base = fibonacci_sphere(nverts)
    for radii in rng.uniform(0.1, 1.0, (nlib, 3)):
        lib.add_convex(base * radii)
    return lib


def cfg3_convex_convex(n=1_000_000, seed=1, nlib=4096, half_width=1.0, nverts=32):
    """cfg3: Convex-Convex distance(), signed, NesterovAcceleration.  Hulls: 32 Fibonacci-sphere
    directions scaled by ellipsoid radii U[0.1,1]^3 (every point is a hull vertex, linear
    support path; no qhull needed).  Shared library of `nlib` hulls."""
    rng = _rng(seed, 3)
    lib = convex_hull_library(rng, nlib, nverts)
    s1, s2 = rng.integers(0, nlib, n), rng.integers(0, nlib, n)
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    from . import abi
    return Batch("cfg3_convex32_distance_nesterov", lib, s1, s2, q1, T1, q2, T2, "distance",
                 {"gjk_variant": abi.NesterovAcceleration})


def cfg3_unique_hulls(n=1_000_000, seed=1, half_width=1.0, nverts=32):
    """cfg3, variant (ii) of SURVEY.md 8d: every pair brings its own two hulls (pair i = hulls 2i, 2i+1 of a
    2n-hull library), so the 2 x 32 x 12 B of vertices are compulsory HBM traffic per query (876 B/query)."""
    rng = _rng(seed, 33)
    base = fibonacci_sphere(nverts)
    radii = rng.uniform(0.1, 1.0, (2 * n, 1, 3))
    lib = geometry.ShapeLibrary()
    lib.add_convex_many(base[None, :, :] * radii)
    s1 = 2 * np.arange(n, dtype=np.int64)
    s2 = s1 + 1
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    from . import abi
    return Batch("cfg3_convex32_unique_hulls_distance_nesterov", lib, s1, s2, q1, T1, q2, T2, "distance",
                 {"gjk_variant": abi.NesterovAcceleration})


def _mixed_library(rng, nper):
    lib = geometry.ShapeLibrary()
    for s in rng.uniform(0.1, 1.0, (nper, 3)):
        lib.add_box(*map(float, s))
    for r in rng.uniform(0.1, 1.0, nper):
        lib.add_sphere(float(r))
    for r, lz in zip(rng.uniform(0.1, 0.8, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_capsule(float(r), float(lz))
    for r in rng.uniform(0.1, 1.0, (nper, 3)):
        lib.add_ellipsoid(*map(float, r))
    base = fibonacci_sphere(32)
    for radii in rng.uniform(0.1, 1.0, (nper, 3)):
        lib.add_convex(base * radii)
    return lib


def all_primitives(n=100_000, seed=1, nper=128, half_width=0.8, kind="collide"):
    """Every supported shape kind against every other (Box, Sphere, Capsule, Cone, Cylinder, Ellipsoid,
    Convex32): exercises the whole dispatch table of shape_shape_func.h:185-211 that is in scope."""
    rng = _rng(seed, 6)
    lib = _mixed_library(rng, nper)
    for r, lz in zip(rng.uniform(0.1, 0.8, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_cone(float(r), float(lz))
    for r, lz in zip(rng.uniform(0.1, 0.8, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_cylinder(float(r), float(lz))
    s1, s2 = rng.integers(0, 7 * nper, n), rng.integers(0, 7 * nper, n)
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    return Batch("all_primitives_" + kind, lib, s1, s2, q1, T1, q2, T2, kind)


def triangle_pairs(n=50_000, seed=1, nper=48, half_width=0.45, kind="collide"):
    """Top-level TriangleP rows of the dispatch table (collision_func_matrix.cpp:295-469): a TriangleP against
    every solid kind, both operand orders, and TriangleP x TriangleP.  collide() only: the reference's distance
    matrix has no TriangleP entries (src/distance_func_matrix.cpp)."""
    rng = _rng(seed, 9)
    lib = _mixed_library(rng, nper)
    for r, lz in zip(rng.uniform(0.1, 0.8, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_cone(float(r), float(lz))
    for r, lz in zip(rng.uniform(0.1, 0.8, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_cylinder(float(r), float(lz))
    base48 = fibonacci_sphere(48)
    for radii in rng.uniform(0.1, 1.0, (nper, 3)):
        lib.add_convex(base48 * radii)  # above the 32-vertex threshold: scanned from memory
    n_solid = 8 * nper
    ntri = 4 * nper
    for k in range(ntri):
        c = rng.uniform(-0.3, 0.3, 3)
        lib.add_triangle(*(c + rng.uniform(-0.6, 0.6, (3, 3))))
    other = rng.integers(0, n_solid + ntri, n)  # a solid or another triangle
    tri = n_solid + rng.integers(0, ntri, n)
    first = rng.integers(0, 2, n).astype(bool)
    s1 = np.where(first, tri, other)
    s2 = np.where(first, other, tri)
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    return Batch("triangle_pairs_" + kind, lib, s1, s2, q1, T1, q2, T2, kind)


def flat_pairs(n=50_000, seed=1, nper=64, half_width=1.0, kind="collide"):
    """Plane / Halfspace rows of the dispatch table: (solid, flat), (flat, solid) and (flat, flat) pairs, the
    solids being every other supported kind (some with a swept-sphere radius)."""
    rng = _rng(seed, 7)
    lib = _mixed_library(rng, nper)
    for r, lz in zip(rng.uniform(0.1, 0.8, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_cone(float(r), float(lz))
    for r, lz in zip(rng.uniform(0.1, 0.8, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_cylinder(float(r), float(lz), swept_sphere_radius=float(rng.uniform(0, 0.1)))
    n_solid = 7 * nper
    nflat = 2 * nper
    for k in range(nflat):
        nrm, d, ssr = rng.normal(size=3), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(0, 0.05)) * (k % 3 == 0)
        if k % 8 == 0:
            nrm = np.array([0.0, 0.0, 1.0])  # parallel flats when both poses share a rotation
        (lib.add_halfspace if k % 2 == 0 else lib.add_plane)(nrm, d, swept_sphere_radius=ssr)
    u = rng.random(n)
    solid, flat1, flat2 = rng.integers(0, n_solid, n), n_solid + rng.integers(0, nflat, n), n_solid + rng.integers(0, nflat, n)
    s1 = np.where(u < 0.45, solid, flat1)
    s2 = np.where(u < 0.45, flat2, np.where(u < 0.9, solid, flat2))
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    par = rng.random(n) < 0.3  # same rotation on both sides: exercises the parallel branches of flat-flat
    q2[par] = q1[par]
    return Batch("flat_pairs_" + kind, lib, s1, s2, q1, T1, q2, T2, kind)


def hull_adjacency(points):
    """Vertex adjacency of a convex point set as Convex<Triangle>::fillNeighbors builds it (shape/details/convex.hxx:
    231-280: per vertex the ascending set of vertices it shares a facet edge with), from the facets of scipy's Qhull
    wrapper.  Returns CSR (offsets[n + 1], ids) for hfcl_lib_set_convex_neighbors / Library.set_convex_neighbors."""
    from scipy.spatial import ConvexHull
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    hull = ConvexHull(pts)
    edges = np.concatenate([hull.simplices[:, [0, 1]], hull.simplices[:, [1, 2]], hull.simplices[:, [2, 0]]])
    edges = np.concatenate([edges, edges[:, ::-1]])
    edges = np.unique(edges, axis=0)  # sorted by (vertex, neighbour)
    offs = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(np.bincount(edges[:, 0], minlength=n), out=offs[1:])
    return offs, edges[:, 1].astype(np.uint32)


def subdivided_box(m=11, half=(1.0, 1.0, 1.0)):
    """A box whose faces are m x m grids of points, triangulated: (points, offsets, ids).  Most of its points are NOT
    extreme -- they lie inside a flat facet or an edge, with every neighbour in that facet's plane -- which is what a
    meshed CAD part handed to Convex<Triangle> looks like (m = 11: 602 points, above the hill-climb threshold)."""
    idx = {}
    pts = []
    for i in range(m):
        for j in range(m):
            for k in range(m):
                if i in (0, m - 1) or j in (0, m - 1) or k in (0, m - 1):
                    idx[(i, j, k)] = len(pts)
                    pts.append([half[0] * (2.0 * i / (m - 1) - 1), half[1] * (2.0 * j / (m - 1) - 1), half[2] * (2.0 * k / (m - 1) - 1)])
    nb = [set() for _ in pts]

    def edge(a, b):
        nb[a].add(b)
        nb[b].add(a)

    for axis in range(3):
        for side in (0, m - 1):
            for u in range(m - 1):
                for w in range(m - 1):
                    def at(du, dw):
                        c = [0, 0, 0]
                        c[axis] = side
                        c[(axis + 1) % 3] = u + du
                        c[(axis + 2) % 3] = w + dw
                        return idx[tuple(c)]
                    a, b, c, d = at(0, 0), at(1, 0), at(1, 1), at(0, 1)
                    for x, y in ((a, b), (b, c), (c, d), (d, a), (a, c)):  # two triangles per grid cell
                        edge(x, y)
    offs = np.zeros(len(pts) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(x) for x in nb])
    return np.array(pts), offs, np.array([v for x in nb for v in sorted(x)], dtype=np.uint32)


def register_adjacency(library, shapes, verts, min_points=33):
    """hull_adjacency for every convex shape of at least `min_points` vertices of a shape table, registered with the
    engine library.  Returns the number of shapes registered."""
    from . import abi
    count = 0
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    for i, s in enumerate(shapes):
        if s["type"] != abi.GEOM_CONVEX or s["num_points"] < min_points:
            continue
        off, n = int(s["vertex_offset"]), int(s["num_points"])
        offs, ids = hull_adjacency(verts[off:off + n])
        library.set_convex_neighbors(i, offs, ids)
        count += 1
    return count


def large_convex(n=50_000, seed=1, sizes=(33, 48, 64, 100, 256), nlib_each=12, half_width=1.0, kind="distance"):
    """Hulls above ConvexBase::num_vertices_large_convex_threshold (32) against each other, small hulls and
    primitives.  Points are random directions scaled onto an ellipsoid, so every point is a hull vertex."""
    rng = _rng(seed, 8)
    lib = geometry.ShapeLibrary()
    for nv in sizes:
        for radii in rng.uniform(0.2, 1.0, (nlib_each, 3)):
            d = rng.normal(size=(nv, 3))
            lib.add_convex(d / np.linalg.norm(d, axis=1, keepdims=True) * radii)
    n_large = len(sizes) * nlib_each
    base = fibonacci_sphere(32)
    for radii in rng.uniform(0.2, 1.0, (nlib_each, 3)):
        lib.add_convex(base * radii)
    for s in rng.uniform(0.2, 1.0, (nlib_each, 3)):
        lib.add_box(*map(float, s))
    for r, lz in zip(rng.uniform(0.1, 0.6, nlib_each), rng.uniform(0.2, 1.0, nlib_each)):
        lib.add_capsule(float(r), float(lz))
    n_all = len(lib)
    s1 = rng.integers(0, n_large, n)                       # always a large hull on one side ...
    s2 = rng.integers(0, n_all, n)
    swap = rng.random(n) < 0.5                             # ... which side is random
    s1, s2 = np.where(swap, s2, s1), np.where(swap, s1, s2)
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    b = Batch("large_convex_" + kind, lib, s1, s2, q1, T1, q2, T2, kind)
    b.n_large = n_large
    return b


def mesh_vs_shapes(n=20_000, seed=1, seg=14, ring=14, n_variants=3, nper=16, half_width=1.2, flats_only=False):
    """BVHModel<OBBRSS> against the convex shape kinds, both operand orders, plus some mesh x mesh and
    shape x shape pairs: the BVH rows / columns of the collision matrix (collision_func_matrix.cpp:471-733)."""
    rng = _rng(seed, 9)
    meshes = mesh_variants(n_variants, seg, ring)
    lib = geometry.ShapeLibrary()
    for k, m in enumerate(meshes):
        lib.add_bvh(k, len(m.vertices))
    for s in rng.uniform(0.2, 0.9, (nper, 3)):
        lib.add_box(*map(float, s))
    for r in rng.uniform(0.1, 0.6, nper):
        lib.add_sphere(float(r))
    for r, lz in zip(rng.uniform(0.1, 0.4, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_capsule(float(r), float(lz))
    for r, lz in zip(rng.uniform(0.1, 0.5, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_cone(float(r), float(lz))
    for r, lz in zip(rng.uniform(0.1, 0.5, nper), rng.uniform(0.2, 1.0, nper)):
        lib.add_cylinder(float(r), float(lz))
    for r in rng.uniform(0.1, 0.7, (nper, 3)):
        lib.add_ellipsoid(*map(float, r))
    base = fibonacci_sphere(24)
    for radii in rng.uniform(0.1, 0.7, (nper, 3)):
        lib.add_convex(base * radii)
    n_solid_end = len(lib)
    for k in range(nper):  # Plane / Halfspace: unbounded BVs, every triangle of the mesh is tested
        nrm, d = rng.normal(size=3), float(rng.uniform(-0.6, 0.6))
        (lib.add_halfspace if k % 2 == 0 else lib.add_plane)(nrm, d)
    n_all = len(lib)
    u = rng.random(n)
    mesh = rng.integers(0, n_variants, n)
    solid = rng.integers(n_solid_end, n_all, n) if flats_only else rng.integers(n_variants, n_solid_end, n)
    s1 = np.where(u < 0.45, mesh, np.where(u < 0.9, solid, np.where(u < 0.95, mesh, solid)))
    s2 = np.where(u < 0.45, solid, np.where(u < 0.9, mesh, np.where(u < 0.95, rng.integers(0, n_variants, n), rng.integers(n_variants, n_solid_end, n))))
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    b = Batch("mesh_vs_shapes_collide", lib, s1, s2, q1, T1, q2, T2, "collide")
    b.meshes = meshes
    return b


SOLID_KINDS = ("box", "sphere", "capsule", "cylinder", "cone", "ellipsoid", "convex32")


def mesh_vs_solid(kind, n=100_000, seed=1, seg=50, nper=64, half_width=1.6):
    """(mesh, solid) collide() / distance() queries, cfg4-size models (seg = ring = 50: 5 000 triangles): SURVEY.md 8(f3),
    the workload of tools/mesh_solid_bench.py (one solid kind) and of bench.py's `cfg4s` line (kind = "mixed": box, sphere,
    capsule, cylinder, ellipsoid, convex32 in equal parts).  The steps per query have a heavy tail (median 1: the boxes at
    the roots are disjoint; mean ~60; maximum in the thousands with hundreds of leaf tests)."""
    rng = _rng(seed, 77)
    meshes = mesh_variants(8, seg, seg)
    lib = geometry.ShapeLibrary()
    for k, m in enumerate(meshes):
        lib.add_bvh(k, len(m.vertices))
    n0 = len(lib)
    kinds = ("box", "sphere", "capsule", "cylinder", "ellipsoid", "convex32") if kind == "mixed" else tuple(kind.split(","))
    for kd in kinds:
        if kd not in SOLID_KINDS:
            raise ValueError(kd)
        for _ in range(nper):
            if kd == "box":
                lib.add_box(*map(float, rng.uniform(0.2, 0.9, 3)))
            elif kd == "sphere":
                lib.add_sphere(float(rng.uniform(0.1, 0.6)))
            elif kd == "capsule":
                lib.add_capsule(float(rng.uniform(0.1, 0.4)), float(rng.uniform(0.2, 1.0)))
            elif kd == "cylinder":
                lib.add_cylinder(float(rng.uniform(0.1, 0.5)), float(rng.uniform(0.2, 1.0)))
            elif kd == "cone":
                lib.add_cone(float(rng.uniform(0.1, 0.5)), float(rng.uniform(0.2, 1.0)))
            elif kd == "ellipsoid":
                lib.add_ellipsoid(*map(float, rng.uniform(0.1, 0.7, 3)))
            else:
                lib.add_convex(fibonacci_sphere(32) * rng.uniform(0.1, 0.7, 3))
    s1 = rng.integers(0, 8, n)
    s2 = rng.integers(n0, n0 + nper * len(kinds), n)
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    b = Batch("mesh_x_" + kind.replace(",", "_"), lib, s1, s2, q1, T1, q2, T2, "collide")
    b.meshes = meshes
    return b


def mixed_scene(n=200_000, seed=1, frac_solid=0.4, frac_mesh_solid=0.4):
    """One batch with every kind of pair a scene of meshes and solids produces -- solid x solid (frac_solid; the six solid kinds of
    mesh_vs_solid("mixed") among themselves), mesh x solid in both operand orders (frac_mesh_solid), mesh x mesh (the rest) -- on cfg4-size
    models: bench.py's `cfgmix` row (what the mesh walks beside the solids' kernels are for; SURVEY.md 8 f3 + configs[3] + configs[4])."""
    b = mesh_vs_solid("mixed", n=n, seed=seed)
    rng = _rng(seed, 91)
    n_lib = len(b.lib)
    u = rng.uniform(size=n)
    mesh_a, mesh_b = rng.integers(0, 8, n), rng.integers(0, 8, n)
    sol_a, sol_b = rng.integers(8, n_lib, n), rng.integers(8, n_lib, n)
    swap = rng.uniform(size=n) < 0.5
    solid = u < frac_solid
    ms = (~solid) & (u < frac_solid + frac_mesh_solid)
    mm = ~(solid | ms)
    s1 = np.where(solid, sol_a, np.where(ms, np.where(swap, sol_a, mesh_a), mesh_a))
    s2 = np.where(solid, sol_b, np.where(ms, np.where(swap, mesh_b, sol_b), mesh_b))
    b.s1, b.s2 = s1.astype(b.s1.dtype), s2.astype(b.s2.dtype)
    b.name = "mixed_scene_collide"
    b.mix = {"solid_x_solid": float(solid.mean()), "mesh_x_solid": float(ms.mean()), "mesh_x_mesh": float(mm.mean())}
    return b


def cfg5_mixed(n=100_000, seed=1, nper=256, half_width=0.8):
    """cfg5-style mixed primitive+convex pairs (type mix 20 % each of Box/Sphere/Capsule/
    Ellipsoid/Convex32), synthetic pair list (cfg5_broadphase_scene takes its pairs from the host broadphase)."""
    rng = _rng(seed, 5)
    lib = _mixed_library(rng, nper)
    s1, s2 = rng.integers(0, 5 * nper, n), rng.integers(0, 5 * nper, n)
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    return Batch("cfg5_mixed_collide", lib, s1, s2, q1, T1, q2, T2, "collide")


def cfg5_broadphase_scene(n_objects=100_000, target_pairs=1_000_000, seed=1, nper=256, n_threads=0):
    """cfg5: a scene of posed {Box, Sphere, Capsule, Ellipsoid, Convex32} objects (20 % each); the
    pair list comes from the host broadphase (engine.world_aabbs -> engine.broadphase_self_pairs,
    i.e. what DynamicAABBTreeCollisionManager::collide + CollisionCallBackCollect would collect).
    The cube side is chosen so that about `target_pairs` AABB pairs overlap."""
    from . import engine
    rng = _rng(seed, 55)
    lib = _mixed_library(rng, nper)
    obj_shape = rng.integers(0, 5 * nper, n_objects).astype(np.uint32)
    quat = uniform_quaternions(rng, n_objects)
    # expected pairs ~ n^2/2 * E[prod_k (w_ik + w_jk)/2 * 2] / L^3; the constant is measured on this library
    side = (n_objects ** 2 * 30.5 / (2.0 * max(target_pairs, 1))) ** (1.0 / 3.0)
    T = rng.uniform(-side / 2, side / 2, (n_objects, 3))
    tf = geometry.make_pose(quat=quat, T=T)
    aabbs = engine.world_aabbs(lib, obj_shape, tf, n_threads)
    pairs = engine.broadphase_self_pairs(aabbs, n_threads)
    i, j = pairs[:, 0], pairs[:, 1]
    b = Batch("cfg5_broadphase_mixed_collide", lib, obj_shape[i], obj_shape[j], quat[i], T[i], quat[j], T[j], "collide")
    b.scene = dict(n_objects=n_objects, side=side, aabbs=aabbs, pairs=pairs, obj_shape=obj_shape, obj_tf=tf)
    return b


class PlannerScene:
    """scene_planner's product: lib, obj_shape (G,), pairs (P, 2), quat (n_conf, G, 4), T (n_conf, G, 3)."""

    def __init__(self, lib, obj_shape, pairs, quat, T):
        self.lib, self.obj_shape, self.pairs, self.quat, self.T = lib, obj_shape, pairs, quat, T
        self.shapes, self.verts = lib.shapes_array(), lib.vertices_array()
        self.kind, self.request_overrides, self.meshes = "collide", {}, None
        self.name = "scene_planner_%dx%d" % (len(quat), len(obj_shape))

    @property
    def obj_tf(self):
        """(n_conf, G, 12) Transform3f images"""
        n_conf, G = self.quat.shape[:2]
        return geometry.make_pose(quat=self.quat.reshape(-1, 4), T=self.T.reshape(-1, 3)).reshape(n_conf, G, 12)

    @property
    def obj_pose_f32(self):
        n_conf, G = self.quat.shape[:2]
        return geometry.pose_f32_from_quat(self.quat.reshape(-1, 4), self.T.reshape(-1, 3)).reshape(n_conf, G, 7)

    def expand(self):
        """The per-pair Batch a caller without scenes builds on the host: query c * P + p = pair p of configuration c."""
        i, j = self.pairs[:, 0], self.pairs[:, 1]
        f = lambda a, k: a[:, k].reshape(-1, a.shape[-1])  # noqa: E731
        n_conf = len(self.quat)
        return Batch(self.name, self.lib, np.tile(self.obj_shape[i], n_conf), np.tile(self.obj_shape[j], n_conf), f(self.quat, i), f(self.T, i),
                     f(self.quat, j), f(self.T, j), "collide")


def scene_planner(n_conf=2048, n_objects=16, seed=1, nper=64, link=1.6, bend=0.8):
    """What a sampling-based planner asks: n_conf configurations of a chain of n_objects bodies (the cfg5 shape mix), and the
    fixed list of all G (G - 1) / 2 body pairs minus the chain's neighbours.  A configuration is a bent chain: body k sits
    `link` away from body k - 1 in the direction e_x + bend * N(0, I), normalised, with a uniformly random orientation.
    The defaults (bodies reach 0.1 .. 1.8 from their centres) leave a minority of the configurations in collision: 38 % of
    256 configurations of 16 bodies, 14 % with 8 bodies (oracle, seed 1; tests/test_scene_cpu.py prints and holds the share)."""
    rng = _rng(seed, 77)
    lib = _mixed_library(rng, nper)
    obj_shape = rng.integers(0, 5 * nper, n_objects).astype(np.uint32)
    quat = uniform_quaternions(rng, n_conf * n_objects).reshape(n_conf, n_objects, 4)
    step = bend * rng.normal(size=(n_conf, n_objects, 3))
    step[..., 0] += 1.0
    step *= link / np.linalg.norm(step, axis=-1, keepdims=True)
    step[:, 0] = 0.0
    T = np.cumsum(step, axis=1)
    i, j = np.triu_indices(n_objects, 2)  # j - i >= 2
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    return PlannerScene(lib, obj_shape, pairs, quat, T)


def scene_robot_env(n_conf, n_links, n_obstacles, seed=1, nper=64, link=1.6, bend=0.8, spread=1.0, split=False, spatial=False, full=True):
    """A robot in a static environment, for the device-made pair lists with object groups (engine.Scene.set_groups): scene_planner's
    bent chain of n_links <= 63 bodies per configuration, then n_obstacles bodies of the same shape mix whose pose is the same in
    every configuration, scattered uniformly through the box the chains sweep over all configurations -- their centres' box grown by
    the bodies' reach, 1.8, and scaled about its centre by `spread`.  Object order: links first.  Returns (scene, groups, pairs):
      scene   a PlannerScene (lib, obj_shape, quat, T; obj_tf / obj_pose_f32 are the pose tables) whose pair list is `pairs`;
      groups  (object_group uint8, collides uint64[n_links + 1]): link k is group k, every obstacle group n_links; allowed are
              link-link but the chain's neighbours and link-obstacle, not obstacle-obstacle;
      pairs   the equivalent explicit list: the allowed pairs (i < j) in lexicographic order, uint32 (P, 2).
    spatial: the obstacles in engine.spatial_order of their centres (the same obstacles, permuted), which is what the tile boxes of a
    scene with an environment (engine.Scene.set_environment) need.  split: two more items, for the calls that take the moving objects'
    poses alone -- (moving table (n_conf, n_links, 12), environment poses (n_obstacles, 12)) and the same as 7-float poses.
    full=False (with split): the returned scene holds configuration 0 alone -- a table of n_conf x n_objects rows is what the split
    forms exist to avoid (4 096 configurations of 65 536 obstacles: 25.8 GB)."""
    if not 1 <= n_links <= 63:
        raise ValueError("scene_robot_env: 1 to 63 links (a group each, one more for the obstacles)")
    chain = scene_planner(n_conf, n_links, seed, nper, link, bend)
    rng = _rng(seed, 78)
    n = n_links + n_obstacles
    obj_shape = np.concatenate([chain.obj_shape, rng.integers(0, 5 * nper, n_obstacles).astype(np.uint32)])
    lo, hi = chain.T.reshape(-1, 3).min(axis=0), chain.T.reshape(-1, 3).max(axis=0)
    mid, half = (lo + hi) / 2, ((hi - lo) / 2 + 1.8) * spread
    T_obs = rng.uniform(mid - half, mid + half, (n_obstacles, 3))
    q_obs = uniform_quaternions(rng, n_obstacles)
    if spatial:
        from . import engine
        order = engine.spatial_order(T_obs)
        T_obs, q_obs = T_obs[order], q_obs[order]
        obj_shape[n_links:] = obj_shape[n_links:][order]
    n_full = n_conf if full or not split else 1
    quat = np.concatenate([chain.quat[:n_full], np.broadcast_to(q_obs, (n_full, n_obstacles, 4))], axis=1)
    T = np.concatenate([chain.T[:n_full], np.broadcast_to(T_obs, (n_full, n_obstacles, 3))], axis=1)
    object_group = np.minimum(np.arange(n), n_links).astype(np.uint8)
    m = np.ones((n_links + 1, n_links + 1), dtype=bool)
    k = np.arange(n_links)
    m[k, k] = False
    m[k[:-1], k[1:]] = m[k[1:], k[:-1]] = False
    m[n_links, n_links] = False
    collides = np.array([(np.uint64(1) << np.flatnonzero(row).astype(np.uint64)).sum(dtype=np.uint64) for row in m], dtype=np.uint64)
    li, lj = np.triu_indices(n_links, 2)
    rows = [np.stack([li, lj], axis=1)] + [np.stack([np.full(n_obstacles, i), np.arange(n_links, n)], axis=1) for i in range(n_links)]
    pairs = np.concatenate(rows).astype(np.int64)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))].astype(np.uint32)
    scene = PlannerScene(chain.lib, obj_shape, np.ascontiguousarray(pairs), np.ascontiguousarray(quat), np.ascontiguousarray(T))
    scene.name = "scene_robot_env_%dx%d+%d" % (n_conf, n_links, n_obstacles)
    if split:
        env_tf, env_pose = scene.obj_tf[0, n_links:], scene.obj_pose_f32[0, n_links:]
        moving_tf = geometry.make_pose(quat=chain.quat.reshape(-1, 4), T=chain.T.reshape(-1, 3)).reshape(n_conf, n_links, 12)
        moving_pose = geometry.pose_f32_from_quat(chain.quat.reshape(-1, 4), chain.T.reshape(-1, 3)).reshape(n_conf, n_links, 7)
        return (scene, (object_group, collides), scene.pairs, (np.ascontiguousarray(moving_tf), np.ascontiguousarray(env_tf)),
                (np.ascontiguousarray(moving_pose), np.ascontiguousarray(env_pose)))
    return scene, (object_group, collides), scene.pairs


_MESH_CACHE = {}


def mesh_variants(n_variants=8, seg=50, ring=50):
    """cfg4 mesh library: perturbed UV spheres (seg=ring=50 -> 5000 triangles, 2502 vertices, 9999 nodes)."""
    from . import bvh_builder
    key = (n_variants, seg, ring)
    if key not in _MESH_CACHE:
        _MESH_CACHE[key] = [bvh_builder.Mesh(*bvh_builder.bumpy_sphere(seg, ring, r=1.0, amp=0.12 + 0.01 * k,
                                                                       freq=2 + (k % 3), phase=0.7 * k))
                            for k in range(n_variants)]
    return _MESH_CACHE[key]


def cfg4_mesh_mesh(n=100_000, seed=1, n_variants=8, seg=50, ring=50, half_width=1.25):
    """cfg4: BVHModel<OBBRSS> x BVHModel<OBBRSS> collide(), default request (first contact)."""
    rng = _rng(seed, 4)
    meshes = mesh_variants(n_variants, seg, ring)
    lib = geometry.ShapeLibrary()
    for k, m in enumerate(meshes):
        lib.add_bvh(k, len(m.vertices))
    s1, s2 = rng.integers(0, n_variants, n), rng.integers(0, n_variants, n)
    q1, T1, q2, T2 = _poses(rng, n, half_width)
    b = Batch("cfg4_mesh_mesh_collide_%dtri" % (2 * seg * ring), lib, s1, s2, q1, T1, q2, T2, "collide")
    b.meshes = meshes
    return b


def cfg4_mesh_mesh_distance(n=100_000, seed=1, n_variants=8, seg=50, ring=50, half_width=2.2):
    """cfg4's distance() variant ("100 000 mesh-mesh collide() (and distance())"): the same models, poses
    spread so that about two thirds of the pairs are separated (a distance() on intersecting meshes ends at the first
    overlapping triangle pair)."""
    b = cfg4_mesh_mesh(n=n, seed=seed, n_variants=n_variants, seg=seg, ring=ring, half_width=half_width)
    b.kind = "distance"
    b.name = "cfg4_mesh_mesh_distance_%dtri" % (2 * seg * ring)
    return b


class HfieldTerrain:
    """A height field and queries of solids against it (hfield_terrain): the field (x_dim, y_dim, heights (ny, nx), min_height), the
    solids' ShapeLibrary, per query the solid's id, the two poses and the operand order."""

    def __init__(self, x_dim, y_dim, heights, min_height, lib, shape, tf_hfield, tf_shape, swapped):
        self.x_dim, self.y_dim, self.heights, self.min_height, self.lib = x_dim, y_dim, heights, min_height, lib
        self.shape, self.tf_hfield, self.tf_shape, self.swapped = shape, tf_hfield, tf_shape, swapped
        self.hfield = np.zeros(len(shape), dtype=np.uint32)

    def __len__(self):
        return len(self.shape)

    def triangulation(self):
        """(vertices, triangles) of the field's top surface, the two triangles of a cell cut along the prisms' diagonal: what a caller
        without height fields hands to BVHModel<OBBRSS>.  A surface, not the solid down to min_height: it answers another question."""
        ny, nx = self.heights.shape
        xg = np.linspace(-0.5 * self.x_dim, 0.5 * self.x_dim, nx)
        yg = np.linspace(0.5 * self.y_dim, -0.5 * self.y_dim, ny)
        X, Y = np.meshgrid(xg, yg)
        verts = np.stack([X.ravel(), Y.ravel(), np.maximum(self.heights, self.min_height).ravel()], axis=1)
        r, c = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
        v00, v01, v10, v11 = (r * nx + c).ravel(), (r * nx + c + 1).ravel(), ((r + 1) * nx + c).ravel(), ((r + 1) * nx + c + 1).ravel()
        tris = np.concatenate([np.stack([v00, v10, v01], axis=1), np.stack([v10, v11, v01], axis=1)]).astype(np.uint32)
        return verts, tris


def hfield_terrain(n_queries=100_000, nx=256, ny=256, seed=1, cell=0.25, nper=16):
    """A smooth random terrain of nx x ny samples, `cell` apart (a sum of a few sine products, heights around 1.3 +- 0.6 over
    min_height = 0), and n_queries solids of the seven kinds a height field collides with, 0.2 to 0.6 across, resting near the
    surface under random rotations: about half of them in contact.  Both operand orders; the field at the identity."""
    rng = _rng(seed, 131)
    x_dim, y_dim = cell * (nx - 1), cell * (ny - 1)
    xg = np.linspace(-0.5 * x_dim, 0.5 * x_dim, nx)
    yg = np.linspace(0.5 * y_dim, -0.5 * y_dim, ny)
    X, Y = np.meshgrid(xg, yg)
    h = np.full((ny, nx), 1.3)
    for _ in range(6):
        lx, ly = rng.uniform(3.0, 12.0, 2)
        h += rng.uniform(0.08, 0.22) * np.sin(2 * np.pi * X / lx + rng.uniform(0, 6.3)) * np.sin(2 * np.pi * Y / ly + rng.uniform(0, 6.3))
    lib = geometry.ShapeLibrary()
    reach = []  # a radius that bounds the solid
    for _ in range(nper):
        s = rng.uniform(0.2, 0.6, 3)
        lib.add_box(*map(float, s))
        reach.append(0.5 * float(np.linalg.norm(s)))
    for r in rng.uniform(0.1, 0.3, nper):
        lib.add_sphere(float(r))
        reach.append(float(r))
    for r, lz in zip(rng.uniform(0.08, 0.2, nper), rng.uniform(0.1, 0.4, nper)):
        lib.add_capsule(float(r), float(lz))
        reach.append(float(r + lz / 2))
    for r, lz in zip(rng.uniform(0.1, 0.3, nper), rng.uniform(0.2, 0.6, nper)):
        lib.add_cone(float(r), float(lz))
        reach.append(float(np.hypot(r, lz / 2)))
    for r, lz in zip(rng.uniform(0.1, 0.3, nper), rng.uniform(0.2, 0.6, nper)):
        lib.add_cylinder(float(r), float(lz))
        reach.append(float(np.hypot(r, lz / 2)))
    for r in rng.uniform(0.1, 0.3, (nper, 3)):
        lib.add_ellipsoid(*map(float, r))
        reach.append(float(r.max()))
    base = fibonacci_sphere(24)
    for r in rng.uniform(0.1, 0.3, (nper, 3)):
        lib.add_convex(base * r)
        reach.append(float(r.max()))
    reach = np.array(reach)
    shape = rng.integers(0, len(lib), n_queries).astype(np.uint32)
    u, v = rng.uniform(0.01, 0.99, n_queries), rng.uniform(0.01, 0.99, n_queries)
    ci, ri = np.minimum((u * (nx - 1)).astype(int), nx - 2), np.minimum((v * (ny - 1)).astype(int), ny - 2)
    ground = np.maximum.reduce([h[ri, ci], h[ri + 1, ci], h[ri, ci + 1], h[ri + 1, ci + 1]])
    T = np.stack([(u - 0.5) * x_dim, (0.5 - v) * y_dim, ground + reach[shape] * rng.uniform(0.0, 1.2, n_queries)], axis=1)
    tf_shape = geometry.make_pose(quat=uniform_quaternions(rng, n_queries), T=T)
    tf_hfield = np.repeat(geometry.make_pose().reshape(1, 12), n_queries, axis=0)
    swapped = (rng.random(n_queries) < 0.5).astype(np.uint8)
    return HfieldTerrain(x_dim, y_dim, h, 0.0, lib, shape, tf_hfield, tf_shape, swapped)


class SceneRobotTerrain:
    """Chains of solids over a terrain (scene_robot_terrain): the terrain (an HfieldTerrain: field and ShapeLibrary), its pose (12
    doubles), the shape of every link and the pose table (n_conf, n_links, 12)."""

    def __init__(self, terrain, tf_terrain, object_shape, moving_tf):
        self.terrain, self.tf_terrain, self.object_shape, self.moving_tf = terrain, tf_terrain, object_shape, moving_tf

    def explicit(self):
        """the same queries as the per-query arrays of Library.hfield_collide: (hfield, shape, tf_hfield, tf_shape), query c * n_links + k"""
        n_conf, n_links = self.moving_tf.shape[:2]
        n = n_conf * n_links
        return (np.zeros(n, dtype=np.uint32), np.tile(self.object_shape, n_conf), np.repeat(self.tf_terrain.reshape(1, 12), n, axis=0),
                np.ascontiguousarray(self.moving_tf.reshape(n, 12)))


def scene_robot_terrain(n_conf=4096, n_links=24, side=256, seed=1, spacing=0.3):
    """n_conf configurations of a chain of n_links solids (the kinds and sizes of hfield_terrain, `spacing` apart along a random heading)
    laid over hfield_terrain's surface of side x side samples: every link sits above the ground under it by the configuration's own
    clearance (0 to 0.5) plus a little of its own, under a random rotation, so that a share of the configurations touch the ground with
    some of their links and the others clear it.  The terrain at the identity."""
    t = hfield_terrain(n_queries=1, nx=side, ny=side, seed=seed)
    rng = _rng(seed, 137)
    ny, nx = t.heights.shape
    object_shape = rng.integers(0, len(t.lib), n_links).astype(np.uint32)
    heading = rng.uniform(0.0, 2 * np.pi, n_conf)
    base = np.stack([rng.uniform(-0.4, 0.4, n_conf) * t.x_dim, rng.uniform(-0.4, 0.4, n_conf) * t.y_dim], axis=1)
    along = (np.arange(n_links) - 0.5 * (n_links - 1)) * spacing
    x = base[:, :1] + np.cos(heading)[:, None] * along[None, :]
    y = base[:, 1:] + np.sin(heading)[:, None] * along[None, :]
    u = np.clip(x / t.x_dim + 0.5, 0.01, 0.99)
    v = np.clip(0.5 - y / t.y_dim, 0.01, 0.99)
    ci, ri = np.minimum((u * (nx - 1)).astype(int), nx - 2), np.minimum((v * (ny - 1)).astype(int), ny - 2)
    h = t.heights
    ground = np.maximum.reduce([h[ri, ci], h[ri + 1, ci], h[ri, ci + 1], h[ri + 1, ci + 1]])
    z = ground + rng.uniform(0.0, 0.5, (n_conf, 1)) + rng.uniform(0.05, 0.2, (n_conf, n_links))
    T = np.stack([(u - 0.5) * t.x_dim, (0.5 - v) * t.y_dim, z], axis=2).reshape(-1, 3)
    moving_tf = geometry.make_pose(quat=uniform_quaternions(rng, n_conf * n_links), T=T).reshape(n_conf, n_links, 12)
    return SceneRobotTerrain(t, geometry.make_pose().reshape(12), object_shape, np.ascontiguousarray(moving_tf))


def make_library(pkg, batch, device=0, options=None):
    """engine.Library for a batch (registers the batch's meshes, if any); options: {key: value} for hfcl_lib_set_option."""
    lib = pkg.Library(batch.lib, device=device, options=options)
    for m in getattr(batch, "meshes", []) or []:
        lib.add_bvh(m)
    return lib


def make_request(batch, abi, **kw):
    req = abi.default_distance_request() if batch.kind == "distance" else abi.default_collision_request()
    over = dict(batch.request_overrides)
    over.update(kw)
    for k, v in over.items():
        if hasattr(req, k):
            setattr(req, k, v)
        else:
            setattr(req.q, k, v)
    return req


# ---- resting contacts (contact patches) ------------------------------------------------------------------------------------
def _rot_axis_angle(axis, ang):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _rot_from_to(u, v):
    """A rotation taking unit vector u onto unit vector v."""
    u, v = np.asarray(u, float) / np.linalg.norm(u), np.asarray(v, float) / np.linalg.norm(v)
    c = float(u @ v)
    w = np.cross(u, v)
    if np.linalg.norm(w) < 1e-12:
        if c > 0:
            return np.eye(3)
        p = np.cross(u, [1.0, 0, 0]) if abs(u[0]) < 0.9 else np.cross(u, [0, 1.0, 0])
        return _rot_axis_angle(p, np.pi)
    return _rot_axis_angle(w, np.arctan2(np.linalg.norm(w), c))


def _local_support(s, verts, d):
    """Support point of a library shape in its own frame along d (swept-sphere radius included)."""
    from . import abi
    k, p = int(s["type"]), s["params"]
    dn = d / np.linalg.norm(d)
    if k == abi.GEOM_BOX:
        r = np.sign(d) * p[:3]
    elif k == abi.GEOM_SPHERE:
        r = p[0] * dn
    elif k == abi.GEOM_ELLIPSOID:
        v = p[:3] ** 2 * d
        r = v / np.sqrt(v @ d)
    elif k == abi.GEOM_CAPSULE:
        r = np.array([0, 0, np.sign(d[2]) * p[1]]) + p[0] * dn
    elif k in (abi.GEOM_CONE, abi.GEOM_CYLINDER):
        rad, h = p[0], p[1]
        xy = np.hypot(d[0], d[1])
        rim = np.array([0.0, 0.0]) if xy < 1e-15 else rad * d[:2] / xy
        if k == abi.GEOM_CYLINDER:
            r = np.array([rim[0], rim[1], np.sign(d[2]) * h])
        else:
            tip, base = np.array([0, 0, h]), np.array([rim[0], rim[1], -h])
            r = tip if tip @ d >= base @ d else base
    elif k in (abi.GEOM_CONVEX, abi.GEOM_TRIANGLE):
        o, n = int(s["vertex_offset"]), int(s["num_points"]) if k == abi.GEOM_CONVEX else 3
        V = verts[o:o + n]
        r = V[int(np.argmax(V @ d))]
    else:
        raise ValueError(k)
    return r + float(s["swept_sphere_radius"]) * dn


def _face_normals(s, verts, rng):
    """Local outward normals of flat faces of a shape (for face-on-face placements); None: any direction."""
    from . import abi
    k = int(s["type"])
    if k == abi.GEOM_BOX:
        return np.concatenate([np.eye(3), -np.eye(3)])
    if k == abi.GEOM_CYLINDER:
        return np.array([[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0]])
    if k == abi.GEOM_CONE:
        return np.array([[0, 0, -1.0], [1.0, 0, 0]])
    if k == abi.GEOM_CAPSULE:
        return np.array([[1.0, 0, 0], [0, 1.0, 0]])
    if k == abi.GEOM_CONVEX:
        from scipy.spatial import ConvexHull
        o, n = int(s["vertex_offset"]), int(s["num_points"])
        eq = ConvexHull(verts[o:o + n]).equations[:, :3]
        return eq[rng.permutation(len(eq))[:8]]
    if k == abi.GEOM_TRIANGLE:
        o = int(s["vertex_offset"])
        a, b, c = verts[o:o + 3]
        nrm = np.cross(b - a, c - a)
        nrm /= np.linalg.norm(nrm)
        return np.array([nrm, -nrm])
    return None


def resting_library(seed=1, nper=8):
    """Every primitive kind (box, sphere, capsule, cone, cylinder, ellipsoid, triangle, plane, halfspace), 32- and 64-vertex
    hulls (random, and prisms with large coplanar faces).  Returns (ShapeLibrary, ids of 64-vertex hulls)."""
    rng = _rng(seed, 21)
    lib = geometry.ShapeLibrary()
    for s in rng.uniform(0.2, 0.8, (nper, 3)):
        lib.add_box(*map(float, s))
    for r in rng.uniform(0.2, 0.6, nper):
        lib.add_sphere(float(r))
    for r, lz in zip(rng.uniform(0.1, 0.4, nper), rng.uniform(0.2, 0.8, nper)):
        lib.add_capsule(float(r), float(lz))
    for r, lz in zip(rng.uniform(0.2, 0.6, nper), rng.uniform(0.2, 0.8, nper)):
        lib.add_cone(float(r), float(lz))
    for r, lz in zip(rng.uniform(0.2, 0.6, nper), rng.uniform(0.2, 0.8, nper)):
        lib.add_cylinder(float(r), float(lz))
    for r in rng.uniform(0.2, 0.6, (nper, 3)):
        lib.add_ellipsoid(*map(float, r))
    for _ in range(nper):
        t = rng.uniform(-0.6, 0.6, (3, 3))
        lib.add_triangle(t[0], t[1], t[2])
    large = []
    for nv in (32, 64):
        for radii in rng.uniform(0.3, 0.8, (nper // 2, 3)):
            d = rng.normal(size=(nv, 3))
            i = lib.add_convex(d / np.linalg.norm(d, axis=1, keepdims=True) * radii)
            if nv > 32:
                large.append(len(lib) - 1)
        for r, h in zip(rng.uniform(0.3, 0.7, nper // 2), rng.uniform(0.2, 0.6, nper // 2)):
            m = nv // 2
            a = 2 * np.pi * np.arange(m) / m
            ring = np.stack([r * np.cos(a), r * np.sin(a)], axis=1)
            lib.add_convex(np.concatenate([np.c_[ring, np.full(m, h)], np.c_[ring, np.full(m, -h)]]))
            if nv > 32:
                large.append(len(lib) - 1)
    for _ in range(nper // 2):
        nrm = rng.normal(size=3)
        lib.add_halfspace(nrm, float(rng.uniform(-0.3, 0.3)))
        lib.add_plane(rng.normal(size=3), float(rng.uniform(-0.3, 0.3)))
    return lib, large


def resting_contacts(n=20_000, seed=1, nper=8, tilt=3e-3, mesh_frac=0.0):
    """Shape 2 resting on shape 1 along a face normal of shape 1 (random yaw, penetration 1e-4 .. 1e-2, tilts of the order
    of patch_tolerance so that support sets gain and lose points), both operand orders.  Random poses almost never give
    face contacts; these do.  The batch's `large` lists the hulls of more than 32 vertices (register_adjacency).
    mesh_frac > 0: that fraction of the pairs are BVHModel<OBBRSS> rows instead -- mesh x solid, solid x mesh and mesh x mesh,
    a small bumpy sphere (radius ~1) against a shape or another mesh placed near its surface (their patches are points; the
    batch's `meshes` go to make_library)."""
    from . import abi
    rng = _rng(seed, 22)
    lib, large = resting_library(seed, nper)
    shapes, verts = lib.shapes_array(), lib.vertices_array()
    flat = np.isin(shapes["type"], [abi.GEOM_PLANE, abi.GEOM_HALFSPACE])
    solid_ids = np.flatnonzero(~flat)
    all_ids = np.arange(len(shapes))
    s1 = rng.choice(all_ids, n)
    s2 = rng.choice(solid_ids, n)
    R1s, T1s, R2s, T2s = np.empty((n, 3, 3)), np.empty((n, 3)), np.empty((n, 3, 3)), np.empty((n, 3))
    for i in range(n):
        a, b = shapes[s1[i]], shapes[s2[i]]
        R1 = geometry.quat_to_matrix(uniform_quaternions(rng, 1))[0]
        T1 = rng.uniform(-0.5, 0.5, 3)
        if flat[s1[i]]:
            nl = np.asarray(a["params"][:3], dtype=np.float64)
            up_l = nl
            h1 = float(a["params"][3]) + float(a["swept_sphere_radius"])
        else:
            fn = _face_normals(a, verts, rng)
            up_l = fn[rng.integers(len(fn))] if fn is not None else rng.normal(size=3)
            up_l = up_l / np.linalg.norm(up_l)
            h1 = float(_local_support(a, verts, up_l) @ up_l)
        up = R1 @ up_l
        fn2 = _face_normals(b, verts, rng)
        down_l = fn2[rng.integers(len(fn2))] if fn2 is not None else rng.normal(size=3)
        down_l = down_l / np.linalg.norm(down_l)
        R2 = _rot_axis_angle(up, rng.uniform(0, 2 * np.pi)) @ _rot_from_to(down_l, -up)
        R2 = _rot_axis_angle(np.cross(up, rng.normal(size=3)), rng.uniform(0, tilt)) @ R2
        h2 = float(_local_support(b, verts, R2.T @ -up) @ (R2.T @ -up))
        depth = 10 ** rng.uniform(-4, -2)
        lateral = rng.normal(size=3) * 0.05
        lateral -= (lateral @ up) * up
        T2 = T1 + (h1 - depth + h2) * up + lateral
        R1s[i], T1s[i], R2s[i], T2s[i] = R1, T1, R2, T2
    swap = rng.random(n) < 0.5
    s1o, s2o = np.where(swap, s2, s1), np.where(swap, s1, s2)
    R1o, R2o = np.where(swap[:, None, None], R2s, R1s), np.where(swap[:, None, None], R1s, R2s)
    T1o, T2o = np.where(swap[:, None], T2s, T1s), np.where(swap[:, None], T1s, T2s)
    meshes = None
    m = int(round(n * mesh_frac))
    if m > 0:
        meshes = mesh_variants(2, seg=14, ring=14)
        bvh_ids = [lib.add_bvh(k, len(mm.vertices)) for k, mm in enumerate(meshes)]
        u = rng.random(m)
        mesh_a = rng.choice(bvh_ids, m)
        mesh_b = rng.choice(bvh_ids, m)
        # (TriangleP has no collide() function against a BVHModel: collision_func_matrix.cpp)
        solid = rng.choice(solid_ids[shapes["type"][solid_ids] != abi.GEOM_TRIANGLE], m)
        first = np.where(u < 0.4, mesh_a, np.where(u < 0.8, solid, mesh_a))
        second = np.where(u < 0.4, solid, np.where(u < 0.8, mesh_a, mesh_b))
        d = rng.normal(size=(m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        gap = np.where(u < 0.8, rng.uniform(0.9, 1.3, m), rng.uniform(1.7, 2.1, m))  # near the ~1-radius surface
        Ta = rng.uniform(-0.5, 0.5, (m, 3))
        s1o[:m], s2o[:m] = first, second
        R1o[:m] = geometry.quat_to_matrix(uniform_quaternions(rng, m))
        R2o[:m] = geometry.quat_to_matrix(uniform_quaternions(rng, m))
        T1o[:m], T2o[:m] = Ta, Ta + gap[:, None] * d
    b = RestingBatch(lib, s1o, s2o, geometry.make_pose(R=R1o, T=T1o), geometry.make_pose(R=R2o, T=T2o), large)
    b.meshes = meshes
    return b


class RestingBatch:
    """collide() pairs with Transform3f poses (no quaternions): resting_contacts."""

    def __init__(self, lib, s1, s2, tf1, tf2, large):
        self.name, self.kind, self.lib = "resting_contacts", "collide", lib
        self.shapes, self.verts = lib.shapes_array(), lib.vertices_array()
        self.s1, self.s2 = np.ascontiguousarray(s1, dtype=np.uint32), np.ascontiguousarray(s2, dtype=np.uint32)
        self.tf1, self.tf2 = np.ascontiguousarray(tf1), np.ascontiguousarray(tf2)
        self.large = large
        self.meshes = None
        self.request_overrides = {}

    def __len__(self):
        return len(self.s1)

    def graphs(self):
        """{shape id: (offsets, ids)} of the hulls of more than 32 vertices (what register_adjacency registers)."""
        out = {}
        for i in self.large:
            s = self.shapes[i]
            o, k = int(s["vertex_offset"]), int(s["num_points"])
            out[i] = hull_adjacency(self.verts[o:o + k])
        return out
