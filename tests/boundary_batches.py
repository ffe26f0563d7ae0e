"""The batches of the mesh collide() tests whose checkers excuse the records of a decision band (compare.boundary_band): one constructor per
batch, shared by the GPU test that runs it and by tests/test_bvh_boundary_cpu.py, which recomputes the band's population from the oracle alone.

CASES: name -> Case(make, margin, kind, allowed).  make(pkg) -> (batch, request); margin: the request's security_margin, the boundary of the
decision; kind: "mm" -- oracle.bvh_collide_batch -- or "mixed" -- oracle.mixed_collide_batch --; allowed: the oracle records within 1e-9 of the
boundary.  It is 0 for every batch here (the nearest record of any of them is 5.2e-8 away, scene-1-0.0), so no record of theirs is excused."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "make margin kind allowed")


def mesh_batch(pkg, meshes, n, seed, half_width):
    """n mesh x mesh pairs drawn from `meshes`."""
    wl, g = pkg.workloads, pkg.geometry
    rng = np.random.default_rng(seed)
    lib = g.ShapeLibrary()
    for k, m in enumerate(meshes):
        lib.add_bvh(k, len(m.vertices))
    s1, s2 = rng.integers(0, len(meshes), n), rng.integers(0, len(meshes), n)
    q1, T1, q2, T2 = wl._poses(rng, n, half_width)
    b = wl.Batch("mesh_pairs", lib, s1, s2, q1, T1, q2, T2, "collide")
    b.meshes = meshes
    return b


def _cfg4(request=None, **kw):
    def make(pkg):
        b = pkg.workloads.cfg4_mesh_mesh(**kw)
        return b, pkg.workloads.make_request(b, pkg.abi, **(request or {}))
    return make


def wide_meshes(pkg):
    """A BVHModel of 72 200 triangles (144 399 nodes) and a small one."""
    bb = pkg.bvh_builder
    return [bb.Mesh(*bb.bumpy_sphere(190, 190, r=1.0, amp=0.1, freq=3, phase=0.3)), bb.Mesh(*bb.bumpy_sphere(20, 20, r=0.7, amp=0.1, freq=2, phase=0.1))]


def _wide(pkg):
    b = mesh_batch(pkg, wide_meshes(pkg), 600, 3, 1.1)
    return b, pkg.workloads.make_request(b, pkg.abi)


def _wide_solids(pkg):
    """The 72 200-triangle model against boxes and capsules."""
    g, wl = pkg.geometry, pkg.workloads
    big = wide_meshes(pkg)[0]
    rng = np.random.default_rng(5)
    L = g.ShapeLibrary()
    L.add_bvh(0, len(big.vertices))
    for _ in range(8):
        L.add_box(*map(float, rng.uniform(0.2, 0.8, 3)))
        L.add_capsule(float(rng.uniform(0.1, 0.3)), float(rng.uniform(0.2, 0.8)))
    n = 1500
    q1, T1, q2, T2 = wl._poses(rng, n, 1.4)
    bs = wl.Batch("big_mesh_x_solid", L, np.zeros(n, dtype=np.int64), rng.integers(1, 17, n), q1, T1, q2, T2, "collide")
    bs.meshes = [big]
    return bs, pkg.abi.default_collision_request()


def deep_mesh(pkg):
    """A strip of triangles whose positions grow geometrically: a tree of more than 100 levels."""
    nt, r = 1200, 3.2
    x = r ** (np.arange(nt // 2 + 2) - float(nt // 2 + 1))  # largest coordinate 1
    v = np.zeros((2 * (nt // 2 + 2), 3))
    k = np.arange(len(v) // 2)
    v[0::2] = np.stack([x[k], 0 * x[k], 0.02 * x[k]], 1)
    v[1::2] = np.stack([x[k], 0.3 * x[k], -0.02 * x[k]], 1)
    t = np.array([[i, i + 1, i + 2] for i in range(nt)], dtype=np.uint32)
    return pkg.bvh_builder.Mesh(v, t)


def _deep(pkg):
    b = mesh_batch(pkg, [deep_mesh(pkg)], 256, 4, 0.05)
    return b, pkg.workloads.make_request(b, pkg.abi)


def _scene(nmax, margin, **kw):
    def make(pkg):
        b = pkg.workloads.mesh_vs_shapes(**kw)
        req = pkg.abi.default_collision_request()
        req.num_max_contacts, req.security_margin = nmax, margin
        return b, req
    return make


def _solid(kind, n, seed, margin=0.0, cached=False, own_request=False):
    def make(pkg):
        abi = pkg.abi
        b = pkg.workloads.mesh_vs_solid(kind, n=n, seed=seed)
        req = pkg.workloads.make_request(b, abi) if own_request else abi.default_collision_request()
        if margin:
            req.security_margin = margin
        if cached:
            req.q.gjk_initial_guess = abi.CachedGuess
            req.q.cached_gjk_guess[:] = [0.3, -0.2, 0.9]
        return b, req
    return make


def _options_mmc(pkg):
    import test_options_gpu as to
    return to._mmc_batch(pkg), pkg.abi.default_collision_request()


def _options_ms(contacts):
    def make(pkg):
        import test_options_gpu as to
        req = pkg.abi.default_collision_request()
        if contacts:
            req.num_max_contacts = 10 ** 6
        return to._ms_batch(pkg), req
    return make


def _mixed_scene(pkg):
    return pkg.workloads.mixed_scene(n=40_000, seed=3), pkg.abi.default_collision_request()


CASES = {
    # tests/test_gpu_parity.py: _check_bvh_records and its twin in test_bvh_models_beyond_16_bit_node_ids
    "bvh-first-12": Case(_cfg4(n=20000, seg=12, ring=12, n_variants=4), 0.0, "mm", 0),
    "bvh-first-50": Case(_cfg4(n=4000, seg=50, ring=50, n_variants=4), 0.0, "mm", 0),
    "bvh-cfg4-100000": Case(_cfg4(n=100_000), 0.0, "mm", 0),
    "bvh-cfg4-250000": Case(_cfg4(n=250_000), 0.0, "mm", 0),
    "bvh-forms": Case(_cfg4(n=30_000, seed=21), 0.0, "mm", 0),
    "bvh-margin": Case(_cfg4(request={"security_margin": 0.05}, n=3000, seg=12, ring=12, n_variants=2), 0.05, "mm", 0),
    "bvh-margin-0": Case(_cfg4(n=3000, seg=12, ring=12, n_variants=2), 0.0, "mm", 0),
    "bvh-wide": Case(_wide, 0.0, "mm", 0),
    "bvh-wide-solids": Case(_wide_solids, 0.0, "mixed", 0),
    "bvh-deep": Case(_deep, 0.0, "mm", 0),
    # tests/test_options_gpu.py: the mm and ms families (the mixed family's batch is the fixture of tests/test_gpu_dispatch.py)
    "options-mmc": Case(_options_mmc, 0.0, "mm", 0),
    "options-ms": Case(_options_ms(False), 0.0, "mixed", 0),
    "options-ms-contacts": Case(_options_ms(True), 0.0, "mixed", 0),
    # tests/test_bvh_shape.py
    "scene-1-0.0": Case(_scene(1, 0.0, n=20000, seed=7), 0.0, "mixed", 0),
    "scene-1000000-0.0": Case(_scene(10 ** 6, 0.0, n=20000, seed=7), 0.0, "mixed", 0),
    "scene-3-0.02": Case(_scene(3, 0.02, n=20000, seed=7), 0.02, "mixed", 0),
    "guesses-False": Case(_solid("box,capsule,convex32", 4000, 11), 0.0, "mixed", 0),
    "guesses-True": Case(_solid("box,capsule,convex32", 4000, 11, cached=True), 0.0, "mixed", 0),
    "margin-forms-box": Case(_solid("box", 4000, 8, margin=0.04), 0.04, "mixed", 0),
    "margin-forms-capsule": Case(_solid("capsule", 4000, 8, margin=0.04), 0.04, "mixed", 0),
    "long-walks-sphere": Case(_solid("sphere", 6000, 3), 0.0, "mixed", 0),
    "long-walks-box": Case(_solid("box", 6000, 3), 0.0, "mixed", 0),
    "long-walks-capsule": Case(_solid("capsule", 6000, 3), 0.0, "mixed", 0),
    "long-walks-ellipsoid": Case(_solid("ellipsoid", 6000, 3), 0.0, "mixed", 0),
    "long-walks-convex32": Case(_solid("convex32", 6000, 3), 0.0, "mixed", 0),
    "solids-100000": Case(_solid("mixed", 100_000, 1, own_request=True), 0.0, "mixed", 0),
    "flats": Case(_scene(1, 0.0, n=3000, seed=12, flats_only=True), 0.0, "mixed", 0),
    "mixed-scene": Case(_mixed_scene, 0.0, "mixed", 0),
}


def make(pkg, name):
    """(batch, request, Case) of the case `name`."""
    case = CASES[name]
    b, req = case.make(pkg)
    assert float(req.security_margin) == case.margin, name
    return b, req, case


def oracle_records(pkg, oracle, b, req, kind, n_threads=16):
    """The oracle's collide() records of batch b."""
    ML = pkg.bvh_builder.MeshLibrary(b.meshes)
    if kind == "mm":
        return oracle.bvh_collide_batch(ML, b.s1, b.s2, b.tf1, b.tf2, req, n_threads=n_threads)
    return oracle.mixed_collide_batch(b.shapes, b.verts, ML, b.s1, b.s2, b.tf1, b.tf2, req, n_threads=n_threads)
