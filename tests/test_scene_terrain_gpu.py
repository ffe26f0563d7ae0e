"""A height-field terrain under a scene's moving objects (include/hppfcl_amd_terrain.h) on the GPU.  The yardstick is the per-query call
Library.hfield_collide_device (held against the host build of the device header in tests/test_hfield_gpu.py) on explicit arrays built
with numpy (tests/terrain_model.py: expand) from the same table: records, bounds, contacts and the count of the terrain call equal its
bytes, and the summaries equal the model's fold of those records and bounds.

Shapes: fields of 2 x 2 (the root is a leaf), 5 x 7 and 34 x 34 samples under an identity and a rotated terrain pose; tables of 1, 7 and
65 rows and 1, 3 and 65 configurations, the list NULL (every row) and a strict subset; objects of the seven solid kinds placed, cycling
with the configuration, far off the field, over a cell, on an edge, on a corner and under min_height, and slabs that cover the field;
margins 0, 0.05 and -0.02; num_max_contacts 1, 2 and 5000, with a contact capacity below the produced count."""
import os
import subprocess

import numpy as np
import pytest

import hfield_cases as hc
import terrain_model as tm

pytestmark = pytest.mark.gpu
ROOT = hc.ROOT
MARGINS = (0.0, 0.05, -0.02)
GRIDS = ((2, 2), (5, 7), (34, 34))  # (nx, ny)
# (n_rows, n_conf, a strict subset?, num_max_contacts, rotated terrain pose?)
CASES = ((1, 65, False, 1, False), (7, 3, True, 2, True), (65, 1, False, 5000, False), (65, 65, True, 2, True), (7, 65, False, 2, False),
         (1, 1, False, 1, True), (65, 3, True, 1, False))


@pytest.fixture(scope="module")
def world(pkg, torch_cuda):
    rng = np.random.default_rng(7)
    fields = [("f%dx%d" % g, 3.0, 4.0, rng.uniform(0.2, 1.5, (g[1], g[0])), -0.3) for g in GRIDS]
    L, solids = hc.seven_solids(pkg, rng)
    cover = L.add_box(9.0, 9.0, 0.5)  # its box covers a whole field under any pose used here
    lib = pkg.Library(L)
    for _, x_dim, y_dim, h, mh in fields:
        lib.add_hfield(x_dim, y_dim, h, mh)
    yield dict(lib=lib, L=L, solids=solids, cover=cover, fields=fields)
    lib.close()


def _object_shapes(w, n_objects):
    """object k: one of the seven solids; every sixth object (k % 6 == 4) a slab that covers the field"""
    return np.array([w["cover"] if k % 6 == 4 else w["solids"][(k // 6 + k) % 7] for k in range(n_objects)], dtype=np.uint32)


def _table(pkg, w, f, n_rows, n_conf, rotated):
    """(terrain pose, (n_conf, n_rows, 12) table): the placements of tests/test_hfield_gpu.py, cycling with object and configuration"""
    geo = pkg.geometry
    _, x_dim, y_dim, h, mh = w["fields"][f]
    ny, nx = h.shape
    rng = np.random.default_rng(1000 * f + 10 * n_rows + n_conf)
    tfh = geo.make_pose(quat=hc.random_rotations(rng, 1)[0], T=np.array([0.4, -0.7, 0.3])) if rotated else geo.make_pose()
    shapes = _object_shapes(w, n_rows)
    local = np.zeros((n_conf, n_rows, 3))
    for c in range(n_conf):
        for k in range(n_rows):
            kind = 4 if shapes[k] == w["cover"] else (0, 1, 2, 3, 5, 1)[(k + c) % 6]
            cx, cy = int(rng.integers(0, nx - 1)), int(rng.integers(0, ny - 1))
            x0, y0 = -x_dim / 2 + (cx + 0.5) * x_dim / (nx - 1), y_dim / 2 - (cy + 0.5) * y_dim / (ny - 1)
            top = h[cy:cy + 2, cx:cx + 2].mean()
            if kind == 0:  # far off the field
                p = (40.0 + k % 5, -35.0, 20.0)
            elif kind == 1:  # over one cell, about half of them touching
                p = (x0, y0, top + rng.uniform(0.0, 0.5))
            elif kind == 2:  # on an edge
                p = (x_dim / 2 + rng.uniform(-0.05, 0.25), y0, 0.3 * top)
            elif kind == 3:  # on a corner
                p = (-x_dim / 2 - rng.uniform(-0.05, 0.2), y_dim / 2 + rng.uniform(-0.05, 0.2), 0.2)
            elif kind == 4:  # the slab dips into the highest samples, or hangs just above them
                p = (0.0, 0.0, h.max() + 0.25 - rng.uniform(-0.1, 0.3))
            else:  # below min_height
                p = (x0, y0, mh - 0.6)
            local[c, k] = p
    rot = hc.random_rotations(rng, n_conf * n_rows).reshape(n_conf, n_rows, 4)
    rot[:, shapes == w["cover"]] = (1.0, 0.0, 0.0, 0.0)  # the slab lies flat in the field's frame ...
    tfh_all = np.repeat(tfh.reshape(1, 12), n_conf * n_rows, axis=0)
    table = geo.compose(tfh_all, geo.make_pose(quat=rot.reshape(-1, 4), T=local.reshape(-1, 3)))  # ... and every solid is placed in it
    return tfh.reshape(12), np.ascontiguousarray(table.reshape(n_conf, n_rows, 12))


def _explicit(torch, lib, pkg, arrays, req, cap):
    """the yardstick: (records, bounds, contacts, produced) of Library.hfield_collide_device on explicit arrays, swapped = NULL"""
    dev = torch.device("cuda:0")
    hf, sh, tfh, tfs = arrays
    n = len(hf)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_out = torch.full((max(n, 1) * 96,), 0x5A, dtype=torch.uint8, device=dev)
    d_dlb = torch.full((max(n, 1),), -7.0, dtype=torch.float64, device=dev)
    d_con = torch.full(((cap + 2) * 96,), 0x5A, dtype=torch.uint8, device=dev)
    nc = lib.hfield_collide_device(t(hf.view(np.int32)), t(sh.view(np.int32)), t(tfh), t(tfs), n, req, d_out, d_bound=d_dlb, d_contacts=d_con,
                                   max_contacts=cap, want_count=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (d_out.cpu().numpy()[:n * 96].view(pkg.abi.RESULT_DTYPE), d_dlb.cpu().numpy()[:n],
            d_con.cpu().numpy()[:min(nc, cap) * 96].view(pkg.abi.CONTACT_DTYPE), nc)


def _terrain_device(torch, sc, pkg, table, n_t, req, cap, records=True):
    """(records, bounds, summaries, contacts, produced) of the device form; guard elements behind every output stay untouched"""
    dev = torch.device("cuda:0")
    n_conf, n = len(table), len(table) * n_t
    d_tf = torch.from_numpy(table).to(dev)
    d_out = torch.full(((n + 1) * 96,), 0x5A, dtype=torch.uint8, device=dev) if records else None
    d_dlb = torch.full((n + 1,), -7.0, dtype=torch.float64, device=dev) if records else None
    d_sum = torch.full(((n_conf + 1) * 24,), 0x5A, dtype=torch.uint8, device=dev)
    d_con = torch.full(((cap + 2) * 96,), 0x5A, dtype=torch.uint8, device=dev) if records else None
    nc = sc.collide_terrain_device(d_tf, n_conf, req, d_out, d_dlb, d_sum, d_con, cap if records else 0, want_count=True,
                                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    summ = d_sum.cpu().numpy()
    assert (summ[n_conf * 24:] == 0x5A).all(), "a summary was written past the configurations"
    summ = summ[:n_conf * 24].view(pkg.abi.SCENE_SUMMARY_DTYPE)
    if not records:
        return None, None, summ, None, nc
    out, dlb, con = d_out.cpu().numpy(), d_dlb.cpu().numpy(), d_con.cpu().numpy()
    assert (out[n * 96:] == 0x5A).all() and dlb[n] == -7.0 and (con[cap * 96:] == 0x5A).all(), "an output was written past its end"
    return out[:n * 96].view(pkg.abi.RESULT_DTYPE), dlb[:n], summ, con[:min(nc, cap) * 96].view(pkg.abi.CONTACT_DTYPE), nc


def _subset(n_rows):
    return np.array([k for k in range(n_rows) if k % 4 != 1], dtype=np.uint32)  # (slabs, k % 6 == 4, among them)


@pytest.mark.parametrize("f", range(len(GRIDS)))
def test_terrain_equals_the_explicit_call(pkg, torch_cuda, world, f):
    lib, abi = world["lib"], pkg.abi
    seen_contacts = seen_dropped = seen_free = seen_hit_confs = seen_free_confs = 0
    for k, (n_rows, n_conf, subset, nmc, rotated) in enumerate(CASES):
        req = abi.default_collision_request()
        req.security_margin = MARGINS[(k + f) % 3]
        req.num_max_contacts = nmc
        tfh, table = _table(pkg, world, f, n_rows, n_conf, rotated)
        with_env = k % 3 == 1  # two more objects behind the table's rows, standing still: n_moving < n_objects, the table narrower
        shapes = _object_shapes(world, n_rows + (2 if with_env else 0))
        objects = _subset(n_rows) if subset else np.arange(n_rows, dtype=np.uint32)
        assert (len(objects) < n_rows) == subset
        n_t = len(objects)
        what = "field %s, %d rows, %d configurations, %d listed, margin %g, num_max_contacts %d" % (GRIDS[f], n_rows, n_conf, n_t,
                                                                                                    req.security_margin, nmc)
        arrays = tm.expand(table, tfh, objects, shapes, f)
        lib.set_option("hfield_chunk", 0)
        lib.set_option("hfield_items", 0)
        want, want_dlb, want_con, want_nc = _explicit(torch_cuda, lib, pkg, arrays, req, cap=1 << 16)
        assert want_nc <= 1 << 16
        want_sum = tm.fold(want_dlb, want["status"], objects, n_conf)
        cap = want_nc // 2 if want_nc > 1 and k % 2 == 0 else want_nc  # a capacity below what is produced: counted and dropped
        sc = lib.scene(shapes, np.zeros((0, 2), dtype=np.uint32))
        if with_env:
            sc.set_environment(n_rows, pkg.geometry.make_pose(T=np.array([[50.0, 0.0, 0.0], [60.0, 0.0, 0.0]])))
            assert sc.n_moving == n_rows < sc.n_objects
        sc.set_terrain(f, tfh, objects if subset else None)
        assert sc.n_terrain_objects == n_t

        def check(got, where):
            out, dlb, summ, con, nc = got
            assert nc == want_nc, (what, where)
            assert hc.compare_records(out, want) == [] and out.tobytes() == want.tobytes(), (what, where)
            assert dlb.tobytes() == want_dlb.tobytes(), (what, where)
            assert con.tobytes() == want_con[:cap].tobytes(), (what, where)
            assert summ.tobytes() == want_sum.tobytes(), (what, where, summ, want_sum)

        # the device form: one chunk; chunks of 7 queries inside the call, which cut configurations (the contact offsets and
        # hfcl_contact::pair carried from chunk to chunk); chunks cut down because they list more than 50 items.  The one case of
        # thousands of queries takes chunks of 512 instead (no multiple of its 48 listed objects): a chunk of 7 queries gives the leaf
        # kernel too little to fill the chip with, and hundreds of them take seconds
        small = n_conf * n_t <= 1000
        for chunk, items in ((0, 0), (7, 0), (0, 50)) if small else ((0, 0), (512, 0)):
            lib.set_option("hfield_chunk", chunk)
            lib.set_option("hfield_items", items)
            check(_terrain_device(torch_cuda, sc, pkg, table, n_t, req, cap), ("device", chunk, items))
        lib.set_option("hfield_items", 0)
        for chunk in (0, 7 if small else 512):  # the host form, whole and in chunks; then summaries only, host and device
            lib.set_option("hfield_chunk", chunk)
            check(sc.collide_terrain(table, req, max_contacts=cap), ("host", chunk))
            _, _, summ, _, nc = sc.collide_terrain(table, req, records=False, bounds=False)
            assert summ.tobytes() == want_sum.tobytes() and nc == want_nc, (what, "host, summaries only", chunk)
            _, _, summ, _, nc = _terrain_device(torch_cuda, sc, pkg, table, n_t, req, 0, records=False)
            assert summ.tobytes() == want_sum.tobytes() and nc == want_nc, (what, "device, summaries only", chunk)
        lib.set_option("hfield_chunk", 0)
        sc.close()
        seen_contacts += want_nc
        seen_dropped += want_nc - cap
        seen_free += int((want["num_contacts"] == 0).sum())
        seen_hit_confs += int((want_sum["n_contacts"] > 0).sum())
        seen_free_confs += int((want_sum["n_contacts"] == 0).sum())
        assert (want_sum["n_contacts"] == (abi.status_contact(want["status"]).reshape(n_conf, n_t).sum(axis=1))).all()
    assert seen_contacts > 0 and seen_dropped > 0 and seen_free > 0 and seen_hit_confs > 0 and seen_free_confs > 0


def test_ties_skips_and_an_empty_list(pkg, torch_cuda, world):
    lib, abi = world["lib"], pkg.abi
    sphere = world["solids"][1]
    shapes = np.array([world["solids"][0], sphere, sphere, sphere], dtype=np.uint32)
    geo = pkg.geometry
    # two identical solids at one pose: the lower object index has the minimum, with and without a contact
    at = lambda z: geo.make_pose(T=np.array([[30.0, 30.0, 30.0], [0.1, 0.2, z], [5.0, 5.0, 9.0], [0.1, 0.2, z]])).reshape(1, 4, 12)  # noqa: E731
    table = np.concatenate([at(0.1), at(4.0)])  # (the field's heights are at least 0.2: a sphere centred at 0.1 is inside the solid)
    sc = lib.scene(shapes, np.zeros((0, 2), dtype=np.uint32))
    sc.set_terrain(1, geo.make_pose().reshape(12))
    rec, dlb, summ, _, nc = sc.collide_terrain(table)
    assert dlb[1] == dlb[3] and dlb[5] == dlb[7] and rec[1].tobytes() == rec[3].tobytes()
    assert summ["min_pair"].tolist() == [1, 1] and summ["min_distance"].tolist() == [dlb[1], dlb[5]]
    assert summ["n_contacts"].tolist() == [2, 0] and summ["first_contact"].tolist() == [1, tm.NONE] and nc == 2
    # the list in another order of objects: the key is the object index, not the rank
    sc.set_terrain(1, geo.make_pose().reshape(12), [2, 3])
    _, dlb2, summ2, _, _ = sc.collide_terrain(table)
    assert summ2["min_pair"].tolist() == [3, 3] and summ2["first_contact"].tolist() == [3, tm.NONE] and dlb2[1] == dlb[3]
    # security_margin = -inf: every record skipped
    req = abi.default_collision_request()
    req.security_margin = -np.inf
    rec, dlb, summ, con, nc = sc.collide_terrain(table, req, max_contacts=4)
    assert nc == 0 and len(con) == 0 and (abi.status_skipped(rec["status"]) == 1).all() and (dlb == np.finfo(np.float64).max).all()
    assert (summ["n_skipped"] == 2).all() and (summ["min_distance"] == np.inf).all() and (summ["min_pair"] == tm.NONE).all()
    assert (summ["n_contacts"] == 0).all() and (summ["first_contact"] == tm.NONE).all()
    # an empty list is legal: no query, every summary the fold of nothing; no configuration: nothing at all
    sc.set_terrain(1, geo.make_pose().reshape(12), [])
    assert sc.n_terrain_objects == 0
    rec, dlb, summ, con, nc = sc.collide_terrain(table)
    assert len(rec) == 0 and nc == 0 and summ.tobytes() == tm.fold(np.zeros(0), np.zeros(0, dtype=np.uint32), [], 2).tobytes()
    sc.set_terrain(1, geo.make_pose().reshape(12))
    rec, dlb, summ, con, nc = sc.collide_terrain(np.zeros((0, 4, 12)))
    assert len(rec) == 0 and len(summ) == 0 and nc == 0
    sc.clear_terrain()
    assert sc.n_terrain_objects == 0
    sc.close()


def test_refusals(pkg, torch_cuda):
    abi, geo = pkg.abi, pkg.geometry
    mesh = pkg.workloads.mesh_variants(1, 12, 10)[0]
    L = pkg.ShapeLibrary()
    ball, box = L.add_sphere(0.3), L.add_box(0.2, 0.3, 0.4)
    m = L.add_bvh(0, len(mesh.vertices))
    flat = L.add_halfspace((0, 0, 1), 0.0)
    lib = pkg.Library(L)
    lib.add_bvh(mesh)
    field = lib.add_hfield(1.0, 1.0, np.ones((2, 2)), 0.0)
    ident = geo.make_pose().reshape(12)
    sc = lib.scene(np.array([ball, box, m, flat, ball], dtype=np.uint32), np.zeros((0, 2), dtype=np.uint32))
    table = geo.make_pose(T=np.array([[0.0, 0.0, 1.2], [0.0, 0.0, 3.0], [9.0, 0.0, 0.0], [0.0, 9.0, 0.0], [0.2, 0.0, 1.1]])).reshape(1, 5, 12)

    def code(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except pkg.engine.EngineError as e:
            return e.code
        return abi.OK

    assert code(sc.collide_terrain, table) == abi.ERR_INVALID_ARGUMENT and "no terrain" in pkg.engine.last_error()  # no terrain set
    assert code(sc.set_terrain, field, ident, [0, 2]) == abi.ERR_UNSUPPORTED_PAIR  # a mesh in the list
    assert code(sc.set_terrain, field, ident, [0, 3]) == abi.ERR_UNSUPPORTED_PAIR  # a halfspace
    assert code(sc.set_terrain, field, ident) == abi.ERR_UNSUPPORTED_PAIR  # NULL: every object, the mesh among them
    assert code(sc.set_terrain, field, ident, [1, 0]) == abi.ERR_INVALID_ARGUMENT  # descending
    assert code(sc.set_terrain, field, ident, [0, 0]) == abi.ERR_INVALID_ARGUMENT  # not strictly ascending
    assert code(sc.set_terrain, field, ident, [0, 5]) == abi.ERR_INVALID_ARGUMENT  # outside the scene
    assert code(sc.set_terrain, field + 1, ident, [0]) == abi.ERR_INVALID_ARGUMENT  # no such field
    assert sc.n_terrain_objects == 0 and code(sc.collide_terrain, table) == abi.ERR_INVALID_ARGUMENT  # (a refused set call sets nothing)
    assert code(sc.set_terrain, field, ident, [0, 1, 4]) == abi.OK and sc.n_terrain_objects == 3
    rec, dlb, summ, _, nc = sc.collide_terrain(table)
    assert rec["num_contacts"].tolist() == [1, 0, 1] and summ["first_contact"][0] == 0 and summ["n_contacts"][0] == 2 and nc == 2
    assert summ["min_pair"][0] == (0 if dlb[0] <= dlb[2] else 4)

    def req_code(**kw):
        req = abi.default_collision_request()
        for k, v in kw.items():
            setattr(req.q if hasattr(req.q, k) else req, k, v)
        return code(sc.collide_terrain, table, req)

    assert req_code() == abi.OK
    assert req_code(num_max_contacts=0) == abi.ERR_INVALID_ARGUMENT
    assert req_code(epa_max_iterations=65) == abi.ERR_LIMIT
    assert req_code(gjk_initial_guess=abi.CachedGuess) == abi.ERR_LIMIT
    assert req_code(distance_upper_bound=1.0) == abi.ERR_LIMIT
    # an environment set afterwards that cuts below a listed index; cleared again, the call works
    sc.set_environment(4, geo.make_pose(T=np.array([[0.2, 0.0, 1.1]])))
    assert code(sc.collide_terrain, table[:, :4]) == abi.ERR_INVALID_ARGUMENT and "environment" in pkg.engine.last_error()
    sc.clear_environment()
    assert code(sc.collide_terrain, table) == abi.OK
    # the fields cleared: the index is no longer on the library
    lib.clear_hfields()
    assert code(sc.collide_terrain, table) == abi.ERR_INVALID_ARGUMENT and "no longer" in pkg.engine.last_error()
    assert lib.add_hfield(1.0, 1.0, np.full((2, 2), 0.5), 0.0) == field  # a caller who registers the updated field and sets it again moves on
    sc.set_terrain(field, ident, [0, 1, 4])
    assert sc.collide_terrain(table)[0]["num_contacts"].tolist() == [0, 0, 0]
    # hfcl_lib_set_shapes: the scene is stale, as for the other scene calls
    shapes, verts = np.ascontiguousarray(L.shapes_array()), np.ascontiguousarray(L.vertices_array(), dtype=np.float64)
    import ctypes as C
    assert pkg.engine.dll().hfcl_lib_set_shapes(lib._h, abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), C.c_size_t(len(verts))) == abi.OK
    assert code(sc.collide_terrain, table) == abi.ERR_INVALID_ARGUMENT and "hfcl_lib_set_shapes" in pkg.engine.last_error()
    assert code(sc.set_terrain, field, ident, [0]) == abi.ERR_INVALID_ARGUMENT
    sc.close()
    lib.close()


def test_neighbours_unchanged(pkg, torch_cuda, world):
    """a standalone hfield_collide_device call and a scene.collide call, each before and after a terrain call on the same library"""
    lib, abi = world["lib"], pkg.abi
    req = abi.default_collision_request()
    req.num_max_contacts = 3
    tfh, table = _table(pkg, world, 1, 7, 3, True)
    shapes = _object_shapes(world, 7)
    arrays = tm.expand(table, tfh, np.arange(7), shapes, 1)
    pairs = np.array([[0, 1], [1, 2], [2, 3], [0, 5], [3, 6]], dtype=np.uint32)
    sc = lib.scene(shapes, pairs)
    dreq = abi.default_collision_request()
    before = _explicit(torch_cuda, lib, pkg, arrays, req, 64), sc.collide(table, dreq)
    sc.set_terrain(1, tfh)
    got = sc.collide_terrain(table, req, max_contacts=64)
    after = _explicit(torch_cuda, lib, pkg, arrays, req, 64), sc.collide(table, dreq)
    for a, b in zip(before[0][:3], after[0][:3]):
        assert a.tobytes() == b.tobytes()
    assert before[0][3] == after[0][3] == got[4]
    assert before[1][0].tobytes() == after[1][0].tobytes() and before[1][1].tobytes() == after[1][1].tobytes()
    assert got[0].tobytes() == before[0][0].tobytes() and got[3].tobytes() == before[0][2].tobytes()
    sc.close()


def test_compat_collide_terrain(pkg, torch_cuda):
    fcl = pkg.compat
    rng = np.random.default_rng(3)
    h = rng.uniform(0.2, 1.0, (6, 5))
    field = fcl.HeightFieldAABB(2.0, 3.0, h, -0.2)
    ftf = fcl.Transform3f(np.eye(3), np.array([0.1, -0.2, 0.05]))
    geoms = [fcl.Sphere(0.3), fcl.Box(0.4, 0.3, 0.5), fcl.Halfspace((0, 0, 1), -5.0), fcl.Capsule(0.15, 0.4), fcl.Cylinder(0.2, 0.3)]
    objs = [fcl.CollisionObject(g, fcl.Transform3f()) for g in geoms]
    confs = [[fcl.Transform3f(np.eye(3), np.array([rng.uniform(-0.8, 0.8), rng.uniform(-1.2, 1.2), rng.uniform(0.6, 1.5)])) for _ in objs]
             for _ in range(4)]
    req = fcl.CollisionRequest()
    req.num_max_contacts = 4
    req.security_margin = 0.01
    results, summ = fcl.collide_terrain(objs, field, ftf, req, transforms=confs)
    listed = [0, 1, 3, 4]  # (the halfspace has no evaluator: not listed)
    hits = 0
    for c, conf in enumerate(confs):
        assert len(results[c]) == len(listed)
        first, count = tm.NONE, 0
        for k, i in enumerate(listed):
            ref = fcl.CollisionResult()
            fcl.collide(field, ftf, geoms[i], conf[i], req, ref)
            got = results[c][k]
            assert got.numContacts() == ref.numContacts() and got.distance_lower_bound == ref.distance_lower_bound
            if ref.isCollision():
                a, b = got.getContact(0), ref.getContact(0)
                assert a.b1 == b.b1 and a.b2 == b.b2 and a.penetration_depth == b.penetration_depth
                assert np.array_equal(a.normal, b.normal) and np.array_equal(a.pos, b.pos) and a.o1 is field and a.o2 is geoms[i]
                first, count = min(first, i), count + 1
        assert summ[c]["n_contacts"] == count and summ[c]["first_contact"] == first
        hits += count
    assert 0 < hits < len(confs) * len(listed)
    with pytest.raises(ValueError):
        fcl.collide_terrain(objs, field, ftf, req, transforms=confs, object_indices=[0, 2])


def test_cpp_shim(pkg, torch_cuda, tmp_path):
    exe = str(tmp_path / "test_terrain_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_terrain", "test_terrain_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "terrain shim ok" in r.stdout and "FAILED" not in r.stdout
