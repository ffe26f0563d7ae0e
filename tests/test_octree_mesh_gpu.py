"""OcTree x BVHModel<OBBRSS> collide() (include/hppfcl_amd_octree_mesh.h) on the GPU.  The yardstick is the host build of the device
header (tests/octree_mesh_harness, held against the fp64 model in tests/test_octree_mesh_cpu.py): records, bounds, contacts and counts
of the device call equal the harness's byte for byte, the host call equals the device call for two values of the chunk option and for
a small item cap.  Independent of the harness, on a tree whose halvings are exact: the (node, triangle) contact set of a query is what
the per-pair collide of this library says of every occupied leaf's Box against every triangle.

Trees: the six of tests/test_octree_gpu.py.  Meshes: one triangle, the 12 triangles of a box, a 288-triangle sphere, a chain BVH at the
depth limit, and on the block a flat sheet that covers it (more items in one query than a workgroup has lanes, between queries with
none).  Batches of 1, 63, 64, 65 and 257 queries; identity and rotated poses; both orders; margins {0, 0.05}; num_max_contacts
{1, 3, 5000}."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import octree_cases as oc
import octree_mesh_cases as omc

pytestmark = pytest.mark.gpu
ROOT = oc.ROOT
SIZES = (1, 63, 64, 65, 257)
MARGINS = (0.0, 0.05)
MAX_CONTACTS = (1, 3, 5000)
TREES = ("empty", "root", "three_state", "mixed_depth4", "chain16", "block")
SHEET = 4  # the flat mesh's id


def _trees(pkg):
    return [(oc.empty_tree(pkg), 0.1, 3), (oc.tree_from_spec(pkg, oc.OCCUPIED), 0.1, 2), (oc.three_state_tree(pkg), 0.1, 2),
            (oc.random_tree(pkg, np.random.default_rng(41), 4), 0.1, 4), (oc.chain_tree(pkg, 16), 0.001, 16), (oc.block_tree(pkg), 0.1, 4)]


def _library(pkg, meshes, trees):
    """a library whose shape row i is mesh i, with one sphere row behind them"""
    L = pkg.geometry.ShapeLibrary()
    for k, m in enumerate(meshes):
        assert L.add_bvh(k, len(m.vertices)) == k
    ball = L.add_sphere(0.1)
    lib = pkg.Library(L)
    for k, m in enumerate(meshes):
        assert lib.add_bvh(m) == k
    for nodes, res, depth in trees:
        lib.add_octree(nodes, res, depth)
    return lib, ball


@pytest.fixture(scope="module")
def world(pkg, torch_cuda, tmp_path_factory):
    trees = _trees(pkg)
    meshes = [omc.one_triangle(), omc.box_mesh(), omc.sphere_mesh(pkg), omc.chain_mesh(omc.DEPTH_LIMIT), omc.flat_mesh(2)]
    assert [len(m.triangles) for m in meshes] == [1, 12, 288, omc.DEPTH_LIMIT, 8]
    lib, ball = _library(pkg, meshes, trees)
    yield dict(lib=lib, ball=ball, trees=trees, meshes=meshes, tables=oc.HarnessTrees(pkg, trees), mtables=omc.HarnessMeshes(pkg, meshes),
               harness=omc.build_harness(tmp_path_factory.mktemp("octree_mesh_harness")))
    lib.close()


def _queries(pkg, w, t, n):
    """n queries on tree t: meshes 0 - 3 (the block: 0 and 1) near its reachable leaves (about half touching), every fifth far off; on
    the block every seventh is the covering sheet, flat in the tree's frame at some height inside the block"""
    geo = pkg.geometry
    rng = np.random.default_rng(1000 * t + n)
    # (on the block the two small meshes only: a walk of 512 voxels against 288 triangles is tens of milliseconds on its one lane, and
    # the host form with a small item cap walks a batch once per chunk)
    _, me, tft, tfm, swapped = omc.random_queries(pkg, rng, [w["trees"][t]], 2 if TREES[t] == "block" else 4, n, spread=0.25 if t != 4 else 0.05)
    far = np.arange(n) % 5 == 4
    if far.any():
        tfm[far] = geo.make_pose(quat=oc.random_rotations(rng, int(far.sum())), T=rng.uniform(30.0, 40.0, (int(far.sum()), 3)))
    if TREES[t] == "block" and n > 3:
        sheet = np.arange(n) % 7 == 3
        me[sheet] = SHEET
        local = np.zeros((int(sheet.sum()), 3))
        local[:, 2] = rng.uniform(0.02, 0.7, int(sheet.sum()))
        tfm[sheet] = geo.compose(tft[sheet], geo.make_pose(T=local))
    return np.full(n, t, dtype=np.uint32), me.astype(np.uint32), tft, tfm, swapped


def _device(torch, lib, pkg, ot, sh, tft, tfm, sw, req, cap):
    dev = torch.device("cuda:0")
    n = len(ot)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_ot, d_sh, d_tft, d_tfm, d_sw = t(ot.view(np.int32)), t(sh.view(np.int32)), t(tft), t(tfm), t(sw)
    d_out = torch.full((n * 96,), 0x5A, dtype=torch.uint8, device=dev)
    d_dlb = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    d_con = torch.full(((cap + 2) * 96,), 0x5A, dtype=torch.uint8, device=dev)  # (two guard records behind the capacity)
    nc = lib.octree_mesh_collide_device(d_ot, d_sh, d_tft, d_tfm, n, req, d_out, d_swapped=d_sw, d_bound=d_dlb, d_contacts=d_con,
                                        max_contacts=cap, want_count=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    con = d_con.cpu().numpy()
    assert (con[cap * 96:] == 0x5A).all(), "a contact was written past the capacity"
    return d_out.cpu().numpy().view(pkg.abi.RESULT_DTYPE), d_dlb.cpu().numpy(), con[:min(nc, cap) * 96].view(pkg.abi.CONTACT_DTYPE), nc


@pytest.mark.parametrize("t", range(len(TREES)), ids=TREES)
def test_device_equals_harness_and_host_equals_device(pkg, torch_cuda, world, t):
    lib, abi = world["lib"], pkg.abi
    seen_contacts = seen_dropped = seen_free = most_items = 0
    used = set()
    for k, n in enumerate(SIZES):
        req = abi.default_collision_request()
        req.security_margin = MARGINS[(k + t) % 2]
        req.num_max_contacts = MAX_CONTACTS[(k + t) % 3]
        ot, me, tft, tfm, sw = _queries(pkg, world, t, n)
        want, want_dlb, want_con, want_nc, items = omc.harness_collide(pkg, world["harness"], world["tables"], world["mtables"], ot, me, tft, tfm,
                                                                      req, sw, cap=1 << 17, items_cap=1 << 18)
        assert want_nc <= 1 << 17 and len(items) < 1 << 18
        what = "tree %s, %d queries, margin %g, num_max_contacts %d, %d items" % (TREES[t], n, req.security_margin, req.num_max_contacts, len(items))
        # a capacity below what is produced (where anything is): counted and dropped
        cap = want_nc // 2 if want_nc > 1 and k % 2 == 0 else want_nc
        got, dlb, con, nc = _device(torch_cuda, lib, pkg, ot, me, tft, tfm, sw, req, cap)
        assert nc == want_nc, what
        assert oc.compare_records(got, want) == [], what
        assert dlb.tobytes() == want_dlb.tobytes(), what
        assert con.tobytes() == want_con[:cap].tobytes(), what
        # the host form: whole; in chunks of 7 queries (the contact offsets and hfcl_contact::pair carried from chunk to chunk); with
        # chunks cut down because they list more than 50 items (a chunk of one query is never cut)
        for chunk, cut in ((0, 0), (7, 0), (0, 50)):
            lib.set_option("octree_chunk", chunk)
            lib.set_option("octree_items", cut)
            h_out, h_dlb, h_con, h_nc = lib.octree_mesh_collide(ot, me, tft, tfm, req, swapped=sw, max_contacts=cap)
            assert h_nc == nc and h_out.tobytes() == got.tobytes() and h_dlb.tobytes() == dlb.tobytes() and h_con.tobytes() == con.tobytes(), what
        lib.set_option("octree_chunk", 0)
        lib.set_option("octree_items", 0)
        seen_contacts += want_nc
        seen_dropped += want_nc - cap
        seen_free += int((want["num_contacts"] == 0).sum())
        per_query = np.bincount(items[:, 0], minlength=n) if len(items) else np.zeros(n, dtype=int)
        most_items = max(most_items, int(per_query.max()))
        used |= set(int(m) for m in me)
        assert (got["status"] & abi.STATUS_SWAPPED != 0).tolist() == sw.astype(bool).tolist()
        hit = got["num_contacts"] > 0
        assert (got["b2"][hit] >= 0).all() and (got["b1"][hit] >= 0).all() and (got["b1"][~hit] == -1).all() and (got["b2"][~hit] == -1).all()
    assert ({0, 1} if TREES[t] == "block" else {0, 1, 2, 3}) <= used
    if TREES[t] == "empty":
        assert seen_contacts == 0 and most_items == 0
    else:
        assert seen_contacts > 0 and seen_dropped > 0 and seen_free > 0
    if TREES[t] == "block":
        assert SHEET in used and most_items > 64  # the sheets: more items in a query than a workgroup has lanes


def test_contacts_are_the_per_pair_answers_of_leaves_and_triangles(pkg, torch_cuda):
    """Independent of the harness.  Resolution 0.25 and a tree pose that is a dyadic translation: every halving and every leaf pose is
    exact.  With num_max_contacts = 5000 the (node, triangle) contacts of a query are the pairs of an occupied leaf's Box (a library
    Box of that side at that pose) and a triangle of the mesh (a library TriangleP under the mesh's pose) whose per-pair record from
    hfcl_collide_batch has the contact flag -- depth, normal and points to 1e-9, Box first."""
    abi, geo, fcl = pkg.abi, pkg.geometry, pkg.compat
    rng = np.random.default_rng(2)
    nodes = oc.random_tree(pkg, rng, 3)
    tree = fcl.OcTree(nodes, 0.25, 3)
    boxes = tree.toBoxes()
    leaves = [(i, lo, hi) for i, lo, hi in tree._leaves() if nodes[i]["occupancy"] >= 0.5]
    assert len(boxes) == len(leaves) >= 20
    meshes = [omc.one_triangle(0.6), omc.box_mesh(0.3, 0.2, 0.35), omc.two_triangles(0.5)]
    L = geo.ShapeLibrary()
    for k, m in enumerate(meshes):
        L.add_bvh(k, len(m.vertices))
    side_id = {s: L.add_box(s, s, s) for s in (0.25, 0.5, 1.0)}
    tri_id = [[L.add_triangle(*m.vertices[t]) for t in m.triangles] for m in meshes]
    lib = pkg.Library(L)
    for m in meshes:
        lib.add_bvh(m)
    tid = lib.add_octree(nodes, 0.25, 3)
    shift = np.array([0.5, -0.25, 0.125])
    nb = len(boxes)
    seen = 0
    for k, m in enumerate(meshes):
        n, nt = 30, len(m.triangles)
        tft = geo.make_pose(T=np.tile(shift, (n, 1)))
        tfm = geo.make_pose(quat=oc.random_rotations(rng, n), T=rng.uniform(-0.9, 0.9, (n, 3)) + shift)
        # explicit pairs: query-major, then leaf, then triangle
        s1 = np.tile(np.repeat(np.array([side_id[float(b[3])] for b in boxes], dtype=np.uint32), nt), n)
        s2 = np.tile(np.array(tri_id[k], dtype=np.uint32), n * nb)
        tf1 = geo.make_pose(T=np.tile(np.repeat(boxes[:, :3] + shift, nt, axis=0), (n, 1)))
        tf2 = np.repeat(tfm.reshape(n, 12), nb * nt, axis=0)
        for margin in MARGINS:
            req = abi.default_collision_request()
            req.security_margin = margin
            pair = lib.collide(s1, s2, tf1, tf2, req).reshape(n, nb, nt)
            flag = abi.status_contact(pair["status"]) != 0
            req.num_max_contacts = 5000
            rec, dlb, con, nc = lib.octree_mesh_collide(np.full(n, tid), np.full(n, k), tft, tfm, req, max_contacts=n * nb * nt)
            assert nc == int(flag.sum()) == len(con) and (rec["num_contacts"] == flag.sum(axis=(1, 2))).all(), (k, margin)
            for q in range(n):
                mine = {(int(c["b1"]), int(c["b2"])): c for c in con[con["pair"] == q]}
                assert set(mine) == {(leaves[j][0], tr) for j, tr in zip(*np.nonzero(flag[q]))}, (k, margin, q)
                for j, tr in zip(*np.nonzero(flag[q])):
                    c, r = mine[(leaves[j][0], int(tr))], pair[q, j, tr]
                    # (the per-pair kernel's own copy of the solver: the numbers equal to rounding, Box first)
                    assert abs(float(c["penetration_depth"]) - float(r["distance"])) <= 1e-9, (k, margin, q)
                    for f in ("normal", "p1", "p2"):
                        assert np.allclose(c[f], r[f], rtol=0, atol=1e-9), (k, margin, q, f)
            assert (dlb <= (pair["distance"] - margin).min(axis=(1, 2)) + 1e-12).all()
            seen += int(flag.sum())
    assert seen > 100
    lib.close()


def test_mesh_first_is_the_octree_first_result_plus_bit_23(pkg, torch_cuda, world):
    lib, abi = world["lib"], pkg.abi
    ot, me, tft, tfm, _ = _queries(pkg, world, 3, 65)
    req = abi.default_collision_request()
    req.num_max_contacts = 3
    a, a_dlb, a_con, a_nc = lib.octree_mesh_collide(ot, me, tft, tfm, req, swapped=np.zeros(65, dtype=np.uint8), max_contacts=256)
    b, b_dlb, b_con, b_nc = lib.octree_mesh_collide(ot, me, tft, tfm, req, swapped=np.ones(65, dtype=np.uint8), max_contacts=256)
    c = lib.octree_mesh_collide(ot, me, tft, tfm, req, max_contacts=256)[0]  # (swapped: NULL)
    assert a_nc == b_nc > 0 and a_con.tobytes() == b_con.tobytes() and a_dlb.tobytes() == b_dlb.tobytes() and a.tobytes() == c.tobytes()
    assert oc.compare_records(a, b) == ["status"] and (b["status"] == a["status"] | abi.STATUS_SWAPPED).all() and (a["status"] & abi.STATUS_SWAPPED == 0).all()
    # the older calls keep refusing a mesh: the octree x solid host form on the same ids
    with pytest.raises(pkg.engine.EngineError) as e:
        lib.octree_collide(ot, me, tft, tfm, req)
    assert e.value.code == abi.ERR_UNSUPPORTED_PAIR


def test_requests_limits_and_bad_ids(pkg, torch_cuda, world):
    lib, abi, torch = world["lib"], pkg.abi, torch_cuda
    ot, me, tft, tfm, sw = _queries(pkg, world, 3, 6)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    def codes(lib, ot, me, req, count_kept=True):
        """(host form's code, device form's code); a refusal leaves every output byte as it was (count_kept: *n_contacts_out too -- the
        refusals of the request and of a mesh too deep come before it is zeroed)"""
        n = len(ot)
        out = np.full(n * 96, 0x5A, dtype=np.uint8).view(abi.RESULT_DTYPE)
        dlb, nc = np.full(n, -7.0), C.c_size_t(77)
        con = np.full(4 * 96, 0x5A, dtype=np.uint8).view(abi.CONTACT_DTYPE)
        ot, me = np.ascontiguousarray(ot, dtype=np.uint32), np.ascontiguousarray(me, dtype=np.uint32)
        a_tft, a_tfm = np.ascontiguousarray(tft[:n]).reshape(-1, 12), np.ascontiguousarray(tfm[:n]).reshape(-1, 12)
        rc = pkg.engine.dll().hfcl_octree_mesh_collide_batch(lib._h, abi.ptr(ot), abi.ptr(me), abi.ptr(a_tft), abi.ptr(a_tfm), C.c_size_t(n), None,
                                                             C.byref(req), abi.ptr(out), abi.ptr(dlb), abi.ptr(con), C.c_size_t(4), C.byref(nc))
        if rc:
            assert (out.view(np.uint8) == 0x5A).all() and (dlb == -7.0).all() and (con.view(np.uint8) == 0x5A).all() and (nc.value == 77 or not count_kept)
        d_out = torch.full((n * 96,), 0x5A, dtype=torch.uint8, device=dev)
        try:
            lib.octree_mesh_collide_device(t(ot.view(np.int32)), t(me.view(np.int32)), t(a_tft), t(a_tfm), n, req, d_out, want_count=True)
            rc2 = abi.OK
        except pkg.engine.EngineError as e:
            rc2 = e.code
            torch.cuda.synchronize()
            assert (d_out.cpu().numpy() == 0x5A).all()
        torch.cuda.synchronize()
        return rc, rc2, d_out.cpu().numpy().view(abi.RESULT_DTYPE)

    def request(**kw):
        req = abi.default_collision_request()
        for k, v in kw.items():
            setattr(req.q if hasattr(req.q, k) else req, k, v)
        return req

    assert codes(lib, ot, me, request())[:2] == (abi.OK, abi.OK)
    for kw, want in ((dict(num_max_contacts=0), abi.ERR_INVALID_ARGUMENT), (dict(security_margin=-0.01), abi.ERR_INVALID_ARGUMENT),
                     (dict(epa_max_iterations=65), abi.ERR_LIMIT), (dict(gjk_initial_guess=abi.CachedGuess), abi.ERR_LIMIT),
                     (dict(gjk_initial_guess=abi.BoundingVolumeGuess), abi.ERR_LIMIT), (dict(distance_upper_bound=1.0), abi.ERR_LIMIT)):
        assert codes(lib, ot, me, request(**kw))[:2] == (want, want), kw
    # -inf margin: every record skipped
    out, dlb, con, nc = lib.octree_mesh_collide(ot, me, tft, tfm, request(security_margin=-np.inf), swapped=sw, max_contacts=4)
    assert nc == 0 and (abi.status_skipped(out["status"]) == 1).all() and (dlb == np.finfo(np.float64).max).all()
    # a shape that is no mesh, ids outside the library: refused by the host form, skipped records from the device form
    ball, n_trees = world["ball"], len(world["trees"])
    rc, rc2, got = codes(lib, [3, 3, 3], [0, ball, 1], request(), False)
    assert (rc, rc2) == (abi.ERR_UNSUPPORTED_PAIR, abi.OK) and abi.status_skipped(got["status"]).tolist() == [0, 1, 0]
    rc, rc2, got = codes(lib, [3, n_trees, 3], [0, 1, ball + 1], request(), False)
    assert (rc, rc2) == (abi.ERR_INVALID_ARGUMENT, abi.OK) and abi.status_skipped(got["status"]).tolist() == [0, 1, 1]
    assert (got["num_contacts"][1:] == 0).all() and (got["distance"][1:] == 0).all()
    # a mesh one level deeper than the limit: the host form refuses a batch that NAMES it and runs one that does not; the device form
    # cannot see the ids and refuses while it is registered at all
    deep = [omc.one_triangle(), omc.chain_mesh(omc.DEPTH_LIMIT + 1)]
    lib2, _ = _library(pkg, deep, world["trees"])
    rc, rc2, _ = codes(lib2, [3, 3], [0, 1], request())
    assert (rc, rc2) == (abi.ERR_LIMIT, abi.ERR_LIMIT) and "levels" in pkg.engine.last_error()
    rc, rc2, _ = codes(lib2, [3, 3], [0, 0], request())
    assert (rc, rc2) == (abi.OK, abi.ERR_LIMIT)
    lib2.close()


def _shim_cases(pkg, nodes, meshes, rng, n):
    """queries of tests/cpp/test_octree_mesh.cpp's input: (mesh, tf_tree, tf_mesh, swapped, margin, num_max_contacts)"""
    geo = pkg.geometry
    boxes = oc.leaf_boxes(nodes, 0.1, 4)
    cases = []
    for i in range(n):
        tft = geo.make_pose(quat=oc.random_rotations(rng, 1)[0], T=rng.uniform(-1.0, 1.0, 3)) if i % 3 else geo.make_pose()
        _, lo, hi = boxes[int(rng.integers(0, len(boxes)))]
        local = 0.5 * (np.array(lo) + np.array(hi)) + rng.uniform(-0.15, 0.15, 3)
        tfm = geo.make_pose(quat=oc.random_rotations(rng, 1)[0], T=geo.transform_point(tft.reshape(1, 12), local.reshape(1, 3))[0])
        cases.append((i % len(meshes), np.asarray(tft).ravel(), np.asarray(tfm).ravel(), i % 2, (0.0, 0.05)[(i // 2) % 2], (1, 3, 5000)[i % 3]))
    return cases


def test_compat_and_cpp_shim_agree(pkg, torch_cuda, tmp_path):
    """compat.collide / ComputeCollision dispatch OcTree x BVHModel in both orders, and hpp::fcl::collide of the C++ shim gives the same
    numbers on the same cases"""
    fcl = pkg.compat
    nodes = oc.random_tree(pkg, np.random.default_rng(41), 4)
    shapes = [omc.one_triangle(), omc.box_mesh(), omc.sphere_mesh(pkg, seg=6, ring=5)]
    cases = _shim_cases(pkg, nodes, shapes, np.random.default_rng(9), 24)
    tree = fcl.OcTree(nodes, 0.1, 4)
    models = []
    for m in shapes:
        bm = fcl.BVHModelOBBRSS()
        bm.beginModel()
        bm.addSubModel(m.vertices, m.triangles)
        bm.endModel()
        models.append(bm)
    lines_want, hits = [], 0
    for mesh, tft, tfm, swapped, margin, nmax in cases:
        tf_t = fcl.Transform3f(tft[:9].reshape(3, 3).T, tft[9:])
        tf_m = fcl.Transform3f(tfm[:9].reshape(3, 3).T, tfm[9:])
        req, res = fcl.CollisionRequest(), fcl.CollisionResult()
        req.security_margin, req.num_max_contacts = margin, nmax
        if swapped:
            fcl.collide(models[mesh], tf_m, tree, tf_t, req, res)
        else:
            fcl.ComputeCollision(tree, models[mesh])(tf_t, tf_m, req, res)
        words = [str(res.numContacts()), float(res.distance_lower_bound).hex()]
        for k in range(res.numContacts()):
            ct = res.getContact(k)
            assert ct.o1 is tree and ct.o2 is models[mesh] and 0 <= ct.b2 < len(shapes[mesh].triangles)
            words += [str(int(ct.b1)), str(int(ct.b2)), float(ct.penetration_depth).hex()]
            words += [float(x).hex() for x in list(ct.normal) + list(ct.getNearestPoint1()) + list(ct.getNearestPoint2())]
        hits += res.numContacts() > 0
        lines_want.append(words)
    assert 4 < hits < len(cases)
    neg = fcl.CollisionRequest()
    neg.security_margin = -0.01
    with pytest.raises(ValueError):
        fcl.collide(tree, fcl.Transform3f(), models[0], fcl.Transform3f(), neg, fcl.CollisionResult())
    with pytest.raises(ValueError):  # distance() for the pair: not done
        fcl.distance(tree, fcl.Transform3f(), models[0], fcl.Transform3f(), fcl.DistanceRequest(), fcl.DistanceResult())

    # the same cases through the C++ shim
    exe = str(tmp_path / "test_octree_mesh")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_octree_mesh.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("%r 4 %d %d %d\n" % (0.1, len(nodes), len(shapes), len(cases)))
        for nd in nodes:
            f.write(" ".join(str(int(c)) for c in nd["child"]) + " %r\n" % float(nd["occupancy"]))
        for m in shapes:
            f.write("%d %d\n" % (len(m.vertices), len(m.triangles)))
            for v in m.vertices:
                f.write(" ".join(repr(float(x)) for x in v) + "\n")
            for t in m.triangles:
                f.write(" ".join(str(int(x)) for x in t) + "\n")
        for mesh, tft, tfm, swapped, margin, nmax in cases:
            f.write("%d " % mesh + " ".join(repr(float(x)) for x in list(tft) + list(tfm)) + " %d %r %d\n" % (swapped, margin, nmax))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    for want, line in zip(lines_want, out[:len(cases)]):
        got = line.split()
        assert got[0] == want[0] and len(got) == len(want), (got, want)
        for g, w in zip(got[1:], want[1:]):
            assert (int(g) == int(w)) if "x" not in w and "n" not in w else (float.fromhex(g) == float.fromhex(w) or (g == w)), (got, want)
    assert "tree first: ok" in r.stdout and "batch: ok" in r.stdout and "negative margin and distance refused" in r.stdout
