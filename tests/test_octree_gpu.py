"""OcTree x convex solid collide() (include/hppfcl_amd_octree.h) on the GPU.  The yardstick is the host build of the device header
(tests/octree_harness, held against the fp64 model in tests/test_octree_cpu.py): records, bounds, contacts and counts of the device
call equal the harness's byte for byte, the host call equals the device call for two values of the chunk option.  Independent of the
harness, on a tree whose halvings are exact: the contact set of a query is what the per-pair collide of this library says of every
occupied leaf's Box.

Trees, the smallest on which each piece can go wrong: the empty tree; the root alone as an occupied leaf; depth 2 with a free, an
uncertain and an occupied child plus an inner node below the threshold whose children are occupied; depth 4 with 67 leaves at mixed
levels at resolution 0.1; one chain down to a single voxel at depth 16 with a few siblings (the deepest stack); a full 8 x 8 x 8 block
under a covering slab (more items in one query than a workgroup has lanes, between queries with none).  Batches of 1, 63, 64, 65 and
257 queries; identity and rotated tree poses; the seven kinds, both orders; margins {0, 0.05}; num_max_contacts {1, 3, 5000}."""
import os
import subprocess

import numpy as np
import pytest

import octree_cases as oc

pytestmark = pytest.mark.gpu
ROOT = oc.ROOT
SIZES = (1, 63, 64, 65, 257)
MARGINS = (0.0, 0.05)
MAX_CONTACTS = (1, 3, 5000)
TREES = ("empty", "root", "three_state", "mixed_depth4", "chain16", "block")


def _trees(pkg):
    return [(oc.empty_tree(pkg), 0.1, 3), (oc.tree_from_spec(pkg, oc.OCCUPIED), 0.1, 2), (oc.three_state_tree(pkg), 0.1, 2),
            (oc.random_tree(pkg, np.random.default_rng(41), 4), 0.1, 4), (oc.chain_tree(pkg, 16), 0.001, 16), (oc.block_tree(pkg), 0.1, 4)]


@pytest.fixture(scope="module")
def world(pkg, torch_cuda, tmp_path_factory):
    rng = np.random.default_rng(7)
    trees = _trees(pkg)
    assert int((~trees[3][0]["child"].any(axis=1)).sum()) == 67 and len(trees[5][0]) == 2 + 8 + 64 + 512
    L, solids = oc.seven_solids(pkg, rng)
    cover = L.add_box(2.0, 2.0, 0.1)  # a slab that covers the whole block (0.8 wide) one to two voxel layers thick
    lib = pkg.Library(L)
    for nodes, res, depth in trees:
        lib.add_octree(nodes, res, depth)
    assert lib.octree_count() == len(trees)
    yield dict(lib=lib, L=L, solids=solids, cover=cover, trees=trees, tables=oc.HarnessTrees(pkg, trees),
               harness=oc.build_harness(tmp_path_factory.mktemp("octree_harness")))
    lib.close()


def _queries(pkg, w, t, n):
    """n queries on tree t: solids near its reachable leaves (about half touching), every fifth far off; on the block every seventh is
    the covering slab, flat in the tree's frame"""
    geo = pkg.geometry
    rng = np.random.default_rng(1000 * t + n)
    _, shape, tft, tfs, swapped = oc.random_queries(pkg, rng, [w["trees"][t]], w["solids"], n, spread=0.25 if t != 4 else 0.05)
    far = np.arange(n) % 5 == 4
    if far.any():
        tfs[far] = geo.make_pose(quat=oc.random_rotations(rng, int(far.sum())), T=rng.uniform(30.0, 40.0, (int(far.sum()), 3)))
    if TREES[t] == "block" and n > 3:
        slab = np.arange(n) % 7 == 3
        shape[slab] = w["cover"]
        local = np.zeros((int(slab.sum()), 3))
        local[:, :2] = -0.4
        local[:, 2] = rng.uniform(-0.75, -0.05, int(slab.sum()))
        tfs[slab] = geo.compose(tft[slab], geo.make_pose(T=local))
    return np.full(n, t, dtype=np.uint32), shape, tft, tfs, swapped


def _device(torch, lib, pkg, ot, sh, tft, tfs, sw, req, cap):
    dev = torch.device("cuda:0")
    n = len(ot)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_ot, d_sh, d_tft, d_tfs, d_sw = t(ot.view(np.int32)), t(sh.view(np.int32)), t(tft), t(tfs), t(sw)
    d_out = torch.full((n * 96,), 0x5A, dtype=torch.uint8, device=dev)
    d_dlb = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    d_con = torch.full(((cap + 2) * 96,), 0x5A, dtype=torch.uint8, device=dev)  # (two guard records behind the capacity)
    nc = lib.octree_collide_device(d_ot, d_sh, d_tft, d_tfs, n, req, d_out, d_swapped=d_sw, d_bound=d_dlb, d_contacts=d_con, max_contacts=cap,
                                   want_count=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    con = d_con.cpu().numpy()
    assert (con[cap * 96:] == 0x5A).all(), "a contact was written past the capacity"
    return d_out.cpu().numpy().view(pkg.abi.RESULT_DTYPE), d_dlb.cpu().numpy(), con[:min(nc, cap) * 96].view(pkg.abi.CONTACT_DTYPE), nc


@pytest.mark.parametrize("t", range(len(TREES)), ids=TREES)
def test_device_equals_harness_and_host_equals_device(pkg, torch_cuda, world, t):
    lib, abi = world["lib"], pkg.abi
    seen_contacts = seen_dropped = seen_free = most_items = 0
    for k, n in enumerate(SIZES):
        req = abi.default_collision_request()
        req.security_margin = MARGINS[(k + t) % 2]
        req.num_max_contacts = MAX_CONTACTS[(k + t) % 3]
        ot, sh, tft, tfs, sw = _queries(pkg, world, t, n)
        want, want_dlb, want_con, want_nc, n_items = oc.harness_collide(pkg, world["harness"], world["tables"], world["L"], ot, sh, tft, tfs, req,
                                                                      sw, cap=1 << 16)
        assert want_nc <= 1 << 16
        what = "tree %s, %d queries, margin %g, num_max_contacts %d, %d items" % (TREES[t], n, req.security_margin, req.num_max_contacts, n_items)
        # a capacity below what is produced (where anything is): counted and dropped
        cap = want_nc // 2 if want_nc > 1 and k % 2 == 0 else want_nc
        # the device form: one chunk; chunks of 7 queries inside the call (the contact offsets and hfcl_contact::pair carried from chunk
        # to chunk); chunks cut down because they list more than 50 items (a chunk of one query is never cut)
        for chunk, items in ((0, 0), (7, 0), (0, 50)):
            lib.set_option("octree_chunk", chunk)
            lib.set_option("octree_items", items)
            got, dlb, con, nc = _device(torch_cuda, lib, pkg, ot, sh, tft, tfs, sw, req, cap)
            assert nc == want_nc, (what, chunk, items)
            assert oc.compare_records(got, want) == [], (what, chunk, items)
            assert dlb.tobytes() == want_dlb.tobytes(), (what, chunk, items)
            assert con.tobytes() == want_con[:cap].tobytes(), (what, chunk, items)
        lib.set_option("octree_items", 0)
        for chunk in (0, 7):  # the host form, whole and in chunks of 7 queries
            lib.set_option("octree_chunk", chunk)
            h_out, h_dlb, h_con, h_nc = lib.octree_collide(ot, sh, tft, tfs, req, swapped=sw, max_contacts=cap)
            assert h_nc == nc and h_out.tobytes() == got.tobytes() and h_dlb.tobytes() == dlb.tobytes() and h_con.tobytes() == con.tobytes(), what
        lib.set_option("octree_chunk", 0)
        seen_contacts += want_nc
        seen_dropped += want_nc - cap
        seen_free += int((want["num_contacts"] == 0).sum())
        most_items = max(most_items, n_items)
        assert (got["status"] & abi.STATUS_SWAPPED != 0).tolist() == sw.astype(bool).tolist()
        assert (got["b2"][got["num_contacts"] > 0] == -1).all() and (got["b1"][got["num_contacts"] > 0] >= 0).all()
    if TREES[t] == "empty":
        assert seen_contacts == 0 and most_items == 0
    else:
        assert seen_contacts > 0 and seen_dropped > 0 and seen_free > 0
    if TREES[t] == "block":
        assert most_items > 64 * 30  # the slabs: more items in a query than a workgroup has lanes


def test_contacts_are_the_per_pair_answers_of_the_leaves(pkg, torch_cuda):
    """Independent of the harness.  Resolution 0.25 and a tree pose that is a dyadic translation: every halving and every leaf pose is
    exact, a level's boxes are bit-equal cubes.  With num_max_contacts = 5000 the contacts of a query are the leaves, in toBoxes()
    order, whose per-pair record from hfcl_collide_batch (a library Box of that side at that pose, num_max_contacts = 1) has the contact
    flag: depth and normal bytes-equal, nearest points pos -+ depth * normal / 2 of that record; with num_max_contacts = 1 the record
    names the first such leaf."""
    abi, geo, fcl = pkg.abi, pkg.geometry, pkg.compat
    rng = np.random.default_rng(2)
    nodes = oc.random_tree(pkg, rng, 3)
    tree = fcl.OcTree(nodes, 0.25, 3)
    boxes = tree.toBoxes()
    leaves = [(i, lo, hi) for i, lo, hi in tree._leaves() if nodes[i]["occupancy"] >= 0.5]
    assert len(boxes) == len(leaves) >= 20 and set(boxes[:, 3]) <= {0.25, 0.5, 1.0} and len(set(boxes[:, 3])) >= 2
    for (i, lo, hi), b in zip(leaves, boxes):  # bit-equal cubes, centres exact
        assert (hi - lo == b[3]).all() and ((lo + hi) * 0.5 == b[:3]).all()
    L, solids = oc.seven_solids(pkg, rng, scale=2.0)
    side_id = {s: L.add_box(s, s, s) for s in (0.25, 0.5, 1.0)}
    lib = pkg.Library(L)
    tid = lib.add_octree(nodes, 0.25, 3)
    n = 70
    shift = np.array([0.5, -0.25, 0.125])
    tft = geo.make_pose(T=np.tile(shift, (n, 1)))
    sh = solids[np.arange(n) % 7]
    tfs = geo.make_pose(quat=oc.random_rotations(rng, n), T=rng.uniform(-1.1, 1.1, (n, 3)) + shift)
    m = len(boxes)
    s1 = np.tile(np.array([side_id[float(b[3])] for b in boxes], dtype=np.uint32), n)
    s2 = np.repeat(sh, m)
    tf1 = geo.make_pose(T=np.tile(boxes[:, :3] + shift, (n, 1)))
    tf2 = np.repeat(tfs.reshape(n, 12), m, axis=0)
    seen = 0
    for margin in MARGINS:
        req = abi.default_collision_request()
        req.security_margin = margin
        pair = lib.collide(s1, s2, tf1, tf2, req).reshape(n, m)
        flag = abi.status_contact(pair["status"]) != 0
        req.num_max_contacts = 5000
        rec, dlb, con, nc = lib.octree_collide(np.full(n, tid), sh, tft, tfs, req, max_contacts=n * m)
        assert nc == int(flag.sum()) == len(con) and (rec["num_contacts"] == flag.sum(axis=1)).all()
        at = 0
        for q in range(n):
            for j in np.flatnonzero(flag[q]):
                c, r = con[at], pair[q, j]
                at += 1
                assert c["pair"] == q and c["b1"] == leaves[j][0] and c["b2"] == -1
                assert np.float64(c["penetration_depth"]).tobytes() == np.float64(r["distance"]).tobytes()
                assert c["normal"].tobytes() == r["normal"].tobytes()
                pos, half = (r["p1"] + r["p2"]) / 2, r["distance"] * r["normal"] / 2
                assert c["p1"].tobytes() == (pos - half).tobytes() and c["p2"].tobytes() == (pos + half).tobytes()
        # the bound: no larger than any leaf's distance - margin
        assert (dlb <= (pair["distance"] - margin).min(axis=1)).all()
        req.num_max_contacts = 1
        rec1, _, con1, nc1 = lib.octree_collide(np.full(n, tid), sh, tft, tfs, req, max_contacts=n)
        hit = flag.any(axis=1)
        assert nc1 == int(hit.sum()) and (rec1["num_contacts"] == hit).all()
        first = [leaves[int(np.argmax(flag[q]))][0] for q in np.flatnonzero(hit)]
        assert rec1["b1"][hit].tolist() == first and (rec1["b1"][~hit] == -1).all()
        assert con1["b1"].tolist() == first
        seen += int(flag.sum())
    assert seen > 100
    assert np.array_equal(lib.octree_root_box(tid), [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    lib.close()


def test_solid_first_is_the_octree_first_result_plus_bit_23(pkg, torch_cuda, world):
    lib, abi = world["lib"], pkg.abi
    ot, sh, tft, tfs, _ = _queries(pkg, world, 3, 65)
    req = abi.default_collision_request()
    req.num_max_contacts = 3
    a, a_dlb, a_con, a_nc = lib.octree_collide(ot, sh, tft, tfs, req, swapped=np.zeros(65, dtype=np.uint8), max_contacts=256)
    b, b_dlb, b_con, b_nc = lib.octree_collide(ot, sh, tft, tfs, req, swapped=np.ones(65, dtype=np.uint8), max_contacts=256)
    c = lib.octree_collide(ot, sh, tft, tfs, req, max_contacts=256)[0]  # (swapped: NULL)
    assert a_nc == b_nc > 0 and a_con.tobytes() == b_con.tobytes() and a_dlb.tobytes() == b_dlb.tobytes() and a.tobytes() == c.tobytes()
    assert oc.compare_records(a, b) == ["status"] and (b["status"] == a["status"] | abi.STATUS_SWAPPED).all() and (a["status"] & abi.STATUS_SWAPPED == 0).all()


def test_thresholds_changed_by_the_setter_change_the_answer(pkg, torch_cuda):
    abi, geo = pkg.abi, pkg.geometry
    L = geo.ShapeLibrary()
    ball = L.add_sphere(0.05)
    lib = pkg.Library(L)
    tid = lib.add_octree(oc.three_state_tree(pkg), 0.1, 2)  # child 1 of the root, node 2: an uncertain leaf (0.3) at x in [0, 0.2], y, z in [-0.2, 0]
    at = geo.make_pose(T=np.array([[0.1, -0.1, -0.1]]))
    tf = geo.make_pose().reshape(1, 12)
    assert lib.octree_collide([tid], [ball], tf, at)[0]["num_contacts"][0] == 0
    lib.octree_set_thresholds(tid, 0.25, 0.0)
    rec = lib.octree_collide([tid], [ball], tf, at)[0]
    assert rec["num_contacts"][0] == 1 and rec["b1"][0] == 2
    lib.octree_set_thresholds(tid, 0.25, 0.3)  # free: occupancy <= free_threshold
    assert lib.octree_collide([tid], [ball], tf, at)[0]["num_contacts"][0] == 0
    lib.octree_set_thresholds(tid, 0.5, 0.0)
    assert lib.octree_collide([tid], [ball], tf, at)[0]["num_contacts"][0] == 0
    with pytest.raises(pkg.engine.EngineError):
        lib.octree_set_thresholds(tid + 1, 0.5, 0.0)
    # clear: indices start over
    lib.clear_octrees()
    assert lib.octree_count() == 0
    with pytest.raises(pkg.engine.EngineError):
        lib.octree_collide([0], [ball], tf, at)
    assert lib.add_octree(oc.tree_from_spec(pkg, oc.OCCUPIED), 0.1, 2) == 0
    assert lib.octree_collide([0], [ball], tf, at)[0]["num_contacts"][0] == 1
    lib.close()


def test_requests_refused_before_any_output(pkg, torch_cuda, world):
    lib, abi, torch = world["lib"], pkg.abi, torch_cuda
    ot, sh, tft, tfs, sw = _queries(pkg, world, 3, 6)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_in = (t(ot.view(np.int32)), t(sh.view(np.int32)), t(tft), t(tfs))

    def code(**kw):
        req = abi.default_collision_request()
        for k, v in kw.items():
            setattr(req.q if hasattr(req.q, k) else req, k, v)
        out = np.full(6 * 96, 0x5A, dtype=np.uint8).view(abi.RESULT_DTYPE)
        codes = []
        try:
            import ctypes as C
            dlb, nc = np.full(6, -7.0), C.c_size_t(77)
            rc = pkg.engine.dll().hfcl_octree_collide_batch(lib._h, abi.ptr(ot), abi.ptr(sh), abi.ptr(np.ascontiguousarray(tft).reshape(-1, 12)),
                                                            abi.ptr(np.ascontiguousarray(tfs).reshape(-1, 12)), C.c_size_t(6), None, C.byref(req),
                                                            abi.ptr(out), abi.ptr(dlb), None, C.c_size_t(0), C.byref(nc))
            codes.append(rc)
            if rc:
                assert (out.view(np.uint8) == 0x5A).all() and (dlb == -7.0).all() and nc.value == 77, kw
            d_out = torch.full((6 * 96,), 0x5A, dtype=torch.uint8, device=dev)
            try:
                lib.octree_collide_device(*d_in, 6, req, d_out, want_count=True)
                codes.append(abi.OK)
            except pkg.engine.EngineError as e:
                codes.append(e.code)
                torch.cuda.synchronize()
                assert (d_out.cpu().numpy() == 0x5A).all(), kw
        finally:
            torch.cuda.synchronize()
        assert codes[0] == codes[1], (kw, codes)
        return codes[0]

    assert code() == abi.OK
    assert code(num_max_contacts=0) == abi.ERR_INVALID_ARGUMENT
    assert code(security_margin=-0.01) == abi.ERR_INVALID_ARGUMENT
    assert code(epa_max_iterations=65) == abi.ERR_LIMIT
    assert code(gjk_initial_guess=abi.CachedGuess) == abi.ERR_LIMIT
    assert code(gjk_initial_guess=abi.BoundingVolumeGuess) == abi.ERR_LIMIT
    assert code(distance_upper_bound=1.0) == abi.ERR_LIMIT
    # -inf margin: every record skipped
    req = abi.default_collision_request()
    req.security_margin = -np.inf
    out, dlb, con, nc = lib.octree_collide(ot, sh, tft, tfs, req, swapped=sw, max_contacts=4)
    assert nc == 0 and (abi.status_skipped(out["status"]) == 1).all() and (dlb == np.finfo(np.float64).max).all()
    # a solid without an evaluator, a tree that is not there: refused by the host form, skipped records from the device form
    L2 = pkg.geometry.ShapeLibrary()
    L2.add_sphere(0.2)
    L2.add_halfspace((0, 0, 1), 0.0)
    lib2 = pkg.Library(L2)
    lib2.add_octree(oc.tree_from_spec(pkg, oc.OCCUPIED), 0.1, 2)
    tf = pkg.geometry.make_pose().reshape(1, 12)
    for ids, want in ((([0], [1]), abi.ERR_UNSUPPORTED_PAIR), (([1], [0]), abi.ERR_INVALID_ARGUMENT)):
        with pytest.raises(pkg.engine.EngineError) as e:
            lib2.octree_collide(ids[0], ids[1], tf, tf)
        assert e.value.code == want
    d_ids = t(np.array([0, 0, 1], dtype=np.int32)), t(np.array([0, 1, 0], dtype=np.int32))
    d_tf = t(np.repeat(tf, 3, axis=0))
    d_out = torch.full((3 * 96,), 0x5A, dtype=torch.uint8, device=dev)
    assert lib2.octree_collide_device(d_ids[0], d_ids[1], d_tf, d_tf, 3, abi.default_collision_request(), d_out, want_count=True) == 1
    got = d_out.cpu().numpy().view(abi.RESULT_DTYPE)
    assert abi.status_skipped(got["status"]).tolist() == [0, 1, 1] and got["num_contacts"].tolist() == [1, 0, 0]
    lib2.close()


def _shim_cases(pkg, nodes, rng, n):
    """queries of tests/cpp/test_octree.cpp's input: (kind, a, b, c, tf_tree, tf_solid, swapped, margin, num_max_contacts)"""
    geo = pkg.geometry
    boxes = oc.leaf_boxes(nodes, 0.1, 4)
    cases = []
    for i in range(n):
        kind = i % 6
        a, b, c = rng.uniform(0.05, 0.2, 3)
        tft = geo.make_pose(quat=oc.random_rotations(rng, 1)[0], T=rng.uniform(-1.0, 1.0, 3)) if i % 3 else geo.make_pose()
        _, lo, hi = boxes[int(rng.integers(0, len(boxes)))]
        local = 0.5 * (np.array(lo) + np.array(hi)) + rng.uniform(-0.15, 0.15, 3)
        tfs = geo.make_pose(quat=oc.random_rotations(rng, 1)[0], T=geo.transform_point(tft.reshape(1, 12), local.reshape(1, 3))[0])
        cases.append((kind, float(a), float(b), float(c), np.asarray(tft).ravel(), np.asarray(tfs).ravel(), i % 2, (0.0, 0.05)[(i // 2) % 2],
                      (1, 3, 5000)[i % 3]))
    return cases


def test_compat_and_cpp_shim_agree(pkg, torch_cuda, tmp_path):
    fcl = pkg.compat
    nodes = oc.random_tree(pkg, np.random.default_rng(41), 4)
    cases = _shim_cases(pkg, nodes, np.random.default_rng(9), 24)
    tree = fcl.OcTree(nodes, 0.1, 4)
    lines_want, hits = [], 0
    for kind, a, b, c, tft, tfs, swapped, margin, nmax in cases:
        solid = (fcl.Box(a, b, c), fcl.Sphere(a), fcl.Capsule(a, b), fcl.Cylinder(a, b), fcl.Cone(a, b), fcl.Ellipsoid(a, b, c))[kind]
        tf_t = fcl.Transform3f(tft[:9].reshape(3, 3).T, tft[9:])
        tf_s = fcl.Transform3f(tfs[:9].reshape(3, 3).T, tfs[9:])
        req, res = fcl.CollisionRequest(), fcl.CollisionResult()
        req.security_margin, req.num_max_contacts = margin, nmax
        if swapped:
            fcl.collide(solid, tf_s, tree, tf_t, req, res)
        else:
            fcl.ComputeCollision(tree, solid)(tf_t, tf_s, req, res)
        words = [str(res.numContacts()), float(res.distance_lower_bound).hex()]
        for k in range(res.numContacts()):
            ct = res.getContact(k)
            assert ct.o1 is tree and ct.o2 is solid and ct.b2 == -1
            words += [str(int(ct.b1)), str(int(ct.b2)), float(ct.penetration_depth).hex()]
            words += [float(x).hex() for x in list(ct.normal) + list(ct.getNearestPoint1()) + list(ct.getNearestPoint2())]
        hits += res.numContacts() > 0
        lines_want.append(words)
    assert 4 < hits < len(cases)
    with pytest.raises(ValueError):
        fcl.collide(tree, fcl.Transform3f(), fcl.Halfspace((0, 0, 1), 0.0), fcl.Transform3f(), fcl.CollisionRequest(), fcl.CollisionResult())
    neg = fcl.CollisionRequest()
    neg.security_margin = -0.01
    with pytest.raises(ValueError):
        fcl.collide(tree, fcl.Transform3f(), fcl.Sphere(0.1), fcl.Transform3f(), neg, fcl.CollisionResult())
    # setOccupancyThres reaches the library: nothing is occupied at 0.99
    tree.setOccupancyThres(0.99)
    res = fcl.CollisionResult()
    fcl.collide(tree, fcl.Transform3f(), fcl.Sphere(5.0), fcl.Transform3f(), fcl.CollisionRequest(), res)
    assert not res.isCollision() and len(tree.toBoxes()) == 0
    tree.setOccupancyThres(0.5)
    res = fcl.CollisionResult()
    fcl.collide(tree, fcl.Transform3f(), fcl.Sphere(5.0), fcl.Transform3f(), fcl.CollisionRequest(), res)
    assert res.isCollision()
    made = fcl.makeOctree(np.array([[0.1, 0.1, 0.1], [0.1, 0.1, 0.1], [-0.6, 0.3, 0.2]]), 0.25)
    assert made.getTreeDepth() == 16 and made.getResolution() == 0.25 and len(made.toBoxes()) == 2 and made.size() == 1 + 16 + 16
    assert np.array_equal(made.getRootBV(), [-8192.0] * 3 + [8192.0] * 3)

    # the same cases through the C++ shim
    exe = str(tmp_path / "test_octree")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_octree.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("%r 4 %d %d\n" % (0.1, len(nodes), len(cases)))
        for nd in nodes:
            f.write(" ".join(str(int(c)) for c in nd["child"]) + " %r\n" % float(nd["occupancy"]))
        for kind, a, b, c, tft, tfs, swapped, margin, nmax in cases:
            f.write("%d %r %r %r " % (kind, a, b, c) + " ".join(repr(float(x)) for x in list(tft) + list(tfs)) + " %d %r %d\n" % (swapped, margin, nmax))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert out[0].split()[0] == "root" and float.fromhex(out[0].split()[1]) == -0.8 and int(out[0].split()[4]) == len(fcl.OcTree(nodes, 0.1, 4).toBoxes())
    for want, line in zip(lines_want, out[1:1 + len(cases)]):
        got = line.split()
        assert got[0] == want[0] and len(got) == len(want), (got, want)
        for g, w in zip(got[1:], want[1:]):
            assert (int(g) == int(w)) if "x" not in w and "n" not in w else (float.fromhex(g) == float.fromhex(w) or (g == w)), (got, want)
    assert "tree first: ok" in r.stdout and "halfspace and negative margin refused" in r.stdout and "makeOctree 33 nodes 2 boxes depth 16" in r.stdout
