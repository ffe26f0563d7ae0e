"""OcTree x convex solid distance() (include/hppfcl_amd_octree_distance.h) on the GPU.  The yardstick is the host build of the device
header (tests/octree_distance_harness, held against the fp64 model in tests/test_octree_distance_cpu.py): records and visited counts of
the device call equal the harness's byte for byte, the host call equals the device call, for three values of the chunk option.
Independent of the harness, on trees whose halvings are exact: the reported leaf's record is the per-pair distance() of this library on
that leaf's Box, and the answer is the ordered walk's -- never below the brute-force minimum over the per-pair records of every
reachable leaf, equal to it for six kinds, above it for some Ellipsoids.

Trees, the smallest on which each piece can go wrong: the empty tree, the root alone, the three-state tree; one chain down to a voxel at
level 16 (the stack at its depth); a full 8 x 8 x 8 block (every lane of the child step is live); three random trees of depth 3 - 5.
Batches of 1, 3 and 5 queries (fewer than a workgroup's four groups) and 257 (the last workgroup partly filled)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import octree_cases as oc
import octree_distance_cases as odc
import octree_distance_model as odm

pytestmark = pytest.mark.gpu
ROOT = oc.ROOT
N = 257
ELLIPSOID = 19
SETS = {"hand_made": (0, 1, 2), "chain16": (3,), "block": (4,), "random": (5, 6, 7)}
DYADIC = 0.25  # a resolution whose halvings, centres and half sides are exact


def _trees(pkg):
    rng = np.random.default_rng(41)
    return [(oc.empty_tree(pkg), 0.1, 3), (oc.tree_from_spec(pkg, oc.OCCUPIED), 0.1, 2), (oc.three_state_tree(pkg), 0.1, 2),
            (oc.chain_tree(pkg, 16), 0.001, 16), (oc.block_tree(pkg), 0.1, 4), (oc.random_tree(pkg, rng, 3), 0.1, 3),
            (oc.random_tree(pkg, rng, 4), 0.1, 4), (oc.random_tree(pkg, rng, 5, p_child=0.35), 0.1, 5, 0.75, 0.1)]


def _big_hull(rng, n=40, r=0.12):
    """more vertices than HULL_MAX (32): the group's support takes the scan path"""
    p = rng.normal(size=(n, 3))
    return r * p / np.linalg.norm(p, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def world(pkg, torch_cuda, tmp_path_factory):
    rng = np.random.default_rng(7)
    trees = _trees(pkg)
    L, solids = oc.seven_solids(pkg, rng)
    big = L.add_convex(_big_hull(rng))
    assert L.shapes_array()["num_points"][big] == 40
    solids = np.append(solids, np.uint32(big))
    lib = pkg.Library(L)
    for t in trees:
        lib.add_octree(*t)
    yield dict(lib=lib, L=L, solids=solids, big=big, trees=trees, tables=oc.HarnessTrees(pkg, trees),
               harness=odc.build_harness(tmp_path_factory.mktemp("octree_distance_harness")))
    lib.close()


def _queries(pkg, w, ids, n, seed, spread):
    rng = np.random.default_rng(seed)
    sub = [w["trees"][t] for t in ids]
    ot, sh, tft, tfs, sw = oc.random_queries(pkg, rng, sub, w["solids"], n, spread=spread)
    return np.array(ids, dtype=np.uint32)[ot], sh, tft, tfs, sw


def _device(torch, lib, pkg, ot, sh, tft, tfs, sw, req, visited=True):
    dev = torch.device("cuda:0")
    n = len(ot)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_ot, d_sh, d_tft, d_tfs = t(ot.view(np.int32)), t(sh.view(np.int32)), t(tft), t(tfs)
    d_sw = t(sw) if sw is not None else None
    d_out = torch.full(((n + 1) * 96,), 0x5A, dtype=torch.uint8, device=dev)  # (a guard record behind the batch)
    d_vis = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    lib.octree_distance_device(d_ot, d_sh, d_tft, d_tfs, n, req, d_out, d_swapped=d_sw, d_visited=d_vis if visited else None,
                               stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, vis = d_out.cpu().numpy(), d_vis.cpu().numpy().view(np.uint32)
    assert (out[n * 96:] == 0x5A).all() and vis[n] == 0x5A5A5A5A, "written past the batch"
    return out[:n * 96].view(pkg.abi.RESULT_DTYPE), vis[:n]


# ---- 1. device equals harness, host equals device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_device_equals_harness_and_host_equals_device(pkg, torch_cuda, world, name):
    lib, abi = world["lib"], pkg.abi
    ids = SETS[name]
    solved = convex_big = 0
    for k, n in enumerate((1, 3, 5, N)):
        req = odc.request(abi, signed=(k != 2))
        ot, sh, tft, tfs, sw = _queries(pkg, world, ids, n, 100 * len(name) + n, spread=0.25 if name != "chain16" else 0.05)
        if n == N:
            sh[::9] = world["big"]
        want, want_vis = odc.harness_distance(pkg, world["harness"], world["tables"], world["L"], ot, sh, tft, tfs, req, sw)
        what = "trees %s, %d queries, signed %d" % (name, n, req.enable_signed_distance)
        try:
            for chunk in (0, 1, 7):
                lib.set_option("octree_chunk", chunk)
                got, vis = _device(torch_cuda, lib, pkg, ot, sh, tft, tfs, sw, req)
                assert oc.compare_records(got, want) == [], (what, chunk)
                assert vis.tobytes() == want_vis.tobytes(), (what, chunk)
                h_out, h_vis = lib.octree_distance(ot, sh, tft, tfs, req, swapped=sw, want_visited=True)
                assert h_out.tobytes() == got.tobytes() and h_vis.tobytes() == vis.tobytes(), (what, chunk)
        finally:
            lib.set_option("octree_chunk", 0)
        no_vis, _ = _device(torch_cuda, lib, pkg, ot, sh, tft, tfs, None, req, visited=False)  # (n_visited and swapped: NULL)
        assert oc.compare_records(no_vis, want) in ([], ["status"]) and (no_vis["status"] & abi.STATUS_SWAPPED == 0).all()
        assert (got["status"] & abi.STATUS_SWAPPED != 0).tolist() == sw.astype(bool).tolist()
        assert (got["b2"] == -1).all() and (got["num_contacts"] == 0).all() and ((got["b1"] >= 0) == (vis > 0)).all()
        solved += int(vis.sum())
        convex_big += int((sh == world["big"]).sum())
    empty = ot == 0
    if name == "hand_made":
        assert empty.any() and (got["distance"][empty] == np.finfo(np.float64).max).all() and (vis[empty] == 0).all()
        assert np.isnan(got["p1"][empty]).all() and (got["b1"][empty] == -1).all()
    assert solved >= N // 2 and convex_big > 20
    if name in ("block", "random"):
        assert vis.max() > 16


# ---- the dyadic world of tests 2 and 3 --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dyadic(pkg, torch_cuda):
    """Resolution 0.25 and tree poses that are dyadic translations: every halving and every leaf pose is exact, so the explicit Box of a
    leaf (a library Box of that side at tf_tree * center) is the box the walk solves, bit for bit."""
    geo = pkg.geometry
    rng = np.random.default_rng(13)
    trees = [(oc.random_tree(pkg, rng, 3), DYADIC, 3), (oc.random_tree(pkg, rng, 4), DYADIC, 4), (oc.block_tree(pkg), DYADIC, 4)]
    L, solids = oc.seven_solids(pkg, rng, scale=2.5)
    sides = sorted({float(hi[0] - lo[0]) for t in trees for _, lo, hi in oc.leaf_boxes(*t)})
    side_id = {s: L.add_box(s, s, s) for s in sides}
    lib = pkg.Library(L)
    for t in trees:
        lib.add_octree(*t)
    leaves = [oc.leaf_boxes(*t) for t in trees]
    for lv in leaves:
        for _, lo, hi in lv:
            assert len({hi[a] - lo[a] for a in range(3)}) == 1
    # queries: the solids of random_queries, the tree poses replaced by dyadic translations (the solids move along)
    ot, sh, tft, tfs, sw = oc.random_queries(pkg, rng, trees, solids, N, spread=1.2, identity_share=1.0)
    shift = np.round(rng.uniform(-2.0, 2.0, (N, 3)) * 8) / 8
    tft = geo.make_pose(T=shift)
    tfs = np.array(tfs, dtype=np.float64).reshape(N, 12).copy()
    tfs[:, 9:12] += shift
    req = odc.request(pkg.abi, True)
    rec, vis = lib.octree_distance(ot, sh, tft, tfs, req, swapped=sw, want_visited=True)
    yield dict(lib=lib, L=L, trees=trees, leaves=leaves, side_id=side_id, ot=ot, sh=sh, tft=np.asarray(tft).reshape(N, 12), tfs=tfs, sw=sw, req=req,
               rec=rec, vis=vis, shift=shift)
    lib.close()


def _per_pair(torch, pkg, lib, s1, s2, tf1, tf2, req):
    """hfcl_distance_batch_device"""
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    n = len(s1)
    d_out = torch.zeros((n * 96,), dtype=torch.uint8, device=dev)
    lib.distance_device(t(s1.view(np.int32)), t(s2.view(np.int32)), t(tf1), t(tf2), n, req, d_out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(pkg.abi.RESULT_DTYPE)


# ---- 2. the per-pair answer of the reported leaf ----------------------------------------------------------------------------------------
def test_record_is_the_per_pair_answer_of_the_reported_leaf(pkg, torch_cuda, dyadic):
    w, geo = dyadic, pkg.geometry
    rec = w["rec"]
    hit = np.flatnonzero(rec["b1"] >= 0)
    assert len(hit) > 0.8 * N
    s1, centers = [], []
    for i in hit:
        box = {node: (lo, hi) for node, lo, hi in w["leaves"][int(w["ot"][i])]}
        lo, hi = box[int(rec["b1"][i])]
        s1.append(w["side_id"][float(hi[0] - lo[0])])
        centers.append(0.5 * (np.array(lo) + np.array(hi)) + w["shift"][i])
    pair = _per_pair(torch_cuda, pkg, w["lib"], np.array(s1, dtype=np.uint32), w["sh"][hit], np.asarray(geo.make_pose(T=np.array(centers))).reshape(-1, 12),
                     w["tfs"][hit], w["req"])
    for k in ("distance", "p1", "p2", "normal"):
        assert rec[k][hit].tobytes() == pair[k].tobytes(), k
    assert (rec["distance"][hit] > 0).sum() > 50 and (rec["distance"][hit] <= 0).sum() > 20


# ---- 3. the ordered walk on the device records ------------------------------------------------------------------------------------------
def test_the_ordered_walk_is_what_the_device_answers(pkg, torch_cuda, dyadic):
    """The brute force: hfcl_distance_batch_device over every reachable leaf of every query.  For every separated query the record's
    distance >= the brute-force minimum (exact: the minimum over a subset of the same numbers); equal, with the DFS-first minimal leaf
    as b1, for every kind but Ellipsoid; strictly greater in at least one Ellipsoid query."""
    w, geo = dyadic, pkg.geometry
    rec = w["rec"]
    types = w["L"].shapes_array()["type"]
    s1, s2, c, tf2, owner = [], [], [], [], []
    for i in range(N):
        for node, lo, hi in w["leaves"][int(w["ot"][i])]:
            s1.append(w["side_id"][float(hi[0] - lo[0])])
            c.append(0.5 * (np.array(lo) + np.array(hi)) + w["shift"][i])
            owner.append(i)
    owner = np.array(owner)
    assert 10000 < len(owner) < 300000
    pair = _per_pair(torch_cuda, pkg, w["lib"], np.array(s1, dtype=np.uint32), w["sh"][owner], np.asarray(geo.make_pose(T=np.array(c))).reshape(-1, 12),
                     w["tfs"][owner], w["req"])
    separated = above = shares = 0
    start = np.searchsorted(owner, np.arange(N + 1))
    for i in range(N):
        d = pair["distance"][start[i]:start[i + 1]]
        m = d.min()
        if not m > 0:
            assert rec["distance"][i] <= 0 or types[w["sh"][i]] == ELLIPSOID, i  # (the Ellipsoid's box can hide a penetrated leaf too)
            continue
        separated += 1
        shares += w["vis"][i] / len(d)
        assert rec["distance"][i] >= m, i
        if types[w["sh"][i]] != ELLIPSOID:
            assert rec["distance"][i] == m and rec["b1"][i] == w["leaves"][int(w["ot"][i])][int(np.argmin(d))][0], i
        elif rec["distance"][i] > m:
            above += 1
    print("separated %d of %d, Ellipsoid queries above the brute-force minimum %d, mean visited share %.3f" % (separated, N, above, shares / separated))
    assert separated > N // 4 and above >= 1


# ---- 4. operand order -------------------------------------------------------------------------------------------------------------------------
def test_solid_first_is_the_octree_first_result_plus_bit_23(pkg, torch_cuda, world):
    lib, abi = world["lib"], pkg.abi
    ot, sh, tft, tfs, _ = _queries(pkg, world, SETS["random"], N, 5, 0.5)
    a, a_vis = lib.octree_distance(ot, sh, tft, tfs, swapped=np.zeros(N, dtype=np.uint8), want_visited=True)
    b, b_vis = lib.octree_distance(ot, sh, tft, tfs, swapped=np.ones(N, dtype=np.uint8), want_visited=True)
    c = lib.octree_distance(ot, sh, tft, tfs)  # (swapped: NULL)
    assert a.tobytes() == c.tobytes() and a_vis.tobytes() == b_vis.tobytes()
    assert oc.compare_records(a, b) == ["status"] and (b["status"] == a["status"] | abi.STATUS_SWAPPED).all() and (a["status"] & abi.STATUS_SWAPPED == 0).all()
    assert (a["distance"] > 0).any() and (a["distance"] <= 0).any()


# ---- 5. thresholds ------------------------------------------------------------------------------------------------------------------------------
def test_thresholds_changed_by_the_setter_change_the_answer(pkg, torch_cuda):
    abi, geo = pkg.abi, pkg.geometry
    rng = np.random.default_rng(3)
    L, solids = oc.seven_solids(pkg, rng)
    ball = L.add_sphere(0.05)
    lib = pkg.Library(L)
    nodes = oc.three_state_tree(pkg)
    tid = lib.add_octree(nodes, 0.1, 2)  # node 2: an uncertain leaf (0.3) at x in [0, 0.2], y, z in [-0.2, 0]
    ot, sh, tft, tfs, sw = oc.random_queries(pkg, rng, [(nodes, 0.1, 2)], solids, N, spread=0.3)
    tfs = np.asarray(tfs).reshape(N, 12).copy()
    tft = np.asarray(tft).reshape(N, 12).copy()
    sh[0], tft[0], tfs[0] = ball, geo.make_pose().reshape(12), geo.make_pose(T=np.array([[0.1, -0.1, -0.1]])).reshape(12)  # inside node 2
    req = odc.request(abi, True)
    seen_node2 = []
    for occ, free in ((0.5, 0.0), (0.25, 0.0), (0.25, 0.3), (0.9, 0.0)):
        lib.octree_set_thresholds(tid, occ, free)
        rec, vis = lib.octree_distance(ot, sh, tft, tfs, req, swapped=sw, want_visited=True)
        recs, visited, near, _ = odm.distance([odm.Tree(nodes, 0.1, 2, occ, free)], ot, L.shapes_array(), L.vertices_array(), sh, tft, tfs, req, sw)
        keep = ~np.array(near)
        assert keep.sum() > 0.95 * N
        assert rec["b1"][keep].tolist() == [r["b1"] for r, k in zip(recs, keep) if k] and vis[keep].tolist() == [v for v, k in zip(visited, keep) if k]
        assert np.allclose(rec["distance"][keep], [r["distance"] for r, k in zip(recs, keep) if k], rtol=0, atol=1e-12)
        seen_node2.append(bool((rec["b1"] == 2).any()))
        # collide sees the same registration
        con = lib.octree_collide([tid], [ball], tft[:1], tfs[:1])[0]
        assert (con["num_contacts"][0] == 1 and con["b1"][0] == 2) == (occ <= 0.3 and free < 0.3), (occ, free)
        assert (rec["b1"][0] == 2 and rec["distance"][0] < 0) == (occ <= 0.3), (occ, free)  # (distance() does not read free_threshold)
    assert seen_node2 == [False, True, True, False]
    lib.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_requests_refused_before_any_output(pkg, torch_cuda, world):
    lib, abi, torch = world["lib"], pkg.abi, torch_cuda
    d = pkg.engine.dll()
    ot, sh, tft, tfs, sw = _queries(pkg, world, SETS["random"], 6, 9, 0.3)
    tft, tfs = np.ascontiguousarray(tft).reshape(-1, 12), np.ascontiguousarray(tfs).reshape(-1, 12)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_in = (t(ot.view(np.int32)), t(sh.view(np.int32)), t(tft), t(tfs))

    def host(h, req, ot=ot, sh=sh):
        out = np.full(6 * 96, 0x5A, dtype=np.uint8)
        vis = np.full(6, 0x5A5A5A5A, dtype=np.uint32)
        rc = d.hfcl_octree_distance_batch(h, abi.ptr(ot), abi.ptr(sh), abi.ptr(tft), abi.ptr(tfs), C.c_size_t(6), None,
                                          C.byref(req) if req is not None else None, abi.ptr(out), abi.ptr(vis))
        if rc:
            assert (out == 0x5A).all() and (vis == 0x5A5A5A5A).all(), "output touched by a refused call"
        return rc

    def device(h, req):
        d_out = torch.full((6 * 96,), 0x5A, dtype=torch.uint8, device=dev)
        d_vis = torch.full((6,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        rc = d.hfcl_octree_distance_batch_device(h, *[C.c_void_p(x.data_ptr()) for x in d_in], C.c_size_t(6), None,
                                                 C.byref(req) if req is not None else None, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_vis.data_ptr()),
                                                 None)
        torch.cuda.synchronize()
        if rc:
            assert (d_out.cpu().numpy() == 0x5A).all() and (d_vis.cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all(), "output touched by a refused call"
        return rc

    def code(**kw):
        req = abi.default_distance_request()
        for k, v in kw.items():
            setattr(req.q if hasattr(req.q, k) else req, k, v)
        codes = (host(lib._h, req), device(lib._h, req))
        assert codes[0] == codes[1], (kw, codes)
        return codes[0]

    assert code() == abi.OK
    assert code(rel_err=0.5, abs_err=0.5, enable_nearest_points=0) == abi.OK  # not read
    assert code(gjk_initial_guess=abi.CachedGuess) == abi.ERR_LIMIT
    assert code(gjk_initial_guess=abi.BoundingVolumeGuess) == abi.ERR_LIMIT
    assert code(epa_max_iterations=65) == abi.ERR_LIMIT
    assert code(epa_max_iterations=64) == abi.OK
    req = abi.default_distance_request()
    assert host(None, req) == device(None, req) == abi.ERR_INVALID_ARGUMENT and "null library" in pkg.engine.last_error()
    assert host(lib._h, None) == device(lib._h, None) == abi.ERR_INVALID_ARGUMENT and "null request" in pkg.engine.last_error()
    null_rc = d.hfcl_distance_batch(lib._h, abi.ptr(sh), abi.ptr(sh), abi.ptr(tft), abi.ptr(tfs), C.c_size_t(6), None, abi.ptr(np.zeros(6, dtype=abi.RESULT_DTYPE)),
                                    None, None)
    assert null_rc == abi.ERR_INVALID_ARGUMENT  # ... as the other calls handle it
    # the host form: ids outside the library, a solid without an evaluator
    bad = ot.copy()
    bad[3] = len(world["trees"])
    assert host(lib._h, req, ot=bad) == abi.ERR_INVALID_ARGUMENT
    bad = sh.copy()
    bad[5] = len(world["L"].shapes_array())
    assert host(lib._h, req, sh=bad) == abi.ERR_INVALID_ARGUMENT
    L2 = pkg.geometry.ShapeLibrary()
    L2.add_sphere(0.2)
    L2.add_halfspace((0, 0, 1), 0.0)
    lib2 = pkg.Library(L2)
    lib2.add_octree(oc.tree_from_spec(pkg, oc.OCCUPIED), 0.1, 2)
    tf = pkg.geometry.make_pose().reshape(1, 12)
    for ids, want in ((([0], [1]), abi.ERR_UNSUPPORTED_PAIR), (([1], [0]), abi.ERR_INVALID_ARGUMENT)):
        with pytest.raises(pkg.engine.EngineError) as e:
            lib2.octree_distance(ids[0], ids[1], tf, tf)
        assert e.value.code == want
    # the device form cannot see the ids: skipped records and HFCL_OK
    d_ids = t(np.array([0, 0, 1], dtype=np.int32)), t(np.array([0, 1, 0], dtype=np.int32))
    d_tf = t(np.repeat(tf, 3, axis=0))
    d_out = torch.full((3 * 96,), 0x5A, dtype=torch.uint8, device=dev)
    d_vis = torch.full((3,), 7, dtype=torch.int32, device=dev)
    d_sw = t(np.array([0, 1, 0], dtype=np.uint8))
    lib2.octree_distance_device(d_ids[0], d_ids[1], d_tf, d_tf, 3, abi.default_distance_request(), d_out, d_swapped=d_sw, d_visited=d_vis)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(abi.RESULT_DTYPE)
    assert abi.status_skipped(got["status"]).tolist() == [0, 1, 1] and d_vis.cpu().numpy().tolist() == [1, 0, 0]
    assert got["status"][1] == 0x80000000 | abi.STATUS_SWAPPED and got["status"][2] == 0x80000000 and got["distance"][1] == 0 and got["b1"][1] == 0
    assert got["distance"][0] < 0 and got["b1"][0] == 0  # the sphere at the centre of the voxel
    lib2.close()


# ---- 7. the shims ----------------------------------------------------------------------------------------------------------------------------
def test_compat_and_cpp_shim_agree_with_the_engine(pkg, torch_cuda, tmp_path):
    fcl, geo, abi = pkg.compat, pkg.geometry, pkg.abi
    nodes = oc.random_tree(pkg, np.random.default_rng(41), 4)
    rng = np.random.default_rng(9)
    boxes = oc.leaf_boxes(nodes, 0.1, 4)
    tree = fcl.OcTree(nodes, 0.1, 4)
    cases = []
    for i in range(12):
        kind = i % 6
        a, b, c = (float(x) for x in rng.uniform(0.05, 0.2, 3))
        tft = geo.make_pose(quat=oc.random_rotations(rng, 1)[0], T=rng.uniform(-1.0, 1.0, 3)) if i % 3 else geo.make_pose()
        _, lo, hi = boxes[int(rng.integers(0, len(boxes)))]
        local = 0.5 * (np.array(lo) + np.array(hi)) + rng.uniform(-0.4, 0.4, 3)
        tfs = geo.make_pose(quat=oc.random_rotations(rng, 1)[0], T=geo.transform_point(tft.reshape(1, 12), local.reshape(1, 3))[0])
        cases.append((kind, a, b, c, np.asarray(tft).ravel(), np.asarray(tfs).ravel(), i % 2, 1 if i % 4 < 3 else 0))
    lines_want, separated = [], 0
    for i, (kind, a, b, c, tft, tfs, swapped, signed) in enumerate(cases):
        solid = (fcl.Box(a, b, c), fcl.Sphere(a), fcl.Capsule(a, b), fcl.Cylinder(a, b), fcl.Cone(a, b), fcl.Ellipsoid(a, b, c))[kind]
        tf_t = fcl.Transform3f(tft[:9].reshape(3, 3).T, tft[9:])
        tf_s = fcl.Transform3f(tfs[:9].reshape(3, 3).T, tfs[9:])
        req, res = fcl.DistanceRequest(), fcl.DistanceResult()
        req.enable_signed_distance = bool(signed)
        d = fcl.distance(solid, tf_s, tree, tf_t, req, res) if swapped else fcl.ComputeDistance(tree, solid)(tf_t, tf_s, req, res)
        # the engine call on the shim's own library
        ctx = fcl._context()
        sid, tid = ctx.add(solid), ctx.add_octree(tree)
        r = ctx.library().octree_distance([tid], [sid], tft.reshape(1, 12), tfs.reshape(1, 12), odc.request(abi, bool(signed)), swapped=[swapped])[0]
        assert bool(r["status"] & abi.STATUS_SWAPPED) == bool(swapped)
        assert res.o1 is tree and res.o2 is solid and res.b2 == -1 and res.b1 == int(r["b1"]) >= 0
        assert d == res.min_distance == float(r["distance"])
        for got_v, k in ((res.normal, "normal"), (res.nearest_points[0], "p1"), (res.nearest_points[1], "p2")):
            assert np.array_equal(np.asarray(got_v), r[k], equal_nan=True), (i, k)
        separated += d > 0
        lines_want.append([float(x).hex() for x in [d, d]] + [str(int(r["b1"])), "-1"] + [float(x).hex() for x in list(r["normal"]) + list(r["p1"]) + list(r["p2"])])
    assert 2 < separated < 12
    with pytest.raises(ValueError):
        fcl.distance(tree, fcl.Transform3f(), fcl.Halfspace((0, 0, 1), 0.0), fcl.Transform3f(), fcl.DistanceRequest(), fcl.DistanceResult())
    with pytest.raises(ValueError):
        fcl.ComputeDistance(tree, tree)

    # the same cases through the C++ shim
    exe = str(tmp_path / "test_octree_distance")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_octree_distance.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("%r 4 %d %d\n" % (0.1, len(nodes), len(cases)))
        for nd in nodes:
            f.write(" ".join(str(int(c)) for c in nd["child"]) + " %r\n" % float(nd["occupancy"]))
        for kind, a, b, c, tft, tfs, swapped, signed in cases:
            f.write("%d %r %r %r " % (kind, a, b, c) + " ".join(repr(float(x)) for x in list(tft) + list(tfs)) + " %d %d\n" % (swapped, signed))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    for want_line, line in zip(lines_want, out[:len(cases)]):
        got = line.split()
        assert len(got) == len(want_line), (got, want_line)
        for g, w in zip(got, want_line):
            assert (int(g) == int(w)) if "x" not in w and "n" not in w else (float.fromhex(g) == float.fromhex(w) or ("nan" in g and "nan" in w)), (got, want_line)
    assert "tree first: ok" in r.stdout and "batch: ok" in r.stdout and "halfspace and octree x octree refused" in r.stdout
