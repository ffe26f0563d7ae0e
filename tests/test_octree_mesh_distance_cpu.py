"""OcTree x BVHModel<OBBRSS> distance() (include/hppfcl_amd_octree_mesh_distance.h) without a GPU: the C ABI's host-only parts (exports,
option keys, the entry points without a device) and the device header built with g++ (tests/octree_mesh_distance_harness) against the
fp64 model (tests/octree_mesh_distance_model.py) on seeded random and hand-made cases.  The answer is the result of the reference's
ORDERED dual walk; both are also held against the brute-force minimum over all reachable leaves x triangles, which the walk equals
whenever that minimum is positive.

Three choices of the random test, each made so that the MODEL alone meets the test's conditions (fewer than 1 % of the queries within
1e-9 of a decision):
  - the meshes of 2, 12 and 288 triangles are triangle soups (octree_mesh_distance_cases.soup): with shared vertices and edges two or
    more triangles are equally far from a voxel in about half of the queries, and the strict `min_distance > distance` between them is a
    decision by less than 1e-9.  (Meshes with shared vertices: tests/test_octree_mesh_distance_gpu.py, device against harness, bytes.)
  - a tree at the identity pose never meets a mesh at the identity rotation: axis-aligned triangles are equally far from several voxels.
  - the requests without enable_signed_distance get meshes placed clear of the tree: a penetrating leaf then reports GJK's distance,
    0 or a little above, and the stop test `<= 0` is a decision by less than 1e-9 for every such query.  test_root_alone_against_one_triangle
    covers that case without the rule.

The request refusals (initial guess, epa_max_iterations, ids, meshes) all come after the device check in the entry points, as in every
compute call of this library, so they are tested in tests/test_octree_mesh_distance_gpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import octree_cases as oc  # noqa: E402
import octree_mesh_distance_cases as omdc  # noqa: E402
import octree_mesh_distance_model as omdm  # noqa: E402
import octree_mesh_model as omm  # noqa: E402
import options_table  # noqa: E402

pkg = ge.load_pkg()
abi, engine, geometry = pkg.abi, pkg.engine, pkg.geometry

DBL_MAX = float(np.finfo(np.float64).max)
SEED = 31
# (spread, signed, clear): 150 queries each.  The spreads were tuned on the model alone until it met the conditions of the random test:
# the two signed batches near the surface give the penetrating share, the two placed clear of the tree the long separated walks
BATCHES = ((0.5, True, False), (0.3, True, False), (0.5, False, True), (1.5, False, True))
N_RANDOM = 600


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return omdc.build_harness(tmp_path_factory.mktemp("octree_mesh_distance_harness"))


# ---- 1. symbols and refusals -----------------------------------------------------------------------------------------------------------
def test_symbols():
    lib = engine.dll()
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_octree_mesh_distance.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_octree_mesh_distance_[a-z0-9_]*)\s*\(", hdr)))
    assert syms == sorted(engine.OCTREE_MESH_DISTANCE_SYMBOLS) == ["hfcl_octree_mesh_distance_batch", "hfcl_octree_mesh_distance_batch_device",
                                                                   "hfcl_octree_mesh_distance_pair_supported"]
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    older = (engine.EXPORTED_SYMBOLS + engine.CULL_SYMBOLS + engine.NEAREST_SYMBOLS + engine.PAIRS_SYMBOLS + engine.PAIRS_SORTED_SYMBOLS +
             engine.GROUPS_SYMBOLS + engine.NEAREST_SELF_SYMBOLS + engine.ENV_SYMBOLS + engine.NEAREST_ENV_SYMBOLS + engine.HFIELD_SYMBOLS +
             engine.TERRAIN_SYMBOLS + engine.OCTREE_SYMBOLS + engine.OCTREE_DISTANCE_SYMBOLS + engine.OCTREE_MESH_SYMBOLS)
    assert not set(syms) & set(older)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert len(re.findall(r'#include "[./]*hppfcl_amd_octree_mesh_distance\.h"', main)) == 1
    assert lib.hfcl_abi_version() == 5
    assert engine.octree_mesh_distance_pair_supported(abi.BV_OBBRSS)
    for t in (9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 0, 1, 4, 6, -1):
        assert not engine.octree_mesh_distance_pair_supported(t), t
    # the older calls keep their answers: the pair stays refused there
    assert not engine.octree_distance_pair_supported(abi.BV_OBBRSS)
    assert lib.hfcl_pair_supported(C.c_int32(abi.GEOM_OCTREE), C.c_int32(abi.BV_OBBRSS), C.c_int(1)) == 0
    assert lib.hfcl_pair_supported(C.c_int32(abi.BV_OBBRSS), C.c_int32(abi.GEOM_OCTREE), C.c_int(1)) == 0
    assert set(engine.option_keys()) == set(options_table.TABLE) and len(engine.option_keys()) == len(options_table.TABLE)  # no key was added
    for m in ("octree_mesh_distance", "octree_mesh_distance_device"):
        assert hasattr(engine.Library, m), m
    assert hasattr(pkg.compat, "distance_octree_mesh")
    # what the header must say
    for words in ("Not done:", "n_nodes == 0", "a choice", "HFCL_OCTREE_MESH_MAX_BVH_DEPTH", "UNSWAPPED", "A wave takes as long as its longest walk",
                  "traversal_node_octree.h:113-124", ":371-458", "rel_err", "not read", "follow-up"):
        assert words in hdr, words


def test_entry_points_without_device():
    """No CPU fallback: without a device both compute entry points say so; with one, a null library is an invalid argument.  No output
    byte is touched."""
    d = engine.dll()
    req = abi.default_distance_request()
    one = np.zeros(1, dtype=np.uint32)
    tf = geometry.make_pose().reshape(1, 12)
    out = np.full(96, 0x5A, dtype=np.uint8)
    vis = np.full(1, 0x5A5A5A5A, dtype=np.uint32)
    no_device = engine.device_count() == 0
    want = abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT
    rc = d.hfcl_octree_mesh_distance_batch(None, abi.ptr(one), abi.ptr(one), abi.ptr(tf), abi.ptr(tf), C.c_size_t(1), None, C.byref(req), abi.ptr(out),
                                           abi.ptr(vis))
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    rc = d.hfcl_octree_mesh_distance_batch_device(None, None, None, None, None, C.c_size_t(1), None, C.byref(req), None, None, None)
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    assert (out == 0x5A).all() and vis[0] == 0x5A5A5A5A


def test_the_dispatch_still_refuses_the_pair():
    """compat._check_pair(tree, mesh, for_distance) raises as before: the call has a name of its own beside the dispatch"""
    fcl = pkg.compat
    tree = fcl.OcTree(oc.tree_from_spec(pkg, oc.OCCUPIED), 0.1, 2)
    m = omdc.one_triangle()
    bm = fcl.BVHModelOBBRSS()
    bm.beginModel()
    bm.addSubModel(m.vertices, m.triangles)
    bm.endModel()
    for a, b in ((tree, bm), (bm, tree)):
        with pytest.raises(ValueError):
            fcl._check_pair(a, b, True)
        fcl._check_pair(a, b, False)  # collide() has the pair
    with pytest.raises(ValueError):  # the call of its own takes an octree and a mesh, nothing else
        fcl.distance_octree_mesh(tree, fcl.Transform3f(), fcl.Sphere(0.1), fcl.Transform3f(), fcl.DistanceRequest(), fcl.DistanceResult())
    with pytest.raises(ValueError):
        fcl.distance_octree_mesh(tree, fcl.Transform3f(), tree, fcl.Transform3f(), fcl.DistanceRequest(), fcl.DistanceResult())


# ---- 2. the harness against the model on random queries ---------------------------------------------------------------------------------
def records_against_model(got, got_visited, recs, visited, keep, needed):
    """Integers equal; floats bit-equal or within 1e-12 absolute (the tolerance of test_octree_distance_cpu.records_against_model).
    needed: the float fields that were not bit-equal somewhere."""
    def same(a, b, what):
        a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
        assert np.array_equal(np.isnan(a), np.isnan(b)), what
        if a.tobytes() != b.tobytes():
            ok = np.isnan(a) | (a == b) | (np.abs(a - b) <= 1e-12)
            assert ok.all(), (what, a, b)
            needed.add(what[0])

    for i in np.flatnonzero(keep):
        r = recs[i]
        assert (int(got[i]["b1"]), int(got[i]["b2"])) == (r["b1"], r["b2"]), i
        assert got[i]["status"] == (15 << 3) | (128 if r["contact"] else 0) | (abi.STATUS_SWAPPED if r["swapped"] else 0), i
        assert int(got[i]["num_contacts"]) == 0
        assert int(got_visited[i]) == visited[i], i
        for k in oc.FLOAT_FIELDS:
            same(got[i][k], r[k], ("record." + k, i))


def pairs_equal(pairs, solved, keep=None):
    mine = [tuple(int(x) for x in r) for r in pairs]
    theirs = [tuple(r) for r in solved]
    if keep is not None:
        mine, theirs = [r for r in mine if keep[r[0]]], [r for r in theirs if keep[r[0]]]
    assert mine == theirs


@pytest.fixture(scope="module")
def step2():
    """the 600 queries of test 2 and the model's answers, computed once: per batch a dict"""
    rng = np.random.default_rng(SEED)
    trees, meshes = omdc.soup_setup(pkg, rng)
    model_trees = [omdm.Tree(*t) for t in trees]
    radii = omdc.mesh_radii(meshes)
    batches = []
    for spread, signed, clear in BATCHES:
        me = omdc.mesh_ids(rng, N_RANDOM // len(BATCHES))
        ot, me, tft, tfm, sw = omdc.random_queries(pkg, rng, trees, me, spread, radii if clear else None)
        req = omdc.request(abi, signed)
        recs, visited, solved, near, took = omdm.distance(model_trees, ot, meshes, me, tft, tfm, req, sw)
        reach = [omdm.reachable_pairs(model_trees[int(o)], meshes[int(m)]) for o, m in zip(ot, me)]
        batches.append(dict(ot=ot, me=me, tft=tft, tfm=tfm, sw=sw, req=req, recs=recs, visited=visited, solved=solved, near=near, took=took, reach=reach,
                            signed=signed))
    return dict(trees=trees, meshes=meshes, model_trees=model_trees, batches=batches)


def _walk_statistics(step2, distances, visited):
    """(meshes used, share of the 288-triangle mesh, separated share, most pairs solved by a query, mean solved share of the reachable pairs)"""
    used, big, sep, total, most, shares = set(), 0, 0, 0, 0, []
    for b, dist, vis in zip(step2["batches"], distances, visited):
        used |= set(int(m) for m in b["me"])
        big += int((b["me"] == 3).sum())
        sep += int((np.asarray(dist) > 0).sum())
        total += len(b["me"])
        most = max(most, int(max(vis)))
        shares += [v / r for v, r in zip(vis, b["reach"]) if r]
    return used, big / total, sep / total, most, float(np.mean(shares))


def _assert_statistics(stats, who):
    used, big, separated, most, share = stats
    print("%s: meshes %s (288 triangles: %.3f of the queries), separated %.3f, most pairs solved in a query %d, mean solved share %.3f" %
          (who, sorted(used), big, separated, most, share))
    assert used == {0, 1, 2, 3} and 0 < big <= 0.1
    assert 0.2 < separated < 0.8
    assert most > 100
    assert share < 0.5  # pruning happens


def test_harness_equals_model_on_random_queries(harness, step2):
    ht, hm = oc.HarnessTrees(pkg, step2["trees"]), omdc.HarnessMeshes(pkg, step2["meshes"])
    ident = geometry.make_pose().reshape(-1)[:9]
    # the model alone meets the conditions
    _assert_statistics(_walk_statistics(step2, [[r["distance"] for r in b["recs"]] for b in step2["batches"]], [b["visited"] for b in step2["batches"]]),
                       "model")
    total = sum(len(b["me"]) for b in step2["batches"])
    model_near = sum(int(sum(b["near"])) for b in step2["batches"])
    took = set().union(*[t for b in step2["batches"] for t in b["took"]])
    print("model: %d queries, %d near a decision (%s)" % (total, model_near, sorted(t for t in took if t.startswith("near"))))
    assert total == N_RANDOM and model_near < 0.01 * total
    assert {"octree by size", "octree by mesh leaf", "mesh"} <= took  # both descent branches, rule 3 also through the size comparison
    assert {s for b in step2["batches"] for s in b["sw"].tolist()} == {0, 1} and {b["signed"] for b in step2["batches"]} == {True, False}
    rot_t = {bool(np.array_equal(t[:9], ident)) for b in step2["batches"] for t in np.asarray(b["tft"]).reshape(-1, 12)}
    rot_m = {bool(np.array_equal(t[:9], ident)) for b in step2["batches"] for t in np.asarray(b["tfm"]).reshape(-1, 12)}
    assert rot_t == {True, False} and rot_m == {True, False}
    # the harness
    needed, got_all = set(), []
    for b in step2["batches"]:
        got, vis, pairs = omdc.harness_distance(pkg, harness, ht, hm, b["ot"], b["me"], b["tft"], b["tfm"], b["req"], b["sw"], pairs_cap=len(b["solved"]) + 4096)
        keep = ~np.array(b["near"])
        records_against_model(got, vis, b["recs"], b["visited"], keep, needed)
        pairs_equal(pairs, b["solved"], keep)
        got_all.append((got, vis))
    print("random queries: %d, set aside near a decision %d; fields that needed the 1e-12 tolerance: %s" % (total, model_near, sorted(needed)))
    _assert_statistics(_walk_statistics(step2, [g["distance"] for g, _ in got_all], [v.tolist() for _, v in got_all]), "harness")


# ---- 3. hand-made cases --------------------------------------------------------------------------------------------------------------------
def _compare(harness, trees, meshes, ot, me, tft, tfm, req, sw=None, every=False):
    """harness against model; every: the queries near a decision too.  Returns (records, visited, pairs, model records, near)"""
    ht, hm = oc.HarnessTrees(pkg, trees), omdc.HarnessMeshes(pkg, meshes)
    recs, visited, solved, near, _ = omdm.distance([omdm.Tree(*t) for t in trees], ot, meshes, me, tft, tfm, req, sw)
    got, vis, pairs = omdc.harness_distance(pkg, harness, ht, hm, ot, me, tft, tfm, req, sw, pairs_cap=len(solved) + 4096)
    keep = np.ones(len(ot), dtype=bool) if every else ~np.array(near)
    records_against_model(got, vis, recs, visited, keep, set())
    pairs_equal(pairs, solved, keep)
    return got, vis, pairs, recs, near


def test_empty_tree_and_unoccupied_root(harness):
    """the empty tree (a choice) and a root that is an unoccupied leaf: DBL_MAX, NaN points, no node, nothing visited"""
    trees = [(oc.empty_tree(pkg), omdc.RESOLUTION, 3), (oc.tree_from_spec(pkg, oc.UNCERTAIN), omdc.RESOLUTION, 2),
             (oc.tree_from_spec(pkg, oc.FREE), omdc.RESOLUTION, 2)]
    meshes = [omdc.one_triangle(), omdc.box_mesh()]
    rng = np.random.default_rng(5)
    n = 12
    tft = geometry.make_pose(quat=oc.random_rotations(rng, n), T=rng.uniform(-0.5, 0.5, (n, 3)))
    tfm = geometry.make_pose(quat=oc.random_rotations(rng, n), T=rng.uniform(-0.5, 0.5, (n, 3)))
    ot, me, sw = np.arange(n) % 3, np.arange(n) % 2, (np.arange(n) // 3) % 2
    got, vis, pairs, _, near = _compare(harness, trees, meshes, ot, me, tft, tfm, omdc.request(abi), sw, every=True)
    assert not any(near) and len(pairs) == 0 and (vis == 0).all()
    assert (got["distance"] == DBL_MAX).all() and (got["b1"] == -1).all() and (got["b2"] == -1).all()
    for k in ("normal", "p1", "p2"):
        assert np.isnan(got[k]).all()
    assert (got["status"] == (15 << 3) | np.where(sw, abi.STATUS_SWAPPED, 0)).all()


def test_root_alone_against_one_triangle(harness):
    """one occupied voxel [-0.2, 0.2]^3 and one triangle: 0.1 above its top face, and through it with and without enable_signed_distance"""
    trees = [(oc.tree_from_spec(pkg, oc.OCCUPIED), omdc.RESOLUTION, 2)]
    meshes = [omm.Mesh([[-0.05, -0.05, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0]], [[0, 1, 2]])]
    tfm = geometry.make_pose(T=np.array([[0.0, 0.0, 0.3], [0.0, 0.0, 0.15], [0.0, 0.0, 0.3]]))
    tft = geometry.make_pose(T=np.zeros((3, 3)))
    got, vis, pairs, _, near = _compare(harness, trees, meshes, [0] * 3, [0] * 3, tft, tfm, omdc.request(abi, True), [0, 0, 1])
    assert not any(near) and vis.tolist() == [1, 1, 1] and [tuple(p) for p in pairs] == [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    assert abs(got["distance"][0] - 0.1) < 1e-9 and (got["b1"][0], got["b2"][0]) == (0, 0) and got["status"][0] == 15 << 3
    assert abs(got["p1"][0][2] - 0.2) < 1e-9 and abs(got["p2"][0][2] - 0.3) < 1e-9 and np.allclose(got["normal"][0], [0, 0, 1], atol=1e-9)
    assert got["distance"][1] < 0 and abs(got["distance"][1] + 0.05) < 1e-6 and got["status"][1] == (15 << 3) | 128
    assert got["status"][2] == (15 << 3) | abi.STATUS_SWAPPED and got[0].tobytes()[:80] == got[2].tobytes()[:80]
    # without enable_signed_distance the penetrating leaf is GJK's `Collision` without EPA: GJK's distance (0 <= d <= its tolerance), NaN
    # points and normal (narrowphase.h:638-656), bit 7.  Within 1e-9 of the stop test by the model's rule: compared without it
    got, vis, pairs, recs, near = _compare(harness, trees, meshes, [0] * 3, [0] * 3, tft, tfm, omdc.request(abi, False), [0, 0, 1], every=True)
    assert near[1] and not near[0] and 0.0 <= recs[1]["distance"] <= 1e-6 and np.isnan(recs[1]["normal"]).all()
    assert 0.0 <= got["distance"][1] <= 1e-6 and got["status"][1] == (15 << 3) | 128 and (got["b1"][1], got["b2"][1]) == (0, 0) and vis[1] == 1
    for k in ("normal", "p1", "p2"):
        assert np.isnan(got[k][1]).all()
    assert abs(got["distance"][0] - 0.1) < 1e-9


def test_three_state_tree(harness):
    """free, uncertain, an inner node below the threshold: the free and the uncertain leaf (nodes 1, 2) and the children of the inner node
    below the threshold (7: the inner node, 8, 9) are never b1, and never solved"""
    rng = np.random.default_rng(2)
    trees = [(oc.three_state_tree(pkg), omdc.RESOLUTION, 2)]
    meshes = [omdc.one_triangle(), omdc.soup(omdc.box_mesh())]
    n = 60
    ot, me, tft, tfm, sw = omdc.random_queries(pkg, rng, trees, rng.integers(0, 2, n).astype(np.uint32), 0.4)
    got, vis, pairs, _, near = _compare(harness, trees, meshes, ot, me, tft, tfm, omdc.request(abi), sw)
    assert sum(near) < 3 and (got["b1"] >= 0).all() and (vis >= 1).all()
    assert not set(got["b1"].tolist()) & {1, 2, 7, 8, 9} and not {int(p[1]) for p in pairs} & {1, 2, 7, 8, 9}
    assert (got["distance"] > 0).any() and (got["distance"] <= 0).any()


def _deep_voxel(nodes, resolution, depth):
    """(node, lo, hi) of the smallest reachable leaf"""
    return min(oc.leaf_boxes(nodes, resolution, depth), key=lambda b: b[2][0] - b[1][0])


def test_chains_at_the_depth_limit(harness):
    """chain_tree(16) against chain_mesh(DEPTH_LIMIT), the chain's LAST triangle next to the tree's deepest voxel: that pair is the nearest,
    every level of both chains lies on the way to it, and a walk that solves it holds 16 octree frames and DEPTH_LIMIT - 1 mesh frames.
    One level deeper the depth computation says so and nothing is written."""
    assert harness.omdh_depth_limit() == omdc.DEPTH_LIMIT
    trees = [(oc.chain_tree(pkg, 16), 0.001, 16)]
    at, over = omdc.chain_mesh(omdc.DEPTH_LIMIT), omdc.chain_mesh(omdc.DEPTH_LIMIT + 1)
    for m, levels in ((at, omdc.DEPTH_LIMIT), (over, omdc.DEPTH_LIMIT + 1)):
        nodes = np.ascontiguousarray(m.nodes)
        assert harness.omdh_bvh_depth(abi.ptr(nodes), C.c_size_t(len(nodes))) == levels == m.depth()
    deep, lo, hi = _deep_voxel(*trees[0])
    assert abs((hi[0] - lo[0]) - 0.001) < 1e-12
    rng = np.random.default_rng(8)
    n = 24
    tft = geometry.make_pose(quat=oc.random_rotations(rng, n), T=rng.uniform(-0.1, 0.1, (n, 3)))
    tft[:8] = geometry.make_pose()
    quat = oc.random_rotations(rng, n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    local = 0.5 * (np.array(lo) + np.array(hi)) + d * rng.uniform(0.002, 0.02, (n, 1))  # where the last triangle's first vertex goes, tree frame
    rot_only = geometry.make_pose(quat=quat, T=np.zeros((n, 3)))
    v = geometry.transform_point(rot_only, np.repeat(at.vertices[3 * (omdc.DEPTH_LIMIT - 1)].reshape(1, 3), n, axis=0))
    tfm = geometry.make_pose(quat=quat, T=geometry.transform_point(tft, local) - v)
    got, vis, pairs, _, near = _compare(harness, trees, [at], [0] * n, [0] * n, tft, tfm, omdc.request(abi))
    full = {int(p[0]) for p in pairs if (int(p[1]), int(p[2])) == (deep, omdc.DEPTH_LIMIT - 1)}
    print("queries whose walk solved (deepest voxel, last triangle): %d of %d" % (len(full), n))
    assert len(full) >= n // 4
    assert any((int(got["b1"][i]), int(got["b2"][i])) == (deep, omdc.DEPTH_LIMIT - 1) for i in full)
    ht, hm = oc.HarnessTrees(pkg, trees), omdc.HarnessMeshes(pkg, [at, over])
    out, vis, _ = omdc.harness_distance(pkg, harness, ht, hm, [0] * n, [0] * (n - 1) + [1], tft, tfm, omdc.request(abi), expect=2)
    assert not out.tobytes().strip(b"\0") and not vis.any()


# ---- 4. the size rule -----------------------------------------------------------------------------------------------------------------------
def test_size_rule_is_the_reference_s(harness):
    """The two-leaf tree and the two-sliver mesh of test_octree_mesh_cpu.test_size_rule_is_the_reference_s, the mesh lifted clear of the
    tree (a walk over touching pairs ends at its first).  extent^2 < diag^2 < 4 extent^2: the reference compares the FULL diagonal
    squared with the HALF extents squared, so the octree side descends first; a rule on the same quantity would descend the mesh.  The
    orders of the solved pairs differ, and the harness has the reference's."""
    trees = [(oc.tree_from_spec(pkg, (oc.OCCUPIED, {0: oc.OCCUPIED, 1: oc.OCCUPIED})), omdc.RESOLUTION, 2)]
    me = omm.Mesh([[-0.5, -0.15, -0.1], [0.5, -0.15, -0.1], [0.0, -0.12, -0.1], [-0.5, -0.05, -0.1], [0.5, -0.05, -0.1], [0.0, -0.02, -0.1]],
                  [[0, 1, 2], [3, 4, 5]])
    ext2, diag2 = omm.sq_norm(me.extent[0]), 3 * 0.4 * 0.4
    assert me.first_child[0] > 0 and ext2 < diag2 < 4 * ext2, (ext2, diag2)
    tft = geometry.make_pose().reshape(1, 12)
    # the slivers about z = 0.15 (the two leaves end at z = 0), tilted a little about x and about y: no two of the four pairs equally far
    ca, sa, cb, sb = np.cos(0.05), np.sin(0.05), np.cos(0.03), np.sin(0.03)
    R = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    tfm = np.concatenate([R.T.reshape(-1), [0.0, 0.0, 0.25]]).reshape(1, 12)  # (the ABI's pose image: the rotation column by column, then T)
    req = omdc.request(abi)
    tree = [omdm.Tree(*trees[0])]
    _, _, ref, near, took = omdm.distance(tree, [0], [me], [0], tft, tfm, req)
    _, _, other, _, took_other = omdm.distance(tree, [0], [me], [0], tft, tfm, req, same_quantity=True)
    ref, other = [r[1:] for r in ref], [r[1:] for r in other]
    assert not near[0] and sorted(ref) == sorted(other) and ref != other and len(ref) == 4, (ref, other)
    assert [r[0] for r in ref] == [1, 1, 2, 2] and [r[1] for r in other] == [other[0][1]] * 2 + [other[2][1]] * 2  # the octree side went first / the mesh side
    assert "octree by size" in took[0] and "octree by size" not in took_other[0]
    got, vis, pairs, _, _ = _compare(harness, trees, [me], [0], [0], tft, tfm, req)
    assert [tuple(int(x) for x in p[1:]) for p in pairs] == ref and vis[0] == 4 and 0.1 < got["distance"][0] < 0.2


# ---- 5. the ordered walk equals brute force --------------------------------------------------------------------------------------------------
def test_the_ordered_walk_equals_brute_force(harness, step2):
    """Both converted boxes enclose their bounding volumes, so a pruned branch holds no pair below the minimum: for every query of test 2
    on a mesh of at most 12 triangles whose brute-force minimum over all reachable occupied leaves x triangles is positive (those near a
    decision left out), the distance is that minimum -- exactly for the model (a minimum over a subset of the same numbers), within 1e-12
    for the harness -- and the pair (b1, b2) attains it.  (A query whose walk answers <= 0 holds a pair <= 0: its minimum is not
    positive, and it needs no brute force.)"""
    ht, hm = oc.HarnessTrees(pkg, step2["trees"]), omdc.HarnessMeshes(pkg, step2["meshes"])
    checked = pairs_total = 0
    for b in step2["batches"]:
        which = [i for i in range(len(b["me"])) if b["me"][i] != 3 and not b["near"][i] and b["recs"][i]["distance"] > 0 and b["reach"][i]]
        brute = omdm.brute_force(step2["model_trees"], b["ot"], step2["meshes"], b["me"], b["tft"], b["tfm"], b["req"], which)
        got, _, _ = omdc.harness_distance(pkg, harness, ht, hm, b["ot"], b["me"], b["tft"], b["tfm"], b["req"], b["sw"])
        for i in which:
            nodes, prims, dist = brute[i]
            assert len(dist) == b["reach"][i]
            pairs_total += len(dist)
            m = float(dist.min())
            assert m > 0, (i, m, b["recs"][i]["distance"])  # (the walk answered > 0: no reachable pair may touch)
            attain = {(int(nd), int(pr)) for nd, pr in zip(nodes[dist == m], prims[dist == m])}
            r = b["recs"][i]
            assert r["distance"] == m and (r["b1"], r["b2"]) in attain, (i, r["distance"], m)
            within = {(int(nd), int(pr)) for nd, pr in zip(nodes[dist <= m + 1e-12], prims[dist <= m + 1e-12])}
            assert abs(float(got["distance"][i]) - m) <= 1e-12 and (int(got["b1"][i]), int(got["b2"][i])) in within, (i, got["distance"][i], m)
            checked += 1
    print("separated queries held against the brute-force minimum: %d (%d pairs)" % (checked, pairs_total))
    assert checked > 100


# ---- 6. the walk in a stand-alone program -----------------------------------------------------------------------------------------------------
def test_host_check_program(tmp_path):
    """the walk on the deepest path stack and on a full block against the 12-triangle mesh in a stand-alone program
    (tests/octree_mesh_distance_harness/host_check.cpp), the form in which the header is run under a sanitizer: built with
    -fsanitize=address,undefined and executed directly"""
    exe = str(tmp_path / "host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + omdc.GCC_FLAGS +
                          ["-o", exe, os.path.join(ROOT, "tests", "octree_mesh_distance_harness", "host_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host_check ok" in r.stdout, r.stdout + r.stderr
