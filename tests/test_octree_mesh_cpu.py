"""OcTree x BVHModel<OBBRSS> collide() (include/hppfcl_amd_octree_mesh.h) without a GPU: the C ABI's host-only parts (exports, option keys,
the entry points without a device) and the device header built with g++ (tests/octree_mesh_harness) against the fp64 model
(tests/octree_mesh_model.py) on seeded random trees, meshes and queries and on hand-made cases."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import octree_cases as oc  # noqa: E402
import octree_mesh_cases as omc  # noqa: E402
import octree_mesh_model as omm  # noqa: E402
import octree_model as om  # noqa: E402
import options_table  # noqa: E402

pkg = ge.load_pkg()
abi, engine, geometry = pkg.abi, pkg.engine, pkg.geometry

MARGINS = (0.0, 0.05)
MAX_CONTACTS = (1, 3, 5000)
# (security_margin, enable_contact).  enable_contact off at margin 0 is left to test_root_alone_against_one_triangle: there a leaf in
# collision reports GJK's distance of 0 without running EPA (narrowphase.h:500-504, 638-656), which is "near" the threshold by the
# model's rule, so every penetrating query of that combination would be set aside
MARGIN_CONTACT = ((0.0, 1), (0.05, 1), (0.05, 0))
N_RANDOM = 1260  # 140 queries for each (margin, enable_contact, num_max_contacts)
RESOLUTION = 0.1
SPREAD = 0.9  # how far off a leaf the meshes are placed: tuned until the MODEL alone meets the conditions of the random test
DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return omc.build_harness(tmp_path_factory.mktemp("octree_mesh_harness"))


# ---- 1. symbols, options, entry points ------------------------------------------------------------------------------------------------
def test_symbols():
    lib = engine.dll()
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_octree_mesh.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_octree_mesh_[a-z0-9_]*)\s*\(", hdr)))
    assert syms == sorted(engine.OCTREE_MESH_SYMBOLS) and len(syms) == 3
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    older = (engine.EXPORTED_SYMBOLS + engine.CULL_SYMBOLS + engine.NEAREST_SYMBOLS + engine.PAIRS_SYMBOLS + engine.PAIRS_SORTED_SYMBOLS +
             engine.GROUPS_SYMBOLS + engine.NEAREST_SELF_SYMBOLS + engine.ENV_SYMBOLS + engine.NEAREST_ENV_SYMBOLS + engine.HFIELD_SYMBOLS +
             engine.TERRAIN_SYMBOLS + engine.OCTREE_SYMBOLS + engine.OCTREE_DISTANCE_SYMBOLS)
    assert not set(syms) & set(older)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert len(re.findall(r'#include "[./]*hppfcl_amd_octree_mesh\.h"', main)) == 1
    assert lib.hfcl_abi_version() == 5
    # the older headers keep their symbol lists, and the older calls their answers: a mesh stays refused there
    old = open(os.path.join(ROOT, "include", "hppfcl_amd_octree.h")).read()
    assert len(set(re.findall(r"\b(hfcl_[a-z0-9_]*octree[a-z0-9_]*)\s*\(", old))) == 10
    assert not engine.octree_pair_supported(abi.BV_OBBRSS) and not engine.octree_distance_pair_supported(abi.BV_OBBRSS)
    for for_distance in (0, 1):
        assert lib.hfcl_pair_supported(C.c_int32(abi.GEOM_OCTREE), C.c_int32(abi.BV_OBBRSS), C.c_int(for_distance)) == 0
        assert lib.hfcl_pair_supported(C.c_int32(abi.BV_OBBRSS), C.c_int32(abi.GEOM_OCTREE), C.c_int(for_distance)) == 0
    assert engine.octree_mesh_pair_supported(abi.BV_OBBRSS)
    for t in (9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 0, 1, 4, 6, -1):
        assert not engine.octree_mesh_pair_supported(t), t
    for m in ("octree_mesh_collide", "octree_mesh_collide_device"):
        assert hasattr(engine.Library, m), m
    limit = re.search(r"#define HFCL_OCTREE_MESH_MAX_BVH_DEPTH (\d+)u", hdr)
    assert limit and int(limit.group(1)) == engine.OCTREE_MESH_MAX_BVH_DEPTH == omc.DEPTH_LIMIT >= 64
    assert "Not done:" in hdr and "eight-argument" in hdr and "factor of four" in hdr  # what the header must say


def test_option_keys_unchanged():
    """the call is chunked by the octree path's two options: no new key"""
    assert set(engine.option_keys()) == set(options_table.TABLE)
    assert "octree_chunk" in engine.option_keys() and "octree_items" in engine.option_keys()


def test_entry_points_without_device():
    """No CPU fallback: without a device both entry points say so; with one, a null library is an invalid argument"""
    d = engine.dll()
    req = abi.default_collision_request()
    one = np.zeros(1, dtype=np.uint32)
    tf = geometry.make_pose().reshape(1, 12)
    out = np.zeros(1, dtype=abi.RESULT_DTYPE)
    n = C.c_size_t(7)
    no_device = engine.device_count() == 0
    want = abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT
    rc = d.hfcl_octree_mesh_collide_batch(None, abi.ptr(one), abi.ptr(one), abi.ptr(tf), abi.ptr(tf), C.c_size_t(1), None, C.byref(req),
                                          abi.ptr(out), None, None, C.c_size_t(0), C.byref(n))
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    rc = d.hfcl_octree_mesh_collide_batch_device(None, None, None, None, None, C.c_size_t(1), None, C.byref(req), None, None, None,
                                                 C.c_size_t(0), C.byref(n), None)
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    assert n.value == 7 and out["status"][0] == 0


def test_model_refusals():
    """what OctreeCollide and collide() refuse, in the model (the library's refusals: tests/test_octree_mesh_gpu.py)"""
    tree = om.Tree(oc.tree_from_spec(pkg, oc.OCCUPIED), RESOLUTION, 2)
    me = omc.one_triangle()
    tf = geometry.make_pose().reshape(1, 12)
    req = abi.default_collision_request()
    req.num_max_contacts = 0
    with pytest.raises(ValueError):
        omm.collide([tree], [0], [me], [0], tf, tf, req)
    req.num_max_contacts = 1
    req.security_margin = -0.01
    with pytest.raises(ValueError):
        omm.collide([tree], [0], [me], [0], tf, tf, req)
    req.security_margin = -np.inf
    recs, bounds, contacts, _, items = omm.collide([tree], [0], [me], [0], tf, tf, req, [1])
    assert recs[0]["skipped"] and recs[0]["swapped"] and bounds == [DBL_MAX] and not contacts and not items


# ---- 2. the harness against the model ---------------------------------------------------------------------------------------------------
def records_against_model(got, dlb, contacts, recs, bounds, model_contacts, keep, needed):
    """Integers and the contact order equal; floats bit-equal or within 1e-12 absolute (the tolerance of
    test_octree_cpu.records_against_model / test_hfield_cpu).  needed: the float fields that were not bit-equal somewhere."""
    def same(a, b, what):
        a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
        assert np.array_equal(np.isnan(a), np.isnan(b)), what
        if a.tobytes() != b.tobytes():
            ok = np.isnan(a) | (a == b) | (np.abs(a - b) <= 1e-12)
            assert ok.all(), (what, a, b)
            needed.add(what[0])

    for i in np.flatnonzero(keep):
        r = recs[i]
        assert int(got[i]["num_contacts"]) == r["num_contacts"], i
        assert (int(got[i]["b1"]), int(got[i]["b2"])) == (r["b1"], r["b2"]), i
        assert got[i]["status"] == (15 << 3) | (128 if r["num_contacts"] else 0) | (abi.STATUS_SWAPPED if r["swapped"] else 0), i
        for k in oc.FLOAT_FIELDS:
            same(got[i][k], r[k], ("record." + k, i))
        same(dlb[i], bounds[i], ("bound", i))
    mine = [c for c in contacts if keep[c["pair"]]]
    theirs = [c for c in model_contacts if keep[c["pair"]]]
    assert [(int(c["pair"]), int(c["b1"]), int(c["b2"])) for c in mine] == [(c["pair"], c["b1"], c["b2"]) for c in theirs]
    for a, b in zip(mine, theirs):
        same(a["penetration_depth"], b["depth"], ("contact.depth", b["pair"]))
        for k in ("normal", "p1", "p2"):
            same(a[k], b[k], ("contact." + k, b["pair"]))


def items_equal(items, model_items, keep=None):
    mine = [tuple(int(x) for x in r) for r in items]
    theirs = [tuple(r) for r in model_items]
    if keep is not None:
        mine, theirs = [r for r in mine if keep[r[0]]], [r for r in theirs if keep[r[0]]]
    assert mine == theirs


def random_setup(rng):
    """the random trees of octree_cases (depth 3 - 5, resolution 0.1; leaves at mixed levels, free and uncertain ones among them) and
    meshes of 1, 2, 12 and 288 triangles"""
    trees = [(oc.random_tree(pkg, rng, 3), RESOLUTION, 3), (oc.random_tree(pkg, rng, 4), RESOLUTION, 4),
             (oc.random_tree(pkg, rng, 5, p_child=0.35), RESOLUTION, 5, 0.75, 0.1)]
    meshes = [omc.one_triangle(), omc.two_triangles(), omc.box_mesh(), omc.sphere_mesh(pkg)]
    assert [len(m.triangles) for m in meshes] == [1, 2, 12, 288]
    return trees, meshes


def test_harness_equals_model_on_random_queries(harness):
    rng = np.random.default_rng(21)
    trees, meshes = random_setup(rng)
    ht, hm = oc.HarnessTrees(pkg, trees), omc.HarnessMeshes(pkg, meshes)
    model_trees = [om.Tree(*t) for t in trees]
    per = N_RANDOM // (len(MARGIN_CONTACT) * len(MAX_CONTACTS))
    assert {m for m, _ in MARGIN_CONTACT} == set(MARGINS) and {e for _, e in MARGIN_CONTACT} == {0, 1}
    needed, rejected, total, in_contact, model_in_contact, used, both_orders = set(), 0, 0, 0, 0, set(), set()
    cut_short, model_cut_short, rotated = 0, 0, set()
    for margin, enable in MARGIN_CONTACT:
        for nmax in MAX_CONTACTS:
            ot, me, tft, tfm, sw = omc.random_queries(pkg, rng, trees, len(meshes), per, SPREAD)
            req = abi.default_collision_request()
            req.security_margin = margin
            req.num_max_contacts = nmax
            req.enable_contact = enable
            recs, bounds, contacts, near, items = omm.collide(model_trees, ot, meshes, me, tft, tfm, req, sw)
            got, dlb, con, n_con, hitems = omc.harness_collide(pkg, harness, ht, hm, ot, me, tft, tfm, req, sw, cap=4096 * per,
                                                               items_cap=len(items) + 16)
            assert n_con <= 4096 * per
            keep = ~np.array(near)
            items_equal(hitems, items)  # the walk does not depend on the leaves: every query
            records_against_model(got, dlb, con, recs, bounds, contacts, keep, needed)
            rejected += int((~keep).sum())
            total += per
            in_contact += int((got["num_contacts"] > 0).sum())
            model_in_contact += sum(1 for r in recs if r["num_contacts"] > 0)
            if nmax == 3:  # a query that reached its third contact with items left to list was cut short
                last = {}
                for k, it in enumerate(items):
                    last[it[0]] = k
                third = {}
                for c in contacts:
                    third.setdefault(c["pair"], []).append((c["pair"], c["b1"], c["b2"]))
                model_cut_short += sum(1 for i, cs in third.items() if len(cs) == 3 and items.index(cs[2]) < last[i])
                cut_short += int((got["num_contacts"] == 3).sum())
            used |= set(int(s) for s in me)
            both_orders |= set(int(s) for s in sw)
            rotated |= set(bool(np.array_equal(t[:9], geometry.make_pose().reshape(-1)[:9])) for t in tfm)
    print("random queries: %d, in contact %d (model %d), cut short by num_max_contacts = 3: %d, rejected near a threshold %d; fields that "
          "needed the 1e-12 tolerance: %s" % (total, in_contact, model_in_contact, model_cut_short, rejected, sorted(needed)))
    assert total == N_RANDOM and used == {0, 1, 2, 3} and both_orders == {0, 1} and rotated == {True, False}
    assert rejected < 0.01 * total
    assert 0.25 * total < model_in_contact < 0.75 * total  # (the model alone meets the conditions)
    assert model_cut_short > 0
    assert 0.25 * total < in_contact < 0.75 * total
    assert cut_short >= model_cut_short


def _compare(harness, trees, meshes, ot, me, tft, tfm, req, sw=None, cap=65536):
    ht, hm = oc.HarnessTrees(pkg, trees), omc.HarnessMeshes(pkg, meshes)
    recs, bounds, contacts, near, items = omm.collide([om.Tree(*t) for t in trees], ot, meshes, me, tft, tfm, req, sw)
    got, dlb, con, n_con, hitems = omc.harness_collide(pkg, harness, ht, hm, ot, me, tft, tfm, req, sw, cap=cap, items_cap=len(items) + 16)
    items_equal(hitems, items)
    records_against_model(got, dlb, con, recs, bounds, contacts, ~np.array(near), set())
    return got, dlb, con, items


def test_hand_made_trees_equal_model(harness):
    """the empty tree, the root alone, the three-state tree (free, uncertain, an inner node below the threshold), the deepest chain"""
    rng = np.random.default_rng(2)
    trees = [(oc.empty_tree(pkg), RESOLUTION, 3), (oc.tree_from_spec(pkg, oc.OCCUPIED), RESOLUTION, 2), (oc.three_state_tree(pkg), RESOLUTION, 2),
             (oc.chain_tree(pkg, 16), 0.001, 16)]
    meshes = [omc.one_triangle(), omc.box_mesh(), omc.sphere_mesh(pkg)]
    ot, me, tft, tfm, sw = omc.random_queries(pkg, rng, trees, len(meshes), 160, 0.15)
    req = abi.default_collision_request()
    req.num_max_contacts = 5000
    req.security_margin = 0.05
    got, dlb, con, items = _compare(harness, trees, meshes, ot, me, tft, tfm, req, sw)
    empty = ot == 0
    assert empty.any() and (got["num_contacts"][empty] == 0).all() and (dlb[empty] == DBL_MAX).all()
    assert np.isnan(got["normal"][empty]).all() and not [it for it in items if ot[it[0]] == 0]
    for t in (1, 2, 3):
        assert (got["num_contacts"][ot == t] > 0).any(), t
    # the children of the inner node below the threshold are never reported (nodes 7, 8, 9 of the three-state tree in preorder)
    assert not {int(c["b1"]) for c in con if ot[c["pair"]] == 2} & {1, 2, 7, 8, 9}


def test_root_alone_against_one_triangle(harness):
    """one occupied voxel [-0.2, 0.2]^3 and one triangle: through its top face, 0.1 above it (inside the margin, outside it), far off --
    both orders; the contact's points are the solver's own"""
    trees = [(oc.tree_from_spec(pkg, oc.OCCUPIED), RESOLUTION, 2)]
    meshes = [omm.Mesh([[-0.05, -0.05, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0]], [[0, 1, 2]])]
    z = np.array([0.15, 0.3, 0.3, 5.0])
    tfm = geometry.make_pose(T=np.stack([np.zeros(4), np.zeros(4), z], axis=1))
    tft = geometry.make_pose(T=np.zeros((4, 3)))
    req = abi.default_collision_request()
    for margin, hits in ((0.0, [1, 0, 0, 0]), (0.15, [1, 1, 1, 0])):
        req.security_margin = margin
        got, dlb, con, items = _compare(harness, trees, meshes, [0] * 4, [0] * 4, tft, tfm, req, [0, 0, 1, 0])
        # (0.1 apart without a margin the boxes are disjoint already: the bound is the box test's and no leaf is listed)
        assert list(got["num_contacts"]) == hits and [tuple(it) for it in items] == ([(0, 0, 0), (1, 0, 0), (2, 0, 0)] if margin else [(0, 0, 0)])
        assert (got["status"][2] & abi.STATUS_SWAPPED) and got[1].tobytes()[:80] == got[2].tobytes()[:80]
        assert abs(got["distance"][0] + 0.05) < 1e-6 and abs(dlb[1] - (0.1 - margin)) < 1e-9 and dlb[3] > 4.0
        assert np.isnan(got["normal"][3]).all() and (got["b1"][3], got["b2"][3]) == (-1, -1)
        if margin:  # separated and in contact through the margin: c1 on the voxel's top face, c2 on the triangle
            assert abs(got["p1"][1][2] - 0.2) < 1e-9 and abs(got["p2"][1][2] - 0.3) < 1e-9 and np.allclose(got["normal"][1], [0, 0, 1], atol=1e-9)
            assert len(con) == 3 and (int(con[1]["b1"]), int(con[1]["b2"])) == (0, 0)
        else:
            assert np.isnan(got["normal"][1]).all()  # no leaf lowered the bound
    # enable_contact off at margin 0: the penetrating leaf is GJK's `Collision` without EPA -- distance = GJK's (0 <= d <= its tolerance),
    # NaN points and normal (narrowphase.h:500-504, 638-656) -- and still a contact.  Compared without the model's "near" rule
    req.security_margin = 0.0
    req.enable_contact = 0
    ht, hm = oc.HarnessTrees(pkg, trees), omc.HarnessMeshes(pkg, meshes)
    recs, bounds, contacts, near, items = omm.collide([om.Tree(*t) for t in trees], [0] * 4, meshes, [0] * 4, tft, tfm, req)
    got, dlb, con, n_con, hitems = omc.harness_collide(pkg, harness, ht, hm, [0] * 4, [0] * 4, tft, tfm, req, cap=8, items_cap=8)
    assert near[0] and recs[0]["num_contacts"] == 1 and 0.0 <= recs[0]["distance"] <= 1e-6 and np.isnan(recs[0]["normal"]).all()
    records_against_model(got, dlb, con, recs, bounds, contacts, np.ones(4, dtype=bool), set())


def test_size_rule_is_the_reference_s(harness):
    """One octree node with children and one inner mesh node with extent^2 < diag^2 < 4 extent^2: the reference compares the FULL
    diagonal squared with the HALF extents squared, so the octree side descends first; a rule on the same quantity would descend the
    mesh.  The item orders differ, and the harness has the reference's."""
    # the root [-0.2, 0.2]^3 (depth 2 at 0.1) with two leaf children, 0 and 1, side by side along x: diag^2 = 0.48
    trees = [(oc.tree_from_spec(pkg, (oc.OCCUPIED, {0: oc.OCCUPIED, 1: oc.OCCUPIED})), RESOLUTION, 2)]
    # two long slivers along x, each through both children: the root's OBB has half extents ~ (0.5, 0.07, 0): extent^2 ~ 0.25
    me = omm.Mesh([[-0.5, -0.15, -0.1], [0.5, -0.15, -0.1], [0.0, -0.12, -0.1], [-0.5, -0.05, -0.1], [0.5, -0.05, -0.1], [0.0, -0.02, -0.1]],
                  [[0, 1, 2], [3, 4, 5]])
    ext2 = omm.sq_norm(me.extent[0])
    diag2 = 3 * 0.4 * 0.4
    assert me.first_child[0] > 0 and ext2 < diag2 < 4 * ext2, (ext2, diag2)
    tf = geometry.make_pose().reshape(1, 12)
    req = abi.default_collision_request()
    req.num_max_contacts = 5000
    tree = om.Tree(*trees[0])
    ref = [e[1:2] + e[4:] for e in omm.walk(tree, om.pose(tf[0]), me, om.pose(tf[0]), 0.0, 1e-6) if e[0] == "leaf"]
    other = [e[1:2] + e[4:] for e in omm.walk(tree, om.pose(tf[0]), me, om.pose(tf[0]), 0.0, 1e-6, same_quantity=True) if e[0] == "leaf"]
    assert sorted(ref) == sorted(other) and ref != other and len(ref) == 4, (ref, other)
    got, dlb, con, items = _compare(harness, trees, [me], [0], [0], tf, tf, req)
    assert [tuple(it[1:]) for it in items] == ref and [r[0] for r in ref] == [1, 1, 2, 2]  # the octree side went first
    assert [(int(c["b1"]), int(c["b2"])) for c in con] == ref  # every listed pair touches: the contacts in walk order


def test_chain_mesh_at_the_depth_limit(harness):
    """a mesh whose BVH is a chain: at the limit the harness walks it as the model does; one level deeper the depth computation says
    so and nothing is written"""
    assert harness.omh_depth_limit() == omc.DEPTH_LIMIT
    trees = [(oc.tree_from_spec(pkg, (oc.OCCUPIED, {0: oc.OCCUPIED, 7: oc.OCCUPIED, 5: oc.OCCUPIED})), RESOLUTION, 2)]
    at, over = omc.chain_mesh(omc.DEPTH_LIMIT), omc.chain_mesh(omc.DEPTH_LIMIT + 1)
    for m, levels in ((at, omc.DEPTH_LIMIT), (over, omc.DEPTH_LIMIT + 1)):
        nodes = np.ascontiguousarray(m.nodes)
        assert harness.omh_bvh_depth(abi.ptr(nodes), C.c_size_t(len(nodes))) == levels == m.depth()
    cyc = np.ascontiguousarray(at.nodes).copy()
    deepest = int(np.flatnonzero(cyc["first_child"] > 0)[-1])
    cyc["first_child"][deepest] = 1  # the deepest inner node names the root's children again
    assert harness.omh_bvh_depth(abi.ptr(cyc), C.c_size_t(len(cyc))) == 0xFFFFFFFF
    rng = np.random.default_rng(8)
    n = 24
    tft = geometry.make_pose(quat=oc.random_rotations(rng, n), T=rng.uniform(-0.1, 0.1, (n, 3)))
    tft[:8] = geometry.make_pose()
    tfm = geometry.make_pose(T=rng.uniform(-0.15, 0.15, (n, 3)))
    req = abi.default_collision_request()
    req.num_max_contacts = 5000
    got, dlb, con, items = _compare(harness, trees, [at], [0] * n, [0] * n, tft, tfm, req)
    assert (got["num_contacts"] > 0).any() and (got["num_contacts"] == 0).any()
    ht, hm = oc.HarnessTrees(pkg, trees), omc.HarnessMeshes(pkg, [at, over])
    out, dlb, con, n_con, _ = omc.harness_collide(pkg, harness, ht, hm, [0] * n, [0] * (n - 1) + [1], tft, tfm, req, cap=16, expect=2)
    assert not out.tobytes().strip(b"\0") and not dlb.any() and n_con == 0


def test_skipped_by_infinite_margin(harness):
    rng = np.random.default_rng(3)
    trees, meshes = random_setup(rng)
    ot, me, tft, tfm, sw = omc.random_queries(pkg, rng, trees, len(meshes), 6)
    req = abi.default_collision_request()
    req.security_margin = -np.inf
    got, dlb, con, n_con, items = omc.harness_collide(pkg, harness, oc.HarnessTrees(pkg, trees), omc.HarnessMeshes(pkg, meshes), ot, me, tft, tfm,
                                                      req, sw, cap=8, items_cap=8)
    assert n_con == 0 and len(items) == 0 and (abi.status_skipped(got["status"]) == 1).all() and (got["num_contacts"] == 0).all()
    assert (dlb == DBL_MAX).all() and ((got["status"] & abi.STATUS_SWAPPED) != 0).tolist() == [bool(s) for s in sw]
    # ids outside the tables: the skipped record of the device form
    req.security_margin = 0.0
    ot[0], me[1] = 3, 4
    got, dlb, con, n_con, items = omc.harness_collide(pkg, harness, oc.HarnessTrees(pkg, trees), omc.HarnessMeshes(pkg, meshes), ot, me, tft, tfm,
                                                      req, sw, cap=4096, items_cap=65536)
    assert (abi.status_skipped(got["status"][:2]) == 1).all() and (abi.status_skipped(got["status"][2:]) == 0).all()
    assert not {0, 1} & {int(it[0]) for it in items} and (dlb[:2] == DBL_MAX).all()


def test_host_check_program(tmp_path):
    """the walk's two stacks and the depth computation in a stand-alone program (tests/octree_mesh_harness/host_check.cpp), the form in
    which they are run under a sanitizer"""
    import subprocess
    exe = str(tmp_path / "host_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                           "-o", exe, os.path.join(ROOT, "tests", "octree_mesh_harness", "host_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host_check ok" in r.stdout, r.stdout + r.stderr
