"""OcTree x convex solid collide() (include/hppfcl_amd_octree.h) without a GPU: the C ABI's host-only parts (struct size, exports,
option keys, the validator, the builder from points against a brute-force dictionary of keys) and the device header built with g++
(tests/octree_harness) against the fp64 model (tests/octree_model.py) on seeded random trees and queries."""
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
import octree_model as om  # noqa: E402

pkg = ge.load_pkg()
abi, engine, geometry = pkg.abi, pkg.engine, pkg.geometry

MARGINS = (0.0, 0.05)
MAX_CONTACTS = (1, 3, 5000)
N_RANDOM = 2016  # 336 queries for each (margin, num_max_contacts)
RESOLUTION = 0.1  # not a power of two: the chain of halvings is not key * resolution in the last bit


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.build_harness(tmp_path_factory.mktemp("octree_harness"))


# ---- 1. struct, symbols, options ------------------------------------------------------------------------------------------------------
def test_struct_size():
    assert abi.OCTREE_NODE_DTYPE.itemsize == 40
    assert abi.OCTREE_NODE_DTYPE.fields["child"][1] == 0 and abi.OCTREE_NODE_DTYPE.fields["occupancy"][1] == 32
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_octree.h")).read()
    assert re.search(r"uint32_t child\[8\];[^}]*double occupancy;\s*\} hfcl_octree_node;", hdr, re.S)


def test_symbols():
    lib = engine.dll()
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_octree.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_[a-z0-9_]*octree[a-z0-9_]*)\s*\(", hdr)))
    assert syms == sorted(engine.OCTREE_SYMBOLS) and len(syms) == 10
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    older = (engine.EXPORTED_SYMBOLS + engine.CULL_SYMBOLS + engine.NEAREST_SYMBOLS + engine.PAIRS_SYMBOLS + engine.GROUPS_SYMBOLS +
             engine.NEAREST_SELF_SYMBOLS + engine.ENV_SYMBOLS + engine.NEAREST_ENV_SYMBOLS + engine.HFIELD_SYMBOLS + engine.TERRAIN_SYMBOLS)
    assert not set(syms) & set(older)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert len(re.findall(r'#include "[./]*hppfcl_amd_octree\.h"', main)) == 1
    assert lib.hfcl_abi_version() == 5
    for other in (9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 5, 18, 20, 21):  # GEOM_OCTREE stays unsupported in the per-pair matrix
        for for_distance in (0, 1):
            assert lib.hfcl_pair_supported(C.c_int32(abi.GEOM_OCTREE), C.c_int32(other), C.c_int(for_distance)) == 0
            assert lib.hfcl_pair_supported(C.c_int32(other), C.c_int32(abi.GEOM_OCTREE), C.c_int(for_distance)) == 0
    for t in (9, 10, 11, 12, 13, 14, 19):
        assert engine.octree_pair_supported(t)
    for t in (15, 16, 17, 5, 0, 18, 20, 21, -1):
        assert not engine.octree_pair_supported(t)
    assert "octree_chunk" in engine.option_keys() and "octree_items" in engine.option_keys()
    for m in ("add_octree", "octree_set_thresholds", "octree_collide", "octree_collide_device", "clear_octrees", "octree_count",
              "octree_root_box"):
        assert hasattr(engine.Library, m), m
    assert "Not done:" in hdr and "NOT checked against it" in hdr and "registered node array" in hdr  # what the header must say


def test_entry_points_without_device():
    """No CPU fallback: without a device both compute entry points say so; with one, a null library is an invalid argument.  The
    host-only calls take no device."""
    d = engine.dll()
    req = abi.default_collision_request()
    one = np.zeros(1, dtype=np.uint32)
    tf = geometry.make_pose().reshape(1, 12)
    out = np.zeros(1, dtype=abi.RESULT_DTYPE)
    n = C.c_size_t(7)
    no_device = engine.device_count() == 0
    want = abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT
    rc = d.hfcl_octree_collide_batch(None, abi.ptr(one), abi.ptr(one), abi.ptr(tf), abi.ptr(tf), C.c_size_t(1), None, C.byref(req), abi.ptr(out),
                                     None, None, C.c_size_t(0), C.byref(n))
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    rc = d.hfcl_octree_collide_batch_device(None, None, None, None, None, C.c_size_t(1), None, C.byref(req), None, None, None, C.c_size_t(0),
                                            C.byref(n), None)
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    assert n.value == 7 and out["status"][0] == 0
    root = oc.tree_from_spec(pkg, oc.OCCUPIED)
    assert d.hfcl_lib_add_octree(None, abi.ptr(root), C.c_size_t(1), C.c_double(0.1), C.c_uint32(1), C.c_double(0.5), C.c_double(0.0)) == -1
    assert d.hfcl_lib_octree_count(None) == 0
    assert d.hfcl_lib_clear_octrees(None) == abi.ERR_INVALID_ARGUMENT
    assert d.hfcl_lib_octree_set_thresholds(None, C.c_int(0), C.c_double(0.5), C.c_double(0.0)) == abi.ERR_INVALID_ARGUMENT
    assert d.hfcl_octree_root_box(None, C.c_int(0), abi.ptr(np.zeros(6))) == abi.ERR_INVALID_ARGUMENT


# ---- 2. the validator: one tree per rule ------------------------------------------------------------------------------------------------
def _validate(nodes, depth):
    nodes = np.ascontiguousarray(nodes, dtype=abi.OCTREE_NODE_DTYPE)
    return engine.dll().hfcl_octree_validate(abi.ptr(nodes) if len(nodes) else None, C.c_size_t(len(nodes)), C.c_uint32(depth))


def test_validator_accepts():
    assert _validate(oc.empty_tree(pkg), 1) == abi.OK
    assert _validate(oc.tree_from_spec(pkg, oc.OCCUPIED), 1) == abi.OK
    assert _validate(oc.three_state_tree(pkg), 2) == abi.OK
    assert _validate(oc.chain_tree(pkg, 16), 16) == abi.OK
    assert _validate(oc.block_tree(pkg), 4) == abi.OK
    engine.octree_validate(oc.three_state_tree(pkg), 2)


@pytest.mark.parametrize("rule", ["depth_zero", "depth_17", "child_out_of_range", "child_is_root_sized", "two_parents", "orphan", "cycle",
                                  "too_deep", "nan_occupancy"])
def test_validator_refusals(rule):
    good = oc.tree_from_spec(pkg, (0.8, {0: 0.8, 3: (0.8, {1: 0.8})}))  # nodes 0 (root), 1, 2, 3; depth 2
    assert _validate(good, 2) == abi.OK
    t, depth = good.copy(), 2
    if rule == "depth_zero":
        depth = 0
    elif rule == "depth_17":
        depth = 17
    elif rule == "child_out_of_range":
        t["child"][2][5] = 4  # n_nodes
    elif rule == "child_is_root_sized":
        t["child"][2][5] = 0xFFFFFFFF
    elif rule == "two_parents":
        t["child"][0][6] = 3  # node 3 is the child of node 2 already
    elif rule == "orphan":
        t["child"][0][0] = 0  # node 1 loses its parent
    elif rule == "cycle":
        # nodes 2 and 3 name each other and the root names neither: every node but the root keeps exactly one parent
        t["child"][0][3] = 0
        t["child"][3][0] = 2
    elif rule == "too_deep":
        depth = 1
    elif rule == "nan_occupancy":
        t["occupancy"][3] = np.nan
    assert _validate(t, depth) == abi.ERR_INVALID_ARGUMENT, rule
    assert "hfcl_octree_validate" in engine.last_error()
    with pytest.raises(pkg.EngineError):
        engine.octree_validate(t, depth)


# ---- 3. the builder from points -----------------------------------------------------------------------------------------------------------
def _brute_force(points, resolution, depth):
    """the tree as nested dictionaries of keys: {path of child indices: hits}"""
    half = 1 << (depth - 1)
    hits = {}
    for p in points:
        key = []
        for x in p:
            if not np.isfinite(x):
                key = None
                break
            k = int(np.floor(x / resolution)) + half
            if k < 0 or k >= (1 << depth):
                key = None
                break
            key.append(k)
        if key is None:
            continue
        path = tuple(((key[0] >> b) & 1) | (((key[1] >> b) & 1) << 1) | (((key[2] >> b) & 1) << 2) for b in range(depth - 1, -1, -1))
        hits[path] = hits.get(path, 0) + 1
    return hits


def _leaf_occupancy(h):
    if h == 1:
        return 0.7
    odds = (0.7 / 0.3) ** h
    return min(odds / (1.0 + odds), 0.97)


@pytest.mark.parametrize("depth,n,seed", [(1, 5, 0), (3, 40, 1), (5, 300, 2), (16, 200, 3)])
def test_from_points_equals_brute_force(depth, n, seed):
    rng = np.random.default_rng(seed)
    res = RESOLUTION
    side = (1 << depth) * res
    pts = rng.uniform(-0.6 * side, 0.6 * side, (n, 3))  # some outside
    pts[: n // 4] = pts[n // 4: 2 * (n // 4)]  # repeated hits
    if n >= 8:
        pts[2] = pts[3] = pts[0]  # ... some voxels more than twice
    pts[-1] = [np.nan, 0.0, 0.0]
    nodes = engine.octree_from_points(pts, res, depth)
    hits = _brute_force(pts, res, depth)
    assert 0 < len(hits) < n  # some dropped
    prefixes = {p[:k] for p in hits for k in range(depth + 1)}
    assert len(nodes) == len(prefixes)
    engine.octree_validate(nodes, depth)
    # preorder with the children in index order = the sorted prefixes
    order = sorted(prefixes)
    index = {p: i for i, p in enumerate(order)}
    for p, i in index.items():
        kids = [int(c) for c in nodes[i]["child"]]
        for k in range(8):
            assert kids[k] == index.get(p + (k,), 0), (p, k)
        if len(p) == depth:
            want = _leaf_occupancy(hits[p])
            assert abs(float(nodes[i]["occupancy"]) - want) < 1e-15 and (hits[p] > 1 or nodes[i]["occupancy"] == 0.7)
            assert 0.7 <= nodes[i]["occupancy"] <= 0.97
        else:
            assert nodes[i]["occupancy"] == max(float(nodes[c]["occupancy"]) for c in kids if c)
    # no points, or none inside: the empty tree
    assert len(engine.octree_from_points(np.zeros((0, 3)), res, depth)) == 0
    assert len(engine.octree_from_points(np.full((3, 3), 10.0 * side), res, depth)) == 0


def test_from_points_refusals():
    d = engine.dll()
    n = C.c_size_t(0)
    p = np.zeros((2, 3))
    p[1] = 0.35
    for res, depth in ((0.0, 4), (-1.0, 4), (np.nan, 4), (np.inf, 4), (0.1, 0), (0.1, 17)):
        assert d.hfcl_octree_from_points(abi.ptr(p), C.c_size_t(2), C.c_double(res), C.c_uint32(depth), None, C.c_size_t(0),
                                         C.byref(n)) == abi.ERR_INVALID_ARGUMENT
    out = np.zeros(3, dtype=abi.OCTREE_NODE_DTYPE)
    assert d.hfcl_octree_from_points(abi.ptr(p), C.c_size_t(2), C.c_double(0.1), C.c_uint32(4), abi.ptr(out), C.c_size_t(3),
                                     C.byref(n)) == abi.ERR_LIMIT
    assert n.value == 7 and (out["occupancy"] == 0).all()  # keys 8 and 11: the voxels share three levels and have two of their own each; nothing written


# ---- 4. the harness against the model ------------------------------------------------------------------------------------------------------
def records_against_model(got, dlb, contacts, recs, bounds, model_contacts, keep, needed):
    """Integers and the contact order equal; floats bit-equal or within 1e-12 absolute (the tolerances of
    test_hfield_cpu.records_against_model).  needed: the float fields that were not bit-equal somewhere."""
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


def random_setup(rng):
    """three random trees of depth 3 - 5 at resolution 0.1 (leaves at mixed levels, free and uncertain ones among them) and the solids"""
    trees = [(oc.random_tree(pkg, rng, 3), RESOLUTION, 3), (oc.random_tree(pkg, rng, 4), RESOLUTION, 4),
             (oc.random_tree(pkg, rng, 5, p_child=0.35), RESOLUTION, 5, 0.75, 0.1)]
    L, solids = oc.seven_solids(pkg, rng)
    return trees, L, solids


def test_halving_is_not_key_times_resolution():
    """why the walk carries the boxes: at resolution 0.1 some box of a depth-5 tree differs from key * resolution in the last bit"""
    rng = np.random.default_rng(5)
    nodes = oc.random_tree(pkg, rng, 5, p_leaf=0.0)
    differ = 0
    for _, lo, hi in oc.leaf_boxes(nodes, RESOLUTION, 5):
        for a in range(3):
            k = round(lo[a] / RESOLUTION)
            differ += (lo[a] != k * RESOLUTION) or (hi[a] != (k + 1) * RESOLUTION)
    assert differ > 0


def test_harness_equals_model_on_random_queries(harness):
    rng = np.random.default_rng(11)
    trees, L, solids = random_setup(rng)
    ht = oc.HarnessTrees(pkg, trees)
    model_trees = [om.Tree(*t) for t in trees]
    per = N_RANDOM // (len(MARGINS) * len(MAX_CONTACTS))
    needed, rejected, total, in_contact, model_in_contact, kinds, both_orders, most = set(), 0, 0, 0, 0, set(), set(), 0
    for margin in MARGINS:
        for nmax in MAX_CONTACTS:
            ot, sh, tft, tfs, sw = oc.random_queries(pkg, rng, trees, solids, per)
            req = abi.default_collision_request()
            req.security_margin = margin
            req.num_max_contacts = nmax
            recs, bounds, contacts, near = om.collide(model_trees, ot, L.shapes_array(), L.vertices_array(), sh, tft, tfs, req, sw)
            got, dlb, con, n_con, n_items = oc.harness_collide(pkg, harness, ht, L, ot, sh, tft, tfs, req, sw, cap=64 * per)
            assert n_con <= 64 * per
            keep = ~np.array(near)
            records_against_model(got, dlb, con, recs, bounds, contacts, keep, needed)
            rejected += int((~keep).sum())
            total += per
            in_contact += int((got["num_contacts"] > 0).sum())
            model_in_contact += sum(1 for r in recs if r["num_contacts"] > 0)
            most = max(most, int(got["num_contacts"].max()))
            kinds |= set(int(s) for s in sh)
            both_orders |= set(int(s) for s in sw)
    print("random queries: %d, in contact %d (model %d), most contacts in a query %d, rejected near a threshold %d; fields that needed "
          "the 1e-12 tolerance: %s" % (total, in_contact, model_in_contact, most, rejected, sorted(needed)))
    assert total == N_RANDOM and len(kinds) == 7 and both_orders == {0, 1}
    assert rejected < 0.01 * total
    assert 0.25 * total < model_in_contact < 0.75 * total  # (the model alone meets the condition)
    assert 0.25 * total < in_contact < 0.75 * total
    assert most > 3  # num_max_contacts = 3 cut some query short, 5000 none


def test_hand_made_trees_equal_model(harness):
    """the empty tree, the root alone, the three-state tree (free, uncertain, an inner node below the threshold), the deepest chain"""
    rng = np.random.default_rng(2)
    trees = [(oc.empty_tree(pkg), RESOLUTION, 3), (oc.tree_from_spec(pkg, oc.OCCUPIED), RESOLUTION, 2), (oc.three_state_tree(pkg), RESOLUTION, 2),
             (oc.chain_tree(pkg, 16), 0.001, 16)]
    L, solids = oc.seven_solids(pkg, rng)
    ht = oc.HarnessTrees(pkg, trees)
    model_trees = [om.Tree(*t) for t in trees]
    ot, sh, tft, tfs, sw = oc.random_queries(pkg, rng, trees, solids, 200)
    req = abi.default_collision_request()
    req.num_max_contacts = 5000
    req.security_margin = 0.05
    recs, bounds, contacts, near = om.collide(model_trees, ot, L.shapes_array(), L.vertices_array(), sh, tft, tfs, req, sw)
    got, dlb, con, n_con, n_items = oc.harness_collide(pkg, harness, ht, L, ot, sh, tft, tfs, req, sw, cap=4096)
    records_against_model(got, dlb, con, recs, bounds, contacts, ~np.array(near), set())
    empty = ot == 0
    assert empty.any() and (got["num_contacts"][empty] == 0).all() and (dlb[empty] == np.finfo(np.float64).max).all()
    assert np.isnan(got["normal"][empty]).all()
    for t in (1, 2, 3):
        assert (got["num_contacts"][ot == t] > 0).any(), t
    # the children of the inner node below the threshold are never reported (nodes 7, 8, 9 of the three-state tree in preorder)
    assert not {int(c["b1"]) for c in con if ot[c["pair"]] == 2} & {1, 2, 7, 8, 9}


def test_skipped_by_infinite_margin(harness):
    rng = np.random.default_rng(3)
    trees, L, solids = random_setup(rng)
    ot, sh, tft, tfs, sw = oc.random_queries(pkg, rng, trees, solids, 5)
    req = abi.default_collision_request()
    req.security_margin = -np.inf
    got, dlb, con, n_con, n_items = oc.harness_collide(pkg, harness, oc.HarnessTrees(pkg, trees), L, ot, sh, tft, tfs, req, sw, cap=8)
    assert n_con == 0 and n_items == 0 and (abi.status_skipped(got["status"]) == 1).all() and (got["num_contacts"] == 0).all()
    assert (dlb == np.finfo(np.float64).max).all()
    recs, bounds, contacts, _ = om.collide([om.Tree(*t) for t in trees], ot, L.shapes_array(), L.vertices_array(), sh, tft, tfs, req, sw)
    assert all(r["skipped"] for r in recs) and not contacts
    req.security_margin = -0.01
    with pytest.raises(ValueError):
        om.collide([om.Tree(*t) for t in trees], ot, L.shapes_array(), L.vertices_array(), sh, tft, tfs, req, sw)


def test_host_check_program(tmp_path):
    """the validator and the builder in a stand-alone program (tests/octree_harness/host_check.cpp), the form in which the two are run
    under a sanitizer"""
    import subprocess
    exe = str(tmp_path / "host_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                           "-o", exe, os.path.join(ROOT, "tests", "octree_harness", "host_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host_check ok" in r.stdout, r.stdout + r.stderr


def test_compat_surface_without_device():
    fcl = pkg.compat
    rng = np.random.default_rng(4)
    nodes = oc.random_tree(pkg, rng, 4)
    tree = fcl.OcTree(nodes, RESOLUTION, 4)
    assert tree.getTreeDepth() == 4 and tree.getResolution() == RESOLUTION and tree.size() == len(nodes) and tree.getNodeType() == abi.GEOM_OCTREE
    d = (1 << 4) * RESOLUTION / 2
    assert np.array_equal(tree.getRootBV(), [-d, -d, -d, d, d, d])
    for occ in (0.5, 0.9):
        tree.setOccupancyThres(occ)
        want = om.Tree(nodes, RESOLUTION, 4, occ, 0.0).to_boxes()
        got = tree.toBoxes()
        assert len(got) == len(want) > 0
        assert got.tobytes() == np.array([w[:6] for w in want]).tobytes()  # the halved boxes, in walk order
    tree.setFreeThres(0.2)
    assert tree.getFreeThres() == 0.2 and tree.getOccupancyThres() == 0.9
    with pytest.raises(ValueError):
        bad = nodes.copy()
        bad["child"][0][0] = len(nodes)
        fcl.OcTree(bad, RESOLUTION, 4)
    made = fcl.makeOctree(np.array([[0.1, 0.1, 0.1], [0.1, 0.1, 0.1], [-0.6, 0.3, 0.2]]), 0.25)
    assert made.getTreeDepth() == 16 and made.size() == 33 and len(made.toBoxes()) == 2
    assert sorted(made.toBoxes()[:, 4].tolist()) == [0.7, engine.octree_from_points(np.full((2, 3), 0.1), 0.25, 16)["occupancy"][0]]
    with pytest.raises(ValueError):
        fcl._check_pair(tree, fcl.Halfspace((0, 0, 1), 0.0), False)
    with pytest.raises(ValueError):
        fcl._check_pair(tree, tree, False)
    fcl._check_pair(fcl.Sphere(0.1), tree, False)
