"""OcTree x convex solid distance() (include/hppfcl_amd_octree_distance.h) without a GPU: the C ABI's host-only parts (exports, what the
header must say, the entry points without a device) and the device header built with g++ (tests/octree_distance_harness) against the
fp64 model (tests/octree_distance_model.py) on seeded random and hand-made trees.  The answer is the result of the reference's ORDERED
walk: the model and the harness are also held against the brute-force minimum over all reachable leaves, which the walk equals for six
kinds and exceeds for some Ellipsoids (computeBV<AABB, Ellipsoid> is R * radii without absolute values).

The request refusals (initial guess, epa_max_iterations, ids, evaluators) all come after the device check in the entry points, as in
every compute call of this library, so they are tested in tests/test_octree_distance_gpu.py."""
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
import octree_distance_cases as odc  # noqa: E402
import octree_distance_model as odm  # noqa: E402
import options_table  # noqa: E402

pkg = ge.load_pkg()
abi, engine, geometry = pkg.abi, pkg.engine, pkg.geometry

DBL_MAX = float(np.finfo(np.float64).max)
ELLIPSOID = 19
SEED = 11
N_RANDOM = 1200  # 300 queries for each (spread, signed)
BATCHES = ((0.7, True), (0.7, False), (1.5, True), (1.5, False))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return odc.build_harness(tmp_path_factory.mktemp("octree_distance_harness"))


# ---- 1. symbols, what the header must say ------------------------------------------------------------------------------------------
def test_symbols():
    lib = engine.dll()
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_octree_distance.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted(engine.OCTREE_DISTANCE_SYMBOLS) == ["hfcl_octree_distance_batch", "hfcl_octree_distance_batch_device",
                                                              "hfcl_octree_distance_pair_supported"]
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    older = (engine.EXPORTED_SYMBOLS + engine.CULL_SYMBOLS + engine.NEAREST_SYMBOLS + engine.PAIRS_SYMBOLS + engine.GROUPS_SYMBOLS +
             engine.NEAREST_SELF_SYMBOLS + engine.ENV_SYMBOLS + engine.NEAREST_ENV_SYMBOLS + engine.HFIELD_SYMBOLS + engine.TERRAIN_SYMBOLS +
             engine.OCTREE_SYMBOLS)
    assert not set(syms) & set(older)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert len(re.findall(r'#include "[./]*hppfcl_amd_octree_distance\.h"', main)) == 1
    assert lib.hfcl_abi_version() == 5
    for other in (9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 5, 18, 20, 21):  # GEOM_OCTREE stays unsupported in the per-pair matrix
        for for_distance in (0, 1):
            assert lib.hfcl_pair_supported(C.c_int32(abi.GEOM_OCTREE), C.c_int32(other), C.c_int(for_distance)) == 0
            assert lib.hfcl_pair_supported(C.c_int32(other), C.c_int32(abi.GEOM_OCTREE), C.c_int(for_distance)) == 0
    for t in (9, 10, 11, 12, 13, 14, 19):
        assert engine.octree_distance_pair_supported(t)
    for t in (15, 16, 17, 5, 0, 18, 20, 21, -1):
        assert not engine.octree_distance_pair_supported(t)
    assert set(engine.option_keys()) == set(options_table.TABLE) and len(engine.option_keys()) == len(options_table.TABLE)  # no key was added
    for m in ("octree_distance", "octree_distance_device"):
        assert hasattr(engine.Library, m), m
    # what the header must say
    assert "Not done:" in hdr
    assert "R * radii" in hdr and "without absolute values" in hdr and "reproduced on purpose" in hdr
    assert "n_nodes == 0" in hdr and "a choice" in hdr
    assert "rel_err" in hdr and "abs_err" in hdr and "not read" in hdr


# ---- 2. no device ------------------------------------------------------------------------------------------------------------------
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
    rc = d.hfcl_octree_distance_batch(None, abi.ptr(one), abi.ptr(one), abi.ptr(tf), abi.ptr(tf), C.c_size_t(1), None, C.byref(req), abi.ptr(out),
                                      abi.ptr(vis))
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    rc = d.hfcl_octree_distance_batch_device(None, None, None, None, None, C.c_size_t(1), None, C.byref(req), None, None, None)
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    assert (out == 0x5A).all() and vis[0] == 0x5A5A5A5A


# ---- 3. the harness against the model on random queries ----------------------------------------------------------------------------------
def records_against_model(got, got_visited, recs, visited, keep, needed):
    """Integers equal; floats bit-equal or within 1e-12 absolute (the tolerances of test_octree_cpu.records_against_model).  needed: the
    float fields that were not bit-equal somewhere."""
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


@pytest.fixture(scope="module")
def step3():
    """the 1 200 queries of test 3 and the model's answers, computed once: per batch a dict"""
    rng = np.random.default_rng(SEED)
    trees, L, solids = odc.random_setup(pkg, rng)
    trees = trees + [(oc.block_tree(pkg), odc.RESOLUTION, 4)]
    model_trees = [odm.Tree(*t) for t in trees]
    batches = []
    for spread, signed in BATCHES:
        ot, sh, tft, tfs, sw = oc.random_queries(pkg, rng, trees, solids, N_RANDOM // len(BATCHES), spread=spread)
        req = odc.request(abi, signed)
        recs, visited, near, leaves = odm.distance(model_trees, ot, L.shapes_array(), L.vertices_array(), sh, tft, tfs, req, sw)
        batches.append(dict(ot=ot, sh=sh, tft=tft, tfs=tfs, sw=sw, req=req, recs=recs, visited=visited, near=near, leaves=leaves, signed=signed))
    return dict(trees=trees, L=L, solids=solids, batches=batches)


def _walk_statistics(step3, distances, visited):
    """(kinds, separated share, most leaves solved by a query, mean visited share of the reachable leaves)"""
    kinds, sep, total, most, shares = set(), 0, 0, 0, []
    for b, dist, vis in zip(step3["batches"], distances, visited):
        types = step3["L"].shapes_array()["type"]
        kinds |= set(int(types[s]) for s in b["sh"])
        sep += int((np.asarray(dist) > 0).sum())
        total += len(b["sh"])
        most = max(most, int(max(vis)))
        shares += [v / len(lv) for v, lv in zip(vis, b["leaves"]) if lv]
    return kinds, sep / total, most, float(np.mean(shares))


def _assert_statistics(stats, who):
    kinds, separated, most, share = stats
    print("%s: kinds %s, separated %.3f, most leaves solved in a query %d, mean visited share %.3f" % (who, sorted(kinds), separated, most, share))
    assert len(kinds) == 7
    assert 0.2 < separated < 0.8
    assert most > 100
    assert share < 0.5  # pruning happens


def test_harness_equals_model_on_random_queries(harness, step3):
    ht = oc.HarnessTrees(pkg, step3["trees"])
    # the model alone meets the conditions
    _assert_statistics(_walk_statistics(step3, [[r["distance"] for r in b["recs"]] for b in step3["batches"]], [b["visited"] for b in step3["batches"]]),
                       "model")
    needed, rejected, total, both_orders, got_all = set(), 0, 0, set(), []
    for b in step3["batches"]:
        got, vis = odc.harness_distance(pkg, harness, ht, step3["L"], b["ot"], b["sh"], b["tft"], b["tfs"], b["req"], b["sw"])
        keep = ~np.array(b["near"])
        records_against_model(got, vis, b["recs"], b["visited"], keep, needed)
        rejected += int((~keep).sum())
        total += len(keep)
        both_orders |= set(int(s) for s in b["sw"])
        got_all.append((got, vis))
    print("random queries: %d, rejected near the running minimum %d; fields that needed the 1e-12 tolerance: %s" % (total, rejected, sorted(needed)))
    assert total == N_RANDOM and both_orders == {0, 1}
    assert rejected < 0.01 * total
    _assert_statistics(_walk_statistics(step3, [g["distance"] for g, _ in got_all], [v.tolist() for _, v in got_all]), "harness")


# ---- 4. hand-made trees ------------------------------------------------------------------------------------------------------------------
def test_hand_made_trees_equal_model(harness):
    """the empty tree, the root alone (the leaf branch of the recursion's first test), the three-state tree (free, uncertain, an inner node
    below the threshold), the deepest chain (the stack at its depth)"""
    rng = np.random.default_rng(2)
    trees = [(oc.empty_tree(pkg), odc.RESOLUTION, 3), (oc.tree_from_spec(pkg, oc.OCCUPIED), odc.RESOLUTION, 2),
             (oc.three_state_tree(pkg), odc.RESOLUTION, 2), (oc.chain_tree(pkg, 16), 0.001, 16)]
    L, solids = oc.seven_solids(pkg, rng)
    ht = oc.HarnessTrees(pkg, trees)
    model_trees = [odm.Tree(*t) for t in trees]
    ot, sh, tft, tfs, sw = oc.random_queries(pkg, rng, trees, solids, 200)
    ident = (tft.reshape(-1, 12) == geometry.make_pose().reshape(1, 12)).all(axis=1)
    assert 0 < ident.sum() < 200  # rotated and identity tree poses
    req = odc.request(abi, True)
    recs, visited, near, leaves = odm.distance(model_trees, ot, L.shapes_array(), L.vertices_array(), sh, tft, tfs, req, sw)
    got, vis = odc.harness_distance(pkg, harness, ht, L, ot, sh, tft, tfs, req, sw)
    records_against_model(got, vis, recs, visited, ~np.array(near), set())
    empty = ot == 0
    assert empty.any() and (got["distance"][empty] == DBL_MAX).all() and (vis[empty] == 0).all()
    assert (got["b1"][empty] == -1).all() and (got["b2"][empty] == -1).all()
    for k in ("normal", "p1", "p2"):
        assert np.isnan(got[k][empty]).all()
    root = ot == 1
    assert root.any() and (got["b1"][root] == 0).all() and (vis[root] == 1).all()
    assert not set(got["b1"][ot == 2].tolist()) & {1, 2, 7, 8, 9} and (got["b1"][ot == 2] >= 0).all()
    chain = ot == 3
    assert chain.any() and (vis[chain] >= 1).all() and len(set(got["b1"][chain].tolist())) > 1
    assert (got["b2"] == -1).all()


# ---- 5. the ordered walk is what is answered ---------------------------------------------------------------------------------------------
def ordered_walk_against_brute_force(distance, b1, kinds, leaves, skip, tol):
    """For every separated query (brute-force minimum over all reachable leaves > 0): distance >= the minimum; equal, with the DFS-first
    minimal leaf as b1, for every kind but Ellipsoid.  Returns (separated, Ellipsoid queries strictly above the minimum)."""
    separated = above = 0
    for i, lv in enumerate(leaves):
        if not lv or skip[i]:
            continue
        ds = [d for _, d in lv]
        m = min(ds)
        if not m > 0:
            continue
        separated += 1
        assert distance[i] >= m - tol, (i, distance[i], m)
        if kinds[i] != ELLIPSOID:
            assert abs(distance[i] - m) <= tol and b1[i] == lv[ds.index(m)][0], (i, kinds[i], distance[i], m)
        elif distance[i] > m + tol:
            above += 1
    return separated, above


def test_the_ordered_walk_is_what_is_answered(harness, step3):
    """On the model alone (exact: a minimum over a subset of the same numbers), then on the harness's records (whose floats test 3 holds
    within 1e-12 of the model's: that tolerance, and the queries test 3 leaves out, left out)."""
    ht = oc.HarnessTrees(pkg, step3["trees"])
    types = step3["L"].shapes_array()["type"]
    sep_m = above_m = sep_h = above_h = 0
    for b in step3["batches"]:
        kinds = [int(types[s]) for s in b["sh"]]
        s, a = ordered_walk_against_brute_force([r["distance"] for r in b["recs"]], [r["b1"] for r in b["recs"]], kinds, b["leaves"],
                                               [False] * len(kinds), 0.0)
        sep_m, above_m = sep_m + s, above_m + a
        got, _ = odc.harness_distance(pkg, harness, ht, step3["L"], b["ot"], b["sh"], b["tft"], b["tfs"], b["req"], b["sw"])
        s, a = ordered_walk_against_brute_force(got["distance"].tolist(), got["b1"].tolist(), kinds, b["leaves"], b["near"], 1e-12)
        sep_h, above_h = sep_h + s, above_h + a
    print("separated queries: model %d, harness %d; Ellipsoid queries above the brute-force minimum: model %d, harness %d" %
          (sep_m, sep_h, above_m, above_h))
    assert sep_m > 100 and above_m >= 1
    assert sep_h > 100 and above_h >= 1


# ---- 7. the walk in a stand-alone program ---------------------------------------------------------------------------------------------------
def test_host_check_program(tmp_path):
    """the walk on the deepest chain and on a full block in a stand-alone program (tests/octree_distance_harness/host_check.cpp), the form
    in which the header is run under a sanitizer: built with -fsanitize=address,undefined and executed directly"""
    exe = str(tmp_path / "host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-o", exe,
                           os.path.join(ROOT, "tests", "octree_distance_harness", "host_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host_check ok" in r.stdout, r.stdout + r.stderr
