"""The clearance per configuration on device-made pairs (include/hppfcl_amd_nearest_self.h) without a GPU: the exports and refusals;
the header (hpp-fcl_amd/csrc/hfcl_nearest_self.hpp) built with g++ (tests/nearest_self_harness) -- the bound from per-box terms
against nearest_bound bit for bit, and its sweeps in both forms, with and without groups and however the call is cut, against the
numpy model of tests/nearest_self_model.py byte for byte; the model against nearest_model.select on the explicit list of every allowed
pair; and the model's answer against the fold over all pairs, with the share of the candidates it evaluates."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nearest_model
import nearest_self_model as model
import pairs_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
FILL32, FILL64 = 0xABABABAB, 0xABABABABABABABAB


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nearest_self_harness") / "libnearest_self_harness.so")
    src = os.path.join(ROOT, "tests", "nearest_self_harness", "nearest_self_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-o", out, src])
    d = C.CDLL(out)
    d.nsh_sweep.restype = C.c_uint64
    d.nsh_sizes.restype = C.c_uint64
    return d


_SCENES = {}


def _robot(pkg, oracle, key):
    """scene_robot_env(*key, seed 1): the scene, its groups, the explicit list P, the host's boxes and the oracle's distance records on P
    (default request).  Computed once, not modified."""
    if key not in _SCENES:
        n_conf, n_links, n_obstacles, spread = key
        ps, groups, P = pkg.workloads.scene_robot_env(n_conf, n_links, n_obstacles, seed=1, spread=spread)
        boxes = np.stack([pkg.engine.world_aabbs(ps.lib, ps.obj_shape, ps.obj_tf[c]) for c in range(n_conf)])
        b = ps.expand()
        rec = oracle.distance_batch(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, pkg.abi.default_distance_request(), n_threads=8)
        _SCENES[key] = (ps, groups, P, boxes, rec)
    return _SCENES[key]


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings(pkg, harness):
    pkg.engine.build_native()
    lib = pkg.engine.dll()
    e = pkg.engine
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_nearest_self.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted(e.NEAREST_SELF_SYMBOLS) == ["hfcl_scene_nearest_self", "hfcl_scene_nearest_self_device",
                                                      "hfcl_scene_nearest_self_device_f32", "hfcl_scene_nearest_self_f32"]
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    assert not set(syms) & set(e.EXPORTED_SYMBOLS + e.CULL_SYMBOLS + e.NEAREST_SYMBOLS + e.PAIRS_SYMBOLS + e.GROUPS_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert main.count('#include "hppfcl_amd_nearest_self.h"') == 1
    assert main.index('#include "hppfcl_amd_nearest_self.h"') < main.index('#include "hppfcl_amd_pairs.h"')
    assert "hfcl_scene_nearest_self" not in main
    assert lib.hfcl_abi_version() == 5
    for m in ("nearest_self", "nearest_self_device", "nearest_self_device_f32"):
        assert hasattr(e.Scene, m), m
    assert pkg.abi.SCENE_CLEARANCE_DTYPE.itemsize == 24 == harness.nsh_sizes(0) and harness.nsh_sizes(1) == 16
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd.h")])
    src = "#include <stddef.h>\n#include \"hppfcl_amd.h\"\ntypedef char is_24[sizeof(hfcl_scene_clearance) == 24 ? 1 : -1];\n" \
          "typedef char at_8[offsetof(hfcl_scene_clearance, min_i) == 8 ? 1 : -1];\n"
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode(), check=True)


def test_refusals(pkg):
    """No CPU fallback: without a device every entry point says so.  With one: a NaN bound, a null scene -- whatever the bound --, and
    (tests/test_scene_nearest_self_gpu.py, which has a scene) a null output are invalid arguments.  Nothing is written."""
    d, abi = pkg.engine.dll(), pkg.abi
    req = abi.default_distance_request()
    tf = np.zeros((2, 12))
    out = np.full(24, 0x5A, dtype=np.uint8).view(abi.SCENE_CLEARANCE_DTYPE)
    before = out.tobytes()
    n = (C.c_size_t * 2)(7, 7)
    n1 = C.c_size_t(1)
    no_device = pkg.engine.device_count() == 0
    for bound, word in ((np.inf, "null scene"), (0.5, "null scene"), (np.nan, "upper_bound")):
        calls = [
            (d.hfcl_scene_nearest_self, (None, abi.ptr(tf), n1, C.byref(req), C.c_double(bound), abi.ptr(out), None, n)),
            (d.hfcl_scene_nearest_self_f32, (None, None, n1, C.byref(req), C.c_double(bound), abi.ptr(out), None, n)),
            (d.hfcl_scene_nearest_self_device, (None, None, n1, C.byref(req), C.c_double(bound), None, None, n, None)),
            (d.hfcl_scene_nearest_self_device_f32, (None, None, n1, C.byref(req), C.c_double(bound), None, None, n, None)),
        ]
        assert sorted(fn.__name__ for fn, _ in calls) == sorted(pkg.engine.NEAREST_SELF_SYMBOLS)
        for fn, args in calls:
            assert fn(*args) == (abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT), fn.__name__
            assert ("no CPU fallback" if no_device else word) in pkg.engine.last_error(), (fn.__name__, pkg.engine.last_error())
    assert out.tobytes() == before and tuple(n) == (7, 7)


# ---- 2. the bound in per-box parts ----------------------------------------------------------------------------------------------------
def _both_bounds(harness, pkg, a, b, r):
    a, b = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 6), np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 6)
    plain, terms = np.full(len(a), np.nan), np.full(len(a), np.nan)
    harness.nsh_bounds(pkg.abi.ptr(a), pkg.abi.ptr(b), C.c_uint64(len(a)), C.c_double(r), pkg.abi.ptr(plain), pkg.abi.ptr(terms))
    return plain, terms


def test_bound_from_terms_is_the_bound_bit_for_bit(pkg, harness):
    rng = np.random.default_rng(29)
    big = np.finfo(np.float64).max
    n = 100_000
    scale = 10.0 ** rng.integers(-3, 6, (n, 1))
    lo_a, lo_b = rng.uniform(-4, 4, (n, 3)) * scale, rng.uniform(-4, 4, (n, 3)) * scale
    a = np.concatenate([lo_a, lo_a + rng.uniform(0.0, 1.0, (n, 3)) * scale], axis=1)
    b = np.concatenate([lo_b, lo_b + rng.uniform(0.0, 1.0, (n, 3)) * scale], axis=1)
    unit = np.array([0, 0, 0, 1, 1, 1.0])
    hand = [
        (unit, unit + [1, 0, 0, 1, 0, 0]), (unit, unit), (unit, unit + [1, 1, 1, 1, 1, 1]),          # touching: a face, all, a corner
        (unit, np.array([3, 0.5, 0.5, 3, 0.5, 0.5])), (unit, np.array([3, 4, 0.5, 3, 4, 0.5])),
        (unit, np.array([3, np.nan, 0, 4, 1, 1])), (np.array([np.nan] * 6), unit), (np.array([np.nan] * 6), np.array([np.nan] * 6)),
        (unit, np.array([2, 2, 2, np.inf, 3, 3])), (np.array([-np.inf, 0, 0, 1, 1, 1]), unit + 5), (unit, np.array([2, 2, 2, 3, 3, -np.inf])),
        (unit, np.array([-big, -big, 5, big, big, 5])), (np.array([-big] * 3 + [big] * 3), unit + 5),  # Plane, unbounded
        (unit, np.array([-big, 2, -big, big, big, big])),                                             # Halfspace: its diagonal overflows
        (unit, unit + 1e150), (unit - big / 2, unit + big / 2), (np.array([-big] * 6), np.array([big] * 6)),  # L or its parts overflow
        (unit * 1e300, unit * 1e300 + [0, 0, 3e300, 0, 0, 3e300]), (unit * 1e160, -unit[[3, 4, 5, 0, 1, 2]] * 1e160 - 1e160),
        (unit * 0.0, unit * 0.0 + 1e-300), (unit * 0.0, unit * 0.0 - 0.0),
    ]
    a = np.concatenate([a, np.stack([h[0] for h in hand]), np.stack([h[1] for h in hand])])
    b = np.concatenate([b, np.stack([h[1] for h in hand]), np.stack([h[0] for h in hand])])
    for r in (nearest_model.R64, nearest_model.R32):
        plain, terms = _both_bounds(harness, pkg, a, b, r)
        assert terms.tobytes() == plain.tobytes()
        assert plain.tobytes() == nearest_model.bound(a, b, r).tobytes()  # ... and both are the definition
        assert np.isneginf(plain[:n]).any() and np.isfinite(plain[:n]).any() and np.isneginf(plain[n:]).sum() >= 2 * 12


# ---- 3. the header's sweeps against the model -----------------------------------------------------------------------------------------
def _header_run(harness, pkg, boxes, groups, records, D, r, chunk_rows, small_max):
    """The whole call on the host: seeds, the list of pass 1, its ranked fold, thresholds, the list of pass 2, its fold, the combination."""
    abi = pkg.abi
    n_conf, n = boxes.shape[:2]
    P = model.explicit_list(n, groups)
    index = np.full((n, n), -1, dtype=np.int64)
    index[P[:, 0], P[:, 1]] = np.arange(len(P))
    b = np.ascontiguousarray(boxes)
    grp = np.ascontiguousarray(groups[0], dtype=np.uint8) if groups is not None else None
    col = np.zeros(64, dtype=np.uint64)
    if groups is not None:
        col[:len(groups[1])] = groups[1]
    seed = np.full(n_conf, FILL64, dtype=np.uint64)
    thr = np.full(n_conf, np.nan)
    cap = max(n_conf * len(P), 1)

    def sweep(mode, pairs, cb):
        return harness.nsh_sweep(abi.ptr(b), C.c_uint32(n), C.c_uint64(n_conf), abi.ptr(grp), abi.ptr(col) if groups is not None else None,
                                 C.c_double(r), C.c_double(D), C.c_int(mode), C.c_uint64(chunk_rows), C.c_uint32(small_max), abi.ptr(seed),
                                 abi.ptr(thr), abi.ptr(pairs), C.c_uint64(cap if pairs is not None else 0), abi.ptr(cb))

    sweep(0, None, None)
    out = dict(seed=seed.copy())
    sums, recs = [], []
    for l in (1, 2):
        pairs = np.full((cap + 3, 2), FILL32, dtype=np.uint32)  # (three guard entries)
        cb = np.full(n_conf + 1, FILL64, dtype=np.uint64)
        k = sweep(l, pairs, cb)
        assert np.all(pairs[k:] == FILL32) and cb[-1] == k
        assert sweep(l, None, np.zeros(n_conf + 1, dtype=np.uint64)) == k  # (the count alone)
        pairs = np.ascontiguousarray(pairs[:k])
        rec = records[pairs_model.conf_of(cb) * len(P) + index[pairs[:, 0], pairs[:, 1]]]
        assert np.all(index[pairs[:, 0], pairs[:, 1]] >= 0)
        summ = pairs_model.fold_ranked(abi, rec, cb)
        if l == 1:
            harness.nsh_threshold(abi.ptr(summ), C.c_uint64(n_conf), C.c_double(D), abi.ptr(thr))
            out["thr"] = thr.copy()
        out["pairs%d" % l], out["conf_begin%d" % l] = pairs, cb
        sums.append(summ)
        recs.append(np.ascontiguousarray(rec))
    clear = np.full(n_conf * 24, 0xAB, dtype=np.uint8).view(abi.SCENE_CLEARANCE_DTYPE)
    mins = np.full(n_conf * 96, 0xAB, dtype=np.uint8).view(abi.RESULT_DTYPE)
    harness.nsh_combine(C.c_uint64(n_conf), abi.ptr(sums[0]), abi.ptr(sums[1]), abi.ptr(out["pairs1"]), abi.ptr(out["pairs2"]),
                        abi.ptr(out["conf_begin1"]), abi.ptr(out["conf_begin2"]), abi.ptr(recs[0]), abi.ptr(recs[1]), abi.ptr(clear), abi.ptr(mins))
    out["clearance"], out["min_records"] = clear, mins
    return out


KEYS = ("seed", "pairs1", "conf_begin1", "thr", "pairs2", "conf_begin2", "clearance", "min_records")


def _synthetic(pkg, n, with_groups, n_conf=3):
    """Random boxes, in all configurations but the first a tenth of them on one spot; records whose distance lies above the bound (or
    below 0 where there is none)."""
    rng = np.random.default_rng([41, n, int(with_groups)])
    side = 1.2 * n ** (1.0 / 3.0)
    lo = rng.uniform(-side, side, (n_conf, n, 3))
    lo[1:, rng.random(n) < 0.1] = 0.25
    g, k = int(np.ceil(n ** (1.0 / 3.0))), np.arange(n)  # the first: a jittered lattice wider than any box -- no pair touches, many are near
    lo[0] = 1.3 * np.stack([k % g, (k // g) % g, k // (g * g)], axis=1) + rng.uniform(0.0, 0.1, (n, 3))
    boxes = np.concatenate([lo, lo + rng.uniform(0.1, 1.0, (n_conf, n, 3))], axis=-1)
    if n_conf > 2:
        boxes[2] = boxes[1]  # (two configurations with the same bounds)
    groups = None
    if with_groups:
        g = rng.integers(0, 3, n).astype(np.uint8)
        g[: n // 4] = 2  # (a run of rows that may pair with little: whole blocks and tiles are skipped)
        groups = (g, np.array([0b011, 0b101, 0b010], dtype=np.uint64))  # 0-0, 0-1, 1-2: symmetric; no 2-2, no 0-2, no 1-1
    P = model.explicit_list(n, groups)
    L = nearest_model.query_bounds(boxes, P) if len(P) else np.zeros((n_conf, 0))
    rec = np.zeros(L.size, dtype=pkg.abi.RESULT_DTYPE)
    rec["distance"] = np.where(np.isfinite(L), L + rng.uniform(0.2, 0.7, L.shape), -rng.uniform(0, 1, L.shape)).reshape(-1)
    rec["b1"] = np.arange(L.size)  # (a record names its query)
    return boxes, groups, P, rec


@pytest.mark.parametrize("with_groups", [False, True])
@pytest.mark.parametrize("n", [2, 3, 33, 63, 64, 65, 257])
def test_header_sweeps_equal_the_model(pkg, harness, n, with_groups):
    boxes, groups, P, rec = _synthetic(pkg, n, with_groups)
    for D in (np.inf, 0.5):
        exp = model.select(pkg.abi, boxes, groups, rec, D)
        if n >= 33:
            assert len(exp["pairs1"]) > 0 and len(exp["pairs2"]) > 0
        forms = ((0, 64), (1, 64), (37, 64), (0, 0), (37, 0)) if n <= 64 else ((0, 64), (1, 64), (37, 64))
        for chunk_rows, small_max in forms:
            got = _header_run(harness, pkg, boxes, groups, rec, D, nearest_model.R64, chunk_rows, small_max)
            for k in KEYS:
                assert got[k].dtype == exp[k].dtype and got[k].tobytes() == exp[k].tobytes(), (k, chunk_rows, small_max, D)


def test_header_sweeps_on_the_robot_scene_of_306_objects(pkg, oracle, harness):
    """Two column tiles, groups, the oracle's records."""
    ps, groups, P, boxes, rec = _robot(pkg, oracle, (4, 6, 300, 3.0))
    assert boxes.shape[1] == 306 > harness.nsh_sizes(2)
    for r in (nearest_model.R64, nearest_model.R32):
        exp = model.select(pkg.abi, boxes, groups, rec, np.inf, r)
        for chunk_rows in (0, 1, 37):
            got = _header_run(harness, pkg, boxes, groups, rec, np.inf, r, chunk_rows, 64)
            for k in KEYS:
                assert got[k].tobytes() == exp[k].tobytes(), (k, chunk_rows)


def test_configurations_without_a_candidate(pkg, harness):
    """One object; groups that allow no pair: no seed, empty lists, the clearance of a configuration without records."""
    abi = pkg.abi
    boxes, _, _, _ = _synthetic(pkg, 65, False)
    none = (np.zeros(65, dtype=np.uint8), np.array([0], dtype=np.uint64))
    rec = np.zeros(0, dtype=abi.RESULT_DTYPE)
    for b, groups, small_max in ((boxes[:, :1], None, 64), (boxes, none, 64), (boxes[:, :40], (none[0][:40], none[1]), 64), (boxes[:, :40], (none[0][:40], none[1]), 0)):
        exp = model.select(abi, b, groups, rec)
        got = _header_run(harness, pkg, b, groups, rec, np.inf, nearest_model.R64, 0, small_max)
        for k in KEYS:
            assert got[k].tobytes() == exp[k].tobytes(), k
        assert np.all(got["seed"] == model.NO_PAIR) and np.all(np.isposinf(got["clearance"]["min_distance"]))
        assert np.all(got["clearance"]["min_i"] == NONE) and np.all(got["clearance"]["n_evaluated"] == 0)
        assert np.all(got["min_records"]["status"] == 0x80000000) and np.all(np.isposinf(got["min_records"]["distance"]))


# ---- 4. the model against the definition already proven: nearest_model.select on the explicit list ---------------------------------------
def _check_model_against_list(abi, boxes, groups, P, rec, D, r=nearest_model.R64):
    sel = model.select(abi, boxes, groups, rec, D, r)
    old = nearest_model.select(abi, nearest_model.query_bounds(boxes, P, r), rec, D)
    n_pairs = len(P)
    key = lambda ij: (ij[:, 0].astype(np.uint64) << np.uint64(32)) | ij[:, 1].astype(np.uint64)  # noqa: E731
    assert np.array_equal(sel["seed"], key(P[old["seed"].astype(np.int64)]))
    assert sel["thr"].tobytes() == old["thr"].tobytes()
    for l in ("1", "2"):
        ids = old["ids" + l].astype(np.int64)
        assert sel["conf_begin" + l].tobytes() == old["conf_begin" + l].tobytes()
        assert np.array_equal(sel["pairs" + l], P[ids % n_pairs])
        assert np.array_equal(pairs_model.conf_of(sel["conf_begin" + l]), ids // n_pairs)
    s, clear = old["summary"], sel["clearance"]
    assert clear["min_distance"].tobytes() == s["min_distance"].tobytes()
    has = s["min_pair"] != NONE
    assert np.array_equal(clear["min_i"][has], P[s["min_pair"][has].astype(np.int64), 0])
    assert np.array_equal(clear["min_j"][has], P[s["min_pair"][has].astype(np.int64), 1])
    assert np.all(clear["min_i"][~has] == NONE) and np.all(clear["min_j"][~has] == NONE)
    assert np.array_equal(clear["n_skipped"], s["n_skipped"])
    assert np.array_equal(clear["n_evaluated"], np.diff(old["conf_begin1"].astype(np.int64)) + np.diff(old["conf_begin2"].astype(np.int64)))
    return sel


@pytest.mark.parametrize("with_groups", [False, True])
def test_model_equals_the_selection_on_the_explicit_list(pkg, oracle, with_groups):
    for n in (3, 33, 65):
        boxes, groups, P, rec = _synthetic(pkg, n, with_groups)
        for D in (np.inf, 0.5, 0.05):
            _check_model_against_list(pkg.abi, boxes, groups, P, rec, D)
    ps, groups, P, boxes, rec = _robot(pkg, oracle, (8, 6, 40, 3.0))
    assert np.array_equal(P, model.explicit_list(boxes.shape[1], groups))  # (the workload's list is the model's)
    for D in (np.inf, 0.5, 0.05):
        _check_model_against_list(pkg.abi, boxes, groups, P, rec, D)


# ---- 5. exactness and shares of the model with the oracle's records ---------------------------------------------------------------------
# scene -> (candidates per configuration x configurations, % evaluated in pass 1, in pass 2, cap on their sum in %)
COUNTED = {
    (8, 6, 40, 3.0): (2000, 0.45, 1.20, 5.0),
    (8, 6, 100, 3.0): (4880, 0.31, 0.33, 5.0),
    (4, 6, 300, 3.0): (7240, 0.07, 0.10, 5.0),
    (8, 12, 300, 1.0): (29240, 1.17, 0.00, None),  # dense: the pass-2-empty case
    (8, 6, 20, 3.0): (1040, None, None, 25.0),     # the small form
}


@pytest.mark.parametrize("key", sorted(COUNTED))
def test_model_is_exact_and_evaluates_a_small_share(pkg, oracle, key):
    candidates, want1, want2, cap = COUNTED[key]
    ps, groups, P, boxes, rec = _robot(pkg, oracle, key)
    sel = _check_model_against_list(pkg.abi, boxes, groups, P, rec, np.inf)
    assert model.check_against_full(pkg.abi, sel, P, rec) == 0
    total = key[0] * len(P)
    s1, s2 = 100.0 * len(sel["pairs1"]) / total, 100.0 * len(sel["pairs2"]) / total
    hit = int((sel["clearance"]["min_distance"] <= 0).sum())
    print("scene_robot_env%r: %d candidates, %.2f %% evaluated in pass 1, %.2f %% in pass 2, %d configurations in collision" % (key, total, s1, s2, hit))
    assert total == candidates
    if want1 is not None:
        assert (round(s1, 2), round(s2, 2)) == (want1, want2)
    if cap is not None:
        assert s1 + s2 <= cap


@pytest.mark.parametrize("D", [0.5, 0.05])
def test_model_with_an_upper_bound(pkg, oracle, D):
    ps, groups, P, boxes, rec = _robot(pkg, oracle, (8, 6, 40, 3.0))
    sel = model.select(pkg.abi, boxes, groups, rec, D)
    beyond = model.check_against_full(pkg.abi, sel, P, rec, D)
    assert 0 < beyond < 8
    unbounded = model.select(pkg.abi, boxes, groups, rec, np.inf)
    assert len(sel["pairs1"]) + len(sel["pairs2"]) < len(unbounded["pairs1"]) + len(unbounded["pairs2"])


# ---- 6. the C++ shim ------------------------------------------------------------------------------------------------------------------
def test_shim_method_compiles(tmp_path):
    src = tmp_path / "shim.cpp"
    src.write_text('#include "hppfcl_amd_compat.hpp"\n'
                   "void use(hpp::fcl::amd::Scene& s, const hpp::fcl::Transform3f* t, std::vector<hfcl_scene_clearance>& c, "
                   "std::vector<hpp::fcl::DistanceResult>& m) { size_t n[2]; s.nearestSelf(t, 1, hpp::fcl::DistanceRequest(), 0.5, c, &m, n); "
                   "s.nearestSelf(t, 1, hpp::fcl::DistanceRequest(), 1.0 / 0.0, c); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
