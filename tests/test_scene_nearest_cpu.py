"""The per-configuration minimum distance with box-bound pruning (include/hppfcl_amd_nearest.h) without a GPU: the exports and
refusals; the header (hpp-fcl_amd/csrc/hfcl_nearest.hpp) built with g++ (tests/nearest_harness) -- its bound and its two lists against
the numpy model of tests/nearest_model.py, bit for bit; the bound against the oracle's distances (it must lie below every one of them);
and the model's answer against the fold over all pairs, with the share of the queries it evaluates."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nearest_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
FILL = 0xABABABABABABABAB


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nearest_harness") / "libnearest_harness.so")
    src = os.path.join(ROOT, "tests", "nearest_harness", "nearest_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-o", out, src])
    d = C.CDLL(out)
    d.nh_r.restype = C.c_double
    return d


_SCENES = {}


def _scene(pkg, oracle, n_conf, n_obj):
    """scene_planner(n_conf, n_obj, seed 1), its host boxes and the oracle's distance records (default request): computed once, not modified."""
    key = (n_conf, n_obj)
    if key not in _SCENES:
        ps = pkg.workloads.scene_planner(n_conf, n_obj, seed=1)
        tf = ps.obj_tf
        boxes = np.stack([pkg.engine.world_aabbs(ps.lib, ps.obj_shape, tf[c]) for c in range(n_conf)])
        b = ps.expand()
        rec = oracle.distance_batch(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, pkg.abi.default_distance_request(), n_threads=8)
        _SCENES[key] = (ps, boxes, rec, pkg.abi.fold_records(rec, len(ps.pairs), None))
    return _SCENES[key]


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings(pkg):
    pkg.engine.build_native()
    lib = pkg.engine.dll()
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_nearest.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted(pkg.engine.NEAREST_SYMBOLS) == ["hfcl_scene_nearest", "hfcl_scene_nearest_device", "hfcl_scene_nearest_device_f32",
                                                          "hfcl_scene_nearest_f32"]
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    assert not set(syms) & set(pkg.engine.EXPORTED_SYMBOLS) and not set(syms) & set(pkg.engine.CULL_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert main.count('#include "hppfcl_amd_nearest.h"') == 1 and "hfcl_scene_nearest" not in main.replace("hppfcl_amd_nearest.h", "")
    assert lib.hfcl_abi_version() == 5
    for m in ("nearest", "nearest_f32", "nearest_device", "nearest_device_f32"):
        assert hasattr(pkg.engine.Scene, m), m
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd.h")])


def test_null_scene_and_nan_bound_are_refused(pkg):
    d, abi = pkg.engine.dll(), pkg.abi
    req = abi.default_distance_request()
    tf = np.zeros((2, 12))
    summ = np.full(1, 0x5A, dtype=np.uint8).repeat(24).view(abi.SCENE_SUMMARY_DTYPE)
    n = (C.c_size_t * 2)(7, 7)
    before = summ.tobytes()
    n1 = C.c_size_t(1)
    for bound, word in ((np.inf, "null scene"), (0.5, "null scene"), (np.nan, "upper_bound")):
        calls = [
            (d.hfcl_scene_nearest, (None, abi.ptr(tf), n1, C.byref(req), C.c_double(bound), abi.ptr(summ), None, n)),
            (d.hfcl_scene_nearest_f32, (None, None, n1, C.byref(req), C.c_double(bound), abi.ptr(summ), None, n)),
            (d.hfcl_scene_nearest_device, (None, None, n1, C.byref(req), C.c_double(bound), None, None, n, None)),
            (d.hfcl_scene_nearest_device_f32, (None, None, n1, C.byref(req), C.c_double(bound), None, None, n, None)),
        ]
        assert sorted(fn.__name__ for fn, _ in calls) == sorted(pkg.engine.NEAREST_SYMBOLS)
        for fn, args in calls:
            assert fn(*args) == abi.ERR_INVALID_ARGUMENT, fn.__name__
            assert word in pkg.engine.last_error(), (fn.__name__, pkg.engine.last_error())
    assert summ.tobytes() == before and tuple(n) == (7, 7)  # (a refused call writes nothing)


# ---- 2. the bound -------------------------------------------------------------------------------------------------------------------
def _header_bound(harness, pkg, a, b, r):
    a, b = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 6), np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 6)
    out = np.full(len(a), np.nan)
    harness.nh_bound(pkg.abi.ptr(a), pkg.abi.ptr(b), C.c_uint64(len(a)), C.c_double(r), pkg.abi.ptr(out))
    return out


def test_header_bound_equals_the_model(pkg, oracle, harness):
    assert harness.nh_r(0) == nearest_model.R64 == 2.0 ** -40 and harness.nh_r(1) == nearest_model.R32 >= 2.0 ** -18
    ps, boxes, _, _ = _scene(pkg, oracle, 64, 16)
    a, b = boxes[:, ps.pairs[:, 0]], boxes[:, ps.pairs[:, 1]]
    for r in (nearest_model.R64, nearest_model.R32):
        exp = nearest_model.query_bounds(boxes, ps.pairs, r)
        got = _header_bound(harness, pkg, a, b, r).reshape(exp.shape)
        assert got.tobytes() == exp.tobytes()
        assert np.isneginf(exp).any() and np.isfinite(exp).any() and (exp[np.isfinite(exp)] > 0).any()
    # ... and the model is the definition, box by box
    big = np.finfo(np.float64).max
    unit = np.array([0, 0, 0, 1, 1, 1.0])
    hand = [
        (unit, unit + [1, 0, 0, 1, 0, 0], -np.inf),                    # a shared face: closed intervals
        (unit, unit, -np.inf),                                         # identical boxes
        (unit, np.array([3, 0.5, 0.5, 3, 0.5, 0.5]), None),            # a zero-extent box, 2 away along x
        (unit, np.array([3, 4, 0.5, 3, 4, 0.5]), None),                # ... 2 along x and 3 along y
        (unit, np.array([3, np.nan, 0, 4, 1, 1]), -np.inf),            # a NaN coordinate
        (np.array([np.nan] * 6), unit, -np.inf),
        (unit, np.array([-big, -big, 5, big, big, 5]), -np.inf),       # a Plane aligned with z: unbounded along x and y
        (np.array([-big] * 3 + [big] * 3), unit + 5, -np.inf),
        (unit, np.array([-big, 2, -big, big, big, big]), -np.inf),     # a Halfspace: separated along y, its diagonal overflows
        (unit, unit + 1e150, None),                                    # finite and far
        (unit, np.array([2, 2, 2, np.inf, 3, 3]), -np.inf),
    ]
    a, b = np.stack([h[0] for h in hand]), np.stack([h[1] for h in hand])
    exp = nearest_model.bound(a, b)
    got = _header_bound(harness, pkg, a, b, nearest_model.R64)
    assert got.tobytes() == exp.tobytes()
    for k, (_, _, want) in enumerate(hand):
        if want is not None:
            assert exp[k] == want, k
    slack = lambda e, M: 2e-10 * e + 2.0 ** -40 * M  # noqa: E731
    assert exp[2] == 2.0 - slack(np.sqrt(3.0), 3.0) and exp[3] == np.sqrt(13.0) - slack(np.sqrt(3.0), 4.0) and np.isfinite(exp[9])
    # symmetric in the two boxes
    assert _header_bound(harness, pkg, b, a, nearest_model.R64).tobytes() == exp.tobytes()


# ---- 3. the selection ---------------------------------------------------------------------------------------------------------------
def _header_select(harness, pkg, boxes, pairs, records, D, r, chunk):
    abi = pkg.abi
    n_conf, n_obj = boxes.shape[:2]
    total = n_conf * len(pairs)
    out = dict(seed=np.full(n_conf, 0xABABABAB, dtype=np.uint32), ids1=np.full(total, FILL, dtype=np.uint64),
               conf_begin1=np.full(n_conf + 1, FILL, dtype=np.uint64), thr=np.full(n_conf, np.nan), ids2=np.full(total, FILL, dtype=np.uint64),
               conf_begin2=np.full(n_conf + 1, FILL, dtype=np.uint64), summary=np.zeros(n_conf, dtype=abi.SCENE_SUMMARY_DTYPE))
    n = (C.c_uint64 * 2)()
    b, p, rec = np.ascontiguousarray(boxes), np.ascontiguousarray(pairs, dtype=np.uint32), np.ascontiguousarray(records)
    harness.nh_select(abi.ptr(b), abi.ptr(p), C.c_uint32(len(p)), C.c_uint64(n_obj), C.c_uint64(n_conf), C.c_double(D), C.c_double(r),
                      abi.ptr(rec), C.c_uint64(chunk), abi.ptr(out["seed"]), abi.ptr(out["ids1"]), abi.ptr(out["conf_begin1"]),
                      abi.ptr(out["thr"]), abi.ptr(out["ids2"]), abi.ptr(out["conf_begin2"]), abi.ptr(out["summary"]), n)
    assert np.all(out["ids1"][n[0]:] == FILL) and np.all(out["ids2"][n[1]:] == FILL)
    out["ids1"], out["ids2"] = out["ids1"][:n[0]], out["ids2"][:n[1]]
    return out


@pytest.mark.parametrize("D", [np.inf, 0.5, 0.05])
def test_header_selection_equals_the_model(pkg, oracle, harness, D):
    """The oracle's distances stand for the records: seeds, the list of pass 1, thresholds, the list of pass 2 and the summaries, however
    the flat range is cut."""
    ps, boxes, rec, _ = _scene(pkg, oracle, 64, 16)
    L = nearest_model.query_bounds(boxes, ps.pairs)
    exp = nearest_model.select(pkg.abi, L, rec, D)
    total = 64 * len(ps.pairs)
    assert total == 6720 and len(exp["ids1"]) > 0 and len(exp["ids2"]) > 0
    assert not np.intersect1d(exp["ids1"], exp["ids2"]).size
    for chunk in (total, 1000, 256, 105, 63, 1):
        got = _header_select(harness, pkg, boxes, ps.pairs, rec, D, nearest_model.R64, chunk)
        for k in ("seed", "ids1", "conf_begin1", "thr", "ids2", "conf_begin2", "summary"):
            assert got[k].dtype == exp[k].dtype and got[k].tobytes() == exp[k].tobytes(), (k, chunk)


def test_header_selection_of_a_long_pair_list(pkg, harness):
    """A pair list of several fold pieces (700 pairs): the seed goes through partials; synthetic boxes and records."""
    abi = pkg.abi
    rng = np.random.default_rng(17)
    n_conf, n_obj = 5, 40
    lo = rng.uniform(-4, 4, (n_conf, n_obj, 3))
    boxes = np.concatenate([lo, lo + rng.uniform(0.1, 1.0, (n_conf, n_obj, 3))], axis=-1)
    boxes[2] = boxes[1]  # (two configurations with the same bounds)
    i, j = np.triu_indices(n_obj, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)[:700]
    L = nearest_model.query_bounds(boxes, pairs)
    rec = np.zeros(L.size, dtype=abi.RESULT_DTYPE)
    rec["distance"] = np.where(np.isfinite(L), L + rng.uniform(0.0, 0.7, L.shape), -rng.uniform(0, 1, L.shape)).reshape(-1)
    exp = nearest_model.select(abi, L, rec, np.inf)
    assert (exp["seed"] >= 256).any()
    for chunk in (L.size, 257):
        got = _header_select(harness, pkg, boxes, pairs, rec, np.inf, nearest_model.R64, chunk)
        for k in ("seed", "ids1", "conf_begin1", "thr", "ids2", "conf_begin2", "summary"):
            assert got[k].tobytes() == exp[k].tobytes(), (k, chunk)
    full = abi.fold_records(rec, 700, None)
    assert nearest_model.check_against_full(exp["summary"], full) == 0
    # the gather: every configuration's minimum is found in one of the two lists, at the position of its id
    where = np.zeros(n_conf, dtype=np.uint64)
    harness.nh_gather(abi.ptr(exp["summary"]), C.c_uint64(n_conf), C.c_uint32(700), abi.ptr(exp["ids1"]), abi.ptr(exp["conf_begin1"]),
                      abi.ptr(exp["ids2"]), abi.ptr(exp["conf_begin2"]), abi.ptr(where))
    for c in range(n_conf):
        q = c * 700 + int(exp["summary"]["min_pair"][c])
        lst = exp["ids2"] if int(where[c]) >> 63 else exp["ids1"]
        assert int(lst[int(where[c]) & (2 ** 63 - 1)]) == q, c
    r, r32 = np.zeros(1, dtype=abi.RESULT_DTYPE), np.zeros(1, dtype=abi.RESULT_F32_DTYPE)
    harness.nh_no_record(abi.ptr(r), abi.ptr(r32))
    for x in (r, r32):
        assert np.isposinf(x["distance"][0]) and x["status"][0] == 0x80000000


# ---- 4. L is a lower bound of the oracle's distance ------------------------------------------------------------------------------------
def test_bound_lies_below_the_oracle_distance_in_the_planner_scenes(pkg, oracle):
    for n_conf, n_obj in ((64, 16), (256, 32)):
        ps, boxes, rec, _ = _scene(pkg, oracle, n_conf, n_obj)
        L = nearest_model.query_bounds(boxes, ps.pairs).reshape(-1)
        d = rec["distance"]
        assert np.all(np.isfinite(d)) and np.all(L <= d)
        fin = np.isfinite(L)
        print("scene_planner(%d, %d): %d of %d queries have a bound; smallest distance - L = %.3g" % (n_conf, n_obj, fin.sum(), len(L), (d - L)[fin].min()))


def test_bound_lies_below_the_oracle_distance_of_aligned_shapes(pkg, oracle):
    """Where the bound is tight: library shapes (every solid kind, Cone and Cylinder included) with identity rotations, their boxes face
    to face along one axis.  The oracle's distance may fall below the raw box distance (inflated supports, rounding) but not below L."""
    abi = pkg.abi
    wl = pkg.workloads.all_primitives(n=1, seed=3, nper=12)
    lib = wl.lib
    n_shapes = len(lib)
    local = pkg.engine.world_aabbs(lib, np.arange(n_shapes, dtype=np.uint32), np.tile(pkg.geometry.make_pose()[None], (n_shapes, 1)))
    rng = np.random.default_rng(23)
    n = 4000
    worst_raw, worst_L = -np.inf, -np.inf
    for offset in (0.0, 30.0, 1000.0, 1e5):
        for sep in (0.01, 3.0, 100.0):
            s1, s2 = rng.integers(0, n_shapes, n), rng.integers(0, n_shapes, n)
            axis = rng.integers(0, 3, n)
            T1 = np.full((n, 3), offset) + rng.uniform(-1, 1, (n, 3))
            T2 = T1 + rng.uniform(-0.05, 0.05, (n, 3))  # (the other two axes: the boxes overlap)
            k = np.arange(n)
            T2[k, axis] = T1[k, axis] + local[s1, 3 + axis] - local[s2, axis] + sep  # box 2's low face `sep` beyond box 1's high face
            tf1, tf2 = pkg.geometry.make_pose(T=T1), pkg.geometry.make_pose(T=T2)
            a = local[s1] + np.tile(T1, 2)
            b = local[s2] + np.tile(T2, 2)
            rec = oracle.distance_batch(wl.shapes, wl.verts, s1, s2, tf1, tf2, abi.default_distance_request(), n_threads=8)
            d = rec["distance"]
            lb, _, M = nearest_model.raw_bound(a, b)
            L = nearest_model.bound(a, b)
            assert np.all(np.isfinite(L)) and np.all(np.abs(lb - sep) <= 1e-9 * max(1.0, offset))
            assert np.all(L <= d), (offset, sep, float((L - d).max()))
            worst_raw, worst_L = max(worst_raw, float((lb - d).max())), max(worst_L, float((L - d).max()))
    print("aligned shapes: the distance falls below the raw box distance by at most %.3g, stays above L by at least %.3g" % (worst_raw, -worst_L))
    assert worst_L <= 0.0


# ---- 5. exactness and shares of the model ---------------------------------------------------------------------------------------------
COUNTED = {(64, 16): 7.07, (256, 16): 6.70, (64, 8): 19.35, (256, 32): 1.88, (2048, 16): 6.48}


@pytest.mark.parametrize("n_conf,n_obj", sorted(COUNTED))
def test_model_is_exact_and_evaluates_a_small_share(pkg, oracle, n_conf, n_obj):
    ps, boxes, rec, full = _scene(pkg, oracle, n_conf, n_obj)
    L = nearest_model.query_bounds(boxes, ps.pairs)
    sel = nearest_model.select(pkg.abi, L, rec, np.inf)
    assert nearest_model.check_against_full(sel["summary"], full) == 0
    s1, s2 = 100.0 * len(sel["ids1"]) / L.size, 100.0 * len(sel["ids2"]) / L.size
    print("scene_planner(%d, %d): %d queries, %.2f %% evaluated in pass 1, %.2f %% in pass 2, %.2f %% in all" % (n_conf, n_obj, L.size, s1, s2, s1 + s2))
    assert round(s1 + s2, 2) == COUNTED[(n_conf, n_obj)]
    if (n_conf, n_obj) == (64, 16):
        assert s1 + s2 < 25.0


@pytest.mark.parametrize("D,beyond", [(0.5, 26), (0.05, 42)])
def test_model_with_an_upper_bound(pkg, oracle, D, beyond):
    ps, boxes, rec, full = _scene(pkg, oracle, 64, 16)
    L = nearest_model.query_bounds(boxes, ps.pairs)
    sel = nearest_model.select(pkg.abi, L, rec, D)
    assert nearest_model.check_against_full(sel["summary"], full, D) == beyond
    unbounded = nearest_model.select(pkg.abi, L, rec, np.inf)
    assert len(sel["ids1"]) + len(sel["ids2"]) < len(unbounded["ids1"]) + len(unbounded["ids2"])
