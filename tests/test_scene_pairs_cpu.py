"""The self-collision pairs of a scene per configuration (include/hppfcl_amd_pairs.h) without a GPU: the exports and the refusal without
a device; the numpy model (tests/pairs_model.py) against the host broadphase entry for entry; the header (hpp-fcl_amd/csrc/hfcl_pairs.hpp)
built with g++ (tests/pairs_harness) -- its count / scan / emit in both forms and however the call is cut, its span searches and its
ranked fold -- against the model byte for byte; and the C++ shim's new methods."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cull_model
import pairs_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
FILL32, FILL64 = 0xABABABAB, 0xABABABABABABABAB
SIZES = [(1, 3), (2, 3), (5, 37), (63, 3), (64, 3), (65, 3), (130, 3), (257, 3), (600, 3)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pairs_harness") / "libpairs_harness.so")
    src = os.path.join(ROOT, "tests", "pairs_harness", "pairs_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-o", out, src])
    d = C.CDLL(out)
    d.ph_self_pairs.restype = C.c_uint64
    d.ph_shares.restype = C.c_uint64
    return d


_SCENES = {}


def _scene(pkg, n_objects, n_conf):
    """Built once, shared, not modified."""
    key = (n_objects, n_conf)
    if key not in _SCENES:
        if "lib" not in _SCENES:
            _SCENES["lib"] = pairs_model.mixed_library(pkg)
        _SCENES[key] = pairs_model.PairScene(pkg, _SCENES["lib"], n_objects, n_conf)
    return _SCENES[key]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings(pkg):
    pkg.engine.build_native()
    lib = pkg.engine.dll()
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_pairs.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]+)\s*\(", hdr)))
    assert len(syms) == 12 and syms == sorted(pkg.engine.PAIRS_SYMBOLS)
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    assert not set(syms) & set(pkg.engine.EXPORTED_SYMBOLS + pkg.engine.CULL_SYMBOLS + pkg.engine.NEAREST_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert main.count('#include "hppfcl_amd_pairs.h"') == 1 and main.rstrip().endswith('#include "hppfcl_amd_pairs.h"\n#endif /* HPPFCL_AMD_H */')
    assert lib.hfcl_abi_version() == 5
    assert "scene_pairs_small_max" in pkg.engine.option_keys()
    for m in ("self_pairs", "collide_self", "distance_self", "self_pairs_device", "collide_pairs_device", "distance_pairs_device",
              "collide_pairs_device_f32", "distance_pairs_device_f32"):
        assert hasattr(pkg.engine.Scene, m), m
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd.h")])


def test_entry_points_without_a_device(pkg):
    """No CPU fallback: without a device every entry point says so; with one, a null scene is an invalid argument.  Nothing is written."""
    d, abi = pkg.engine.dll(), pkg.abi
    creq, dreq = abi.default_collision_request(), abi.default_distance_request()
    n1, z, infl = C.c_size_t(1), C.c_size_t(0), C.c_double(0.0)
    n = C.c_size_t(7)
    tf = np.zeros((2, 12))
    calls = [
        (d.hfcl_scene_self_pairs, (None, abi.ptr(tf), n1, infl, None, z, None, C.byref(n))),
        (d.hfcl_scene_self_pairs_f32, (None, None, n1, infl, None, z, None, C.byref(n))),
        (d.hfcl_scene_self_pairs_device, (None, None, n1, infl, None, z, None, None, None)),
        (d.hfcl_scene_self_pairs_device_f32, (None, None, n1, infl, None, z, None, None, None)),
        (d.hfcl_scene_collide_pairs_device, (None, None, n1, None, z, None, C.byref(creq), None, None, None, None, None)),
        (d.hfcl_scene_distance_pairs_device, (None, None, n1, None, z, None, C.byref(dreq), None, None, None, None, None)),
        (d.hfcl_scene_collide_pairs_device_f32, (None, None, n1, None, z, None, C.byref(creq), None, None, None)),
        (d.hfcl_scene_distance_pairs_device_f32, (None, None, n1, None, z, None, C.byref(dreq), None, None, None)),
        (d.hfcl_scene_collide_self, (None, abi.ptr(tf), n1, infl, C.byref(creq), None, z, None, None, None, None, None, C.byref(n))),
        (d.hfcl_scene_distance_self, (None, abi.ptr(tf), n1, infl, C.byref(dreq), None, z, None, None, None, None, None, C.byref(n))),
        (d.hfcl_scene_collide_self_f32, (None, None, n1, infl, C.byref(creq), None, z, None, None, None, C.byref(n))),
        (d.hfcl_scene_distance_self_f32, (None, None, n1, infl, C.byref(dreq), None, z, None, None, None, C.byref(n))),
    ]
    assert sorted(fn.__name__ for fn, _ in calls) == sorted(pkg.engine.PAIRS_SYMBOLS)
    no_device = pkg.engine.device_count() == 0
    for fn, args in calls:
        assert fn(*args) == (abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT), fn.__name__
        assert ("no CPU fallback" if no_device else "null scene") in pkg.engine.last_error(), fn.__name__
    assert n.value == 7


def test_shim_methods_compile(tmp_path):
    src = tmp_path / "shim.cpp"
    src.write_text('#include "hppfcl_amd_compat.hpp"\n'
                   "void use(hpp::fcl::amd::Scene& s, const hpp::fcl::Transform3f* t, std::vector<uint32_t>& p, std::vector<uint64_t>& b, "
                   "std::vector<hfcl_scene_summary>& m) { s.selfPairs(t, 1, 0.0, p, b); "
                   "s.collideSelf(t, 1, 0.0, hpp::fcl::CollisionRequest(), nullptr, p, b, &m); s.distanceSelf(t, 1, 0.0, hpp::fcl::DistanceRequest(), nullptr, p, b, &m); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


# ---- the model is the host broadphase -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_objects,n_conf", SIZES)
def test_model_equals_the_host_broadphase(pkg, n_objects, n_conf):
    sc = _scene(pkg, n_objects, n_conf)
    counts = sc.check_shares()
    pairs, cb = sc.expected()
    assert pairs.dtype == np.uint32 and cb.dtype == np.uint64 and cb[0] == 0 and cb[-1] == len(pairs) == counts.sum()
    for c in range(n_conf):
        host = pkg.engine.broadphase_self_pairs(sc.boxes[c])
        mine = pairs[int(cb[c]):int(cb[c + 1])]
        assert mine.tobytes() == host.astype(np.uint32).tobytes(), c
    if len(pairs):
        assert np.all(pairs[:, 0] < pairs[:, 1]) and pairs.max() < n_objects
    # grown boxes list more
    p25, cb25 = sc.expected(inflate=0.25)
    assert np.all(np.diff(cb25.astype(np.int64)) >= counts)


# ---- the header -------------------------------------------------------------------------------------------------------------------------
def _header_pairs(harness, pkg, boxes, inflate, chunk_rows=0, small_max=64, capacity=None, count_only=False):
    n_conf, n = boxes.shape[:2]
    cap = max(n_conf * n * (n - 1) // 2, 1) if capacity is None else capacity
    pairs = np.full((max(cap, 1) + 3, 2), FILL32, dtype=np.uint32)  # (three guard entries)
    cb = np.full(n_conf + 1, FILL64, dtype=np.uint64)
    n_chunks = C.c_uint64(0)
    b = np.ascontiguousarray(boxes)
    got = harness.ph_self_pairs(pkg.abi.ptr(b), C.c_uint32(n), C.c_uint64(n_conf), C.c_double(inflate), C.c_uint64(chunk_rows), C.c_uint32(small_max),
                                None if count_only else pkg.abi.ptr(pairs), C.c_uint64(cap), pkg.abi.ptr(cb), C.byref(n_chunks))
    return pairs, cb, int(got), int(n_chunks.value)


@pytest.mark.parametrize("n_objects,n_conf", SIZES[2:])
def test_header_list_equals_the_model(pkg, harness, n_objects, n_conf):
    sc = _scene(pkg, n_objects, n_conf)
    for f32, inflate in ((False, 0.0), (False, 0.25), (True, 0.0)):
        exp, exp_cb = sc.expected(f32, inflate)
        boxes = sc.boxes32 if f32 else sc.boxes
        # one chunk; chunks that start in the middle of a configuration (tiled form: 16 rows a block); a block a chunk; the other form
        for chunk_rows, small_max in ((0, 64), (n_objects + 16, 64), (40, 64), (1, 64), (0, 0), (40, 0)):
            pairs, cb, n, n_chunks = _header_pairs(harness, pkg, boxes, inflate, chunk_rows, small_max)
            what = (f32, inflate, chunk_rows, small_max)
            assert n == len(exp), what
            assert pairs[:n].tobytes() == exp.tobytes() and cb.tobytes() == exp_cb.tobytes(), what
            assert np.all(pairs[n:] == FILL32), what
            if chunk_rows == 40 and (n_objects > 64 or small_max == 0) and n_objects > 48:
                assert n_chunks > n_conf  # (some chunk starts inside a configuration)


def test_header_small_scenes_and_edges(pkg, harness):
    for n_objects, n_conf in SIZES[:2]:
        sc = _scene(pkg, n_objects, n_conf)
        exp, exp_cb = sc.expected()
        for small_max in (64, 0):
            pairs, cb, n, _ = _header_pairs(harness, pkg, sc.boxes, 0.0, 0, small_max)
            assert n == len(exp) and pairs[:n].tobytes() == exp.tobytes() and cb.tobytes() == exp_cb.tobytes()
    sc = _scene(pkg, 130, 3)
    exp, exp_cb = sc.expected()
    # count only
    pairs, cb, n, _ = _header_pairs(harness, pkg, sc.boxes, 0.0, 40, count_only=True)
    assert n == len(exp) and cb.tobytes() == exp_cb.tobytes() and np.all(pairs == FILL32)
    # a capacity below the count: the count is true, the entries below the capacity are right, nothing is written past it
    cap = len(exp) // 2
    pairs, cb, n, _ = _header_pairs(harness, pkg, sc.boxes, 0.0, 40, capacity=cap)
    assert n == len(exp) and pairs[:cap].tobytes() == exp[:cap].tobytes() and np.all(pairs[cap:] == FILL32) and cb.tobytes() == exp_cb.tobytes()
    # a NaN keeps the pair where only its axis separates; closed intervals: a shared face counts
    nan = sc.boxes.copy()
    nan[0, 7, 1] = np.nan
    e, e_cb = pairs_model.self_pairs(nan, 0.0)
    assert exp_cb[1] == 0 and e_cb[1] >= 1  # (configuration 0 had no pair)
    pairs, cb, n, _ = _header_pairs(harness, pkg, nan, 0.0)
    assert n == len(e) and pairs[:n].tobytes() == e.tobytes() and cb.tobytes() == e_cb.tobytes()
    touching = np.array([[[0, 0, 0, 1, 1, 1.0], [1, 0, 0, 2, 1, 1.0], [2.5, 0, 0, 3, 1, 1]]])
    pairs, cb, n, _ = _header_pairs(harness, pkg, touching, 0.0)
    assert n == 1 and tuple(pairs[0]) == (0, 1)
    pairs, cb, n, _ = _header_pairs(harness, pkg, touching, 0.25)
    assert n == 2 and [tuple(p) for p in pairs[:2]] == [(0, 1), (1, 2)]


def test_header_span_search(pkg, harness):
    """The configuration of a list entry: spans with empty configurations in front, in between and at the end."""
    rng = np.random.default_rng(5)
    for counts in ([3, 0, 0, 5, 1, 0], [0, 0, 4], [1], [0, 7, 0, 0, 0, 0, 0, 0, 0, 2, 0], list(rng.integers(0, 4, 200))):
        cb = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        n = int(cb[-1])
        exp = pairs_model.conf_of(cb).astype(np.uint64)
        for stride in (1, 11, 64):
            a, b = np.full(n, FILL64, dtype=np.uint64), np.full(n, FILL64, dtype=np.uint64)
            harness.ph_conf_of(pkg.abi.ptr(cb), C.c_uint64(len(counts)), C.c_uint64(n), C.c_uint64(stride), pkg.abi.ptr(a), pkg.abi.ptr(b))
            assert a.tobytes() == exp.tobytes() and b.tobytes() == exp.tobytes(), (counts[:8], stride)
    # pieces of 256 entries a configuration can have: no more entries than the list, or than pairs
    assert [harness.ph_shares(C.c_uint64(a), C.c_uint64(b)) for a, b in ((0, 16), (120, 16), (121, 16), (10 ** 6, 16), (257, 600), (10 ** 6, 10 ** 5),
                                                                        (256, 1), (2 ** 40, 2 ** 22))] == [1, 1, 1, 1, 2, 3907, 1, 2 ** 32]


def _synthetic(pkg, rng, n, f32):
    rec = np.zeros(n, dtype=pkg.abi.RESULT_F32_DTYPE if f32 else pkg.abi.RESULT_DTYPE)
    t = rec["distance"].dtype.type
    d = rng.integers(-2, 3, n).astype(t) * t(0.37)  # few distinct values: ties are the rule
    d[rng.random(n) < 0.1] = np.nan
    rec["distance"] = d
    st = rng.integers(0, 1 << 23, n).astype(np.uint32) & ~np.uint32(1 << 7)
    st |= (rng.random(n) < 0.3).astype(np.uint32) << 7
    st |= (rng.random(n) < 0.15).astype(np.uint32) << 31
    rec["status"] = st
    return rec


@pytest.mark.parametrize("f32", [False, True])
def test_header_ranked_fold_equals_numpy(pkg, harness, f32):
    abi = pkg.abi
    rng = np.random.default_rng(13)
    for counts in ([5, 0, 700, 1, 0, 300], [0, 0, 3], [1000], [0, 2, 0, 0, 0, 0, 0, 0, 1]):
        cb = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        n, n_conf = int(cb[-1]), len(counts)
        rec = _synthetic(pkg, rng, n, f32)
        shares = (max(counts) + 255) // 256
        for margin, collide in ((0.0, 0), (0.125, 1)):
            exp = pairs_model.fold_ranked(abi, rec, cb, margin if collide else None)
            empty = [c for c in range(n_conf) if counts[c] == 0]
            assert np.all(np.isposinf(exp["min_distance"][empty])) and np.all(exp["min_pair"][empty] == NONE)
            for chunk in (n, 1, 37, 256, 257):
                got = np.full(n_conf, 0xAB, dtype=np.uint8).repeat(24).view(abi.SCENE_SUMMARY_DTYPE)
                fn = harness.ph_fold_ranked_f32 if f32 else harness.ph_fold_ranked
                fn(abi.ptr(rec), abi.ptr(cb), C.c_uint64(n), C.c_uint64(n_conf), C.c_uint32(shares), C.c_double(margin), C.c_int(collide),
                   C.c_uint64(chunk), abi.ptr(got))
                assert got.tobytes() == exp.tobytes(), (counts, chunk, margin)
