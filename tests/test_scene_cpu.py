"""Scene queries (hfcl_scene_*) without a GPU: the C ABI's exports and null checks, the summary's layout, and the scene header
(hpp-fcl_amd/csrc/hfcl_scene.hpp) built with g++ (tests/scene_harness) -- its fold and its index arithmetic against numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("scene_harness") / "libscene_harness.so")
    src = os.path.join(ROOT, "tests", "scene_harness", "scene_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-o", out, src])
    d = C.CDLL(out)
    d.sh_summary_size.restype = C.c_size_t
    d.sh_fold_share.restype = C.c_uint32
    return d


def _scene_symbols():
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    return sorted(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]+)\s*\(", hdr)))


def test_exports_and_bindings(pkg):
    pkg.engine.build_native()
    lib = pkg.engine.dll()
    syms = _scene_symbols()
    assert {"hfcl_scene_create", "hfcl_scene_set_pairs", "hfcl_scene_destroy", "hfcl_scene_num_objects", "hfcl_scene_num_pairs",
            "hfcl_scene_collide", "hfcl_scene_distance", "hfcl_scene_collide_device", "hfcl_scene_distance_device",
            "hfcl_scene_collide_f32", "hfcl_scene_distance_f32", "hfcl_scene_collide_device_f32",
            "hfcl_scene_distance_device_f32"} == set(syms)
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
        assert s in pkg.engine.EXPORTED_SYMBOLS, "engine.py does not bind " + s
    assert lib.hfcl_abi_version() == 5
    assert "scene_chunk" in pkg.engine.option_keys()
    assert hasattr(pkg.engine.Library, "scene") and hasattr(pkg.engine, "Scene")


def test_summary_layout(pkg, harness):
    dt = pkg.abi.SCENE_SUMMARY_DTYPE
    assert harness.sh_summary_size() == 24 == dt.itemsize
    assert [dt.fields[k][1] for k in ("min_distance", "min_pair", "first_contact", "n_contacts", "n_skipped")] == [0, 8, 12, 16, 20]
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    body = hdr[hdr.index("typedef struct hfcl_scene_summary {"):hdr.index("} hfcl_scene_summary;")]
    assert re.findall(r"^\s*(double|uint32_t)\s+(\w+);", body, re.M) == [
        ("double", "min_distance"), ("uint32_t", "min_pair"), ("uint32_t", "first_contact"), ("uint32_t", "n_contacts"),
        ("uint32_t", "n_skipped")]


def test_null_arguments_do_not_crash(pkg):
    d = pkg.engine.dll()
    abi = pkg.abi
    ids = np.zeros(2, dtype=np.uint32)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    d.hfcl_scene_create.restype = C.c_void_p
    assert not d.hfcl_scene_create(None, abi.ptr(ids), C.c_size_t(2), abi.ptr(pairs), C.c_size_t(1))
    assert "null library" in pkg.engine.last_error()
    d.hfcl_scene_destroy(None)  # a no-op
    assert d.hfcl_scene_num_objects(None) == 0 and d.hfcl_scene_num_pairs(None) == 0
    assert d.hfcl_scene_set_pairs(None, abi.ptr(pairs), C.c_size_t(1)) == abi.ERR_INVALID_ARGUMENT
    tf = np.zeros((2, 12))
    pose = np.zeros((2, 7), dtype=np.float32)
    out = np.zeros(1, dtype=abi.RESULT_DTYPE)
    out32 = np.zeros(1, dtype=abi.RESULT_F32_DTYPE)
    summ = np.zeros(1, dtype=abi.SCENE_SUMMARY_DTYPE)
    creq, dreq = abi.default_collision_request(), abi.default_distance_request()
    n1 = C.c_size_t(1)
    calls = [
        (d.hfcl_scene_collide, (None, abi.ptr(tf), n1, C.byref(creq), abi.ptr(out), abi.ptr(summ), None, None)),
        (d.hfcl_scene_distance, (None, abi.ptr(tf), n1, C.byref(dreq), abi.ptr(out), abi.ptr(summ), None, None)),
        (d.hfcl_scene_collide_device, (None, None, n1, C.byref(creq), None, None, None, None, None)),
        (d.hfcl_scene_distance_device, (None, None, n1, C.byref(dreq), None, None, None, None, None)),
        (d.hfcl_scene_collide_f32, (None, abi.ptr(pose), n1, C.byref(creq), abi.ptr(out32), abi.ptr(summ))),
        (d.hfcl_scene_distance_f32, (None, abi.ptr(pose), n1, C.byref(dreq), abi.ptr(out32), abi.ptr(summ))),
        (d.hfcl_scene_collide_device_f32, (None, None, n1, C.byref(creq), None, None, None)),
        (d.hfcl_scene_distance_device_f32, (None, None, n1, C.byref(dreq), None, None, None)),
    ]
    for fn, args in calls:
        assert fn(*args) == abi.ERR_INVALID_ARGUMENT, fn.__name__
        assert "null scene" in pkg.engine.last_error()


# ---- the fold ---------------------------------------------------------------------------------------------------------------
def _plain_fold(value, status, n_pairs):
    """The summary's definition, record by record in plain Python (the yardstick of abi.fold_records and of the header)."""
    n_conf = len(value) // n_pairs
    out = []
    for c in range(n_conf):
        best, bp, first, nc, ns = np.inf, NONE, NONE, 0, 0
        seen = False
        for p in range(n_pairs):
            v, s = value[c * n_pairs + p], int(status[c * n_pairs + p])
            if s >> 31:
                ns += 1
                continue
            if not np.isnan(v) and (not seen or v < best):
                best, bp, seen = v, p, True
            if (s >> 7) & 1:
                nc += 1
                if first == NONE:
                    first = p
        out.append((best, bp, first, nc, ns))
    return out


def _synthetic(pkg, rng, n, f32=False, p_nan=0.1, p_skip=0.15, p_contact=0.3, levels=5):
    rec = np.zeros(n, dtype=pkg.abi.RESULT_F32_DTYPE if f32 else pkg.abi.RESULT_DTYPE)
    # few distinct values: ties at different indices are the rule
    d = rng.integers(-2, levels - 2, n).astype(rec["distance"].dtype) * rec["distance"].dtype.type(0.37)
    d[rng.random(n) < p_nan] = np.nan
    d[rng.random(n) < 0.02] = np.inf
    rec["distance"] = d
    st = rng.integers(0, 1 << 23, n).astype(np.uint32) & ~np.uint32(1 << 7)
    st |= (rng.random(n) < p_contact).astype(np.uint32) << 7
    st |= (rng.random(n) < p_skip).astype(np.uint32) << 31
    rec["status"] = st
    return rec


def _header_fold(harness, pkg, rec, n_pairs, margin, collide, chunk):
    n_conf = len(rec) // n_pairs
    out = np.full(n_conf, 0xAB, dtype=np.uint8).repeat(24).view(pkg.abi.SCENE_SUMMARY_DTYPE)  # (every summary must be written)
    fn = harness.sh_fold_f32 if rec.dtype == pkg.abi.RESULT_F32_DTYPE else harness.sh_fold
    fn(pkg.abi.ptr(rec), C.c_uint64(len(rec)), C.c_uint32(n_pairs), C.c_double(margin), C.c_int(collide), C.c_uint64(chunk), pkg.abi.ptr(out))
    return out


def _assert_same(a, b, what):
    assert a.tobytes() == b.tobytes(), "%s\n%r\n%r" % (what, a[:4], b[:4])


@pytest.mark.parametrize("f32", [False, True])
def test_numpy_fold_is_the_definition(pkg, f32):
    rng = np.random.default_rng(7)
    for n_pairs, n_conf, margin in ((1, 5, None), (7, 9, 0.25), (130, 3, -0.5), (64, 4, 0.0)):
        rec = _synthetic(pkg, rng, n_pairs * n_conf, f32)
        t = rec["distance"].dtype.type
        with np.errstate(invalid="ignore"):
            v = (rec["distance"] if margin is None else rec["distance"] - t(margin)).astype(np.float64)
        got = pkg.abi.fold_records(rec, n_pairs, margin)
        for c, exp in enumerate(_plain_fold(v, rec["status"], n_pairs)):
            assert tuple(got[c].tolist()) == exp, (n_pairs, c)


@pytest.mark.parametrize("f32", [False, True])
def test_header_fold_equals_numpy(pkg, harness, f32):
    """Ties, NaNs, infinities, skipped records, one chunk and chunks that straddle configurations, pair lists of one piece and of
    several (the two-launch form): equal field for field."""
    rng = np.random.default_rng(11)
    share = harness.sh_fold_share()
    assert share == 256
    for n_pairs, n_conf in ((1, 70), (3, 41), (64, 9), (105, 33), (share, 3), (share + 1, 3), (3 * share + 17, 2)):
        rec = _synthetic(pkg, rng, n_pairs * n_conf, f32)
        for margin, collide in ((0.0, 0), (0.125, 1), (-1.0 / 3.0, 1)):
            exp = pkg.abi.fold_records(rec, n_pairs, margin if collide else None)
            for chunk in (len(rec), 1, 37, 64, n_pairs, n_pairs + 1, 2 * n_pairs + 5, share - 1, 1000, 3000):
                got = _header_fold(harness, pkg, rec, n_pairs, margin, collide, chunk)
                _assert_same(got, exp, "n_pairs %d chunk %d margin %r" % (n_pairs, chunk, margin))


def test_header_fold_all_skipped_all_nan_and_forced_ties(pkg, harness):
    abi = pkg.abi
    n_pairs, n_conf = 50, 3
    rec = np.zeros(n_pairs * n_conf, dtype=abi.RESULT_DTYPE)
    rec["status"] = 1 << 31
    for chunk in (7, 150):
        got = _header_fold(harness, pkg, rec, n_pairs, 0.0, 1, chunk)
        assert np.all(np.isposinf(got["min_distance"])) and np.all(got["min_pair"] == NONE) and np.all(got["first_contact"] == NONE)
        assert np.all(got["n_contacts"] == 0) and np.all(got["n_skipped"] == n_pairs)
    rec["status"] = 0
    rec["distance"] = np.nan
    got = _header_fold(harness, pkg, rec, n_pairs, 0.0, 0, 7)
    assert np.all(np.isposinf(got["min_distance"])) and np.all(got["min_pair"] == NONE) and np.all(got["n_skipped"] == 0)
    # every pair twice: the first of the two wins; a NaN in front of the minimum does not poison it
    rec["distance"] = np.tile(np.repeat(np.arange(25, 0, -1.0), 2), n_conf)
    rec["distance"][0] = np.nan
    rec["status"][48::50] = 1 << 7
    rec["status"][49::50] = 1 << 7
    for chunk in (1, 49, 150):
        got = _header_fold(harness, pkg, rec, n_pairs, 0.5, 1, chunk)
        assert list(got["min_pair"]) == [48] * 3 and list(got["min_distance"]) == [0.5] * 3
        assert list(got["first_contact"]) == [48] * 3 and list(got["n_contacts"]) == [2] * 3
        _assert_same(got, abi.fold_records(rec, n_pairs, 0.5), chunk)


def test_header_fold_split_at_every_boundary(pkg, harness):
    """One configuration cut in two at every possible place, and three configurations cut by every chunk size: the same summaries."""
    rng = np.random.default_rng(3)
    rec = _synthetic(pkg, rng, 90)
    exp1 = pkg.abi.fold_records(rec, 90, 0.2)
    exp3 = pkg.abi.fold_records(rec, 30, 0.2)
    for cut in range(1, 90):
        # chunks [0, cut) and [cut, 90): a chunk size of `cut` makes further chunks too, which must not matter either
        _assert_same(_header_fold(harness, pkg, rec, 90, 0.2, 1, cut), exp1, cut)
        _assert_same(_header_fold(harness, pkg, rec, 30, 0.2, 1, cut), exp3, cut)


# ---- the expansion ------------------------------------------------------------------------------------------------------------
def test_expansion_index_arithmetic(pkg, harness):
    rng = np.random.default_rng(5)
    n_objects, n_pairs, n_conf = 11, 23, 6
    pairs = rng.integers(0, n_objects, (n_pairs, 2)).astype(np.uint32)
    pairs[3] = (4, 4)  # i == j is allowed
    obj_shape = rng.integers(0, 1000, n_objects).astype(np.uint32)
    table = rng.normal(size=(n_conf, n_objects, 12))
    i, j = pairs[:, 0], pairs[:, 1]
    exp_s1, exp_s2 = np.tile(obj_shape[i], n_conf), np.tile(obj_shape[j], n_conf)
    exp_tf1, exp_tf2 = table[:, i].reshape(-1, 12), table[:, j].reshape(-1, 12)
    total = n_conf * n_pairs
    for chunk in (total, 1, 10, n_pairs, n_pairs + 7, 64):  # (10, 30, 64 straddle configurations)
        s1, s2 = np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.uint32)
        tf1, tf2 = np.zeros((total, 12)), np.zeros((total, 12))
        for q0 in range(0, total, chunk):
            m = min(chunk, total - q0)
            a, b, t1, t2 = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32), np.zeros((m, 12)), np.zeros((m, 12))
            harness.sh_expand(pkg.abi.ptr(pairs), pkg.abi.ptr(obj_shape), pkg.abi.ptr(table), C.c_uint64(n_objects), C.c_uint32(n_pairs),
                              C.c_uint64(q0), C.c_uint32(m), pkg.abi.ptr(a), pkg.abi.ptr(b), pkg.abi.ptr(t1), pkg.abi.ptr(t2))
            s1[q0:q0 + m], s2[q0:q0 + m], tf1[q0:q0 + m], tf2[q0:q0 + m] = a, b, t1, t2
        assert np.array_equal(s1, exp_s1) and np.array_equal(s2, exp_s2), chunk
        assert tf1.tobytes() == exp_tf1.tobytes() and tf2.tobytes() == exp_tf2.tobytes(), chunk


def test_chunk_relative_query_equals_the_division(harness):
    """scene_query_from (one 32-bit division per lane, from the chunk's own (c0, p0)) against q / n_pairs, also where p0 + row
    passes 2^32 and where q0 is beyond 2^32."""
    rng = np.random.default_rng(13)
    top = (1 << 32) - 16
    cases = [(0, 0, 1), (5, 7, 3), (top - 1, top - 1, top), (top - 1, 0xFFFFFFEF, top), (1 << 40, 12345, 105), ((1 << 40) + 104, 0xFFFFFFEF, 105)]
    for _ in range(2000):
        n_pairs = int(rng.integers(1, top + 1)) if rng.random() < 0.5 else int(rng.integers(1, 3000))
        cases.append((int(rng.integers(0, 1 << 45)), int(rng.integers(0, 0xFFFFFFF0)), n_pairs))
    for q0, row, n_pairs in cases:
        assert harness.sh_query_from_agrees(C.c_uint64(q0), C.c_uint32(row), C.c_uint32(n_pairs)) == 1, (q0, row, n_pairs)


def test_scene_planner_expands_like_the_arithmetic(pkg):
    ps = pkg.workloads.scene_planner(n_conf=5, n_objects=6, seed=2)
    assert len(ps.pairs) == 6 * 5 // 2 - 5 and np.all(ps.pairs[:, 1] - ps.pairs[:, 0] >= 2)
    b = ps.expand()
    tf = ps.obj_tf
    assert b.tf1.tobytes() == tf[:, ps.pairs[:, 0]].reshape(-1, 12).tobytes()
    assert b.tf2.tobytes() == tf[:, ps.pairs[:, 1]].reshape(-1, 12).tobytes()
    assert np.array_equal(b.s1, np.tile(ps.obj_shape[ps.pairs[:, 0]], 5))


def test_scene_planner_minority_collides(pkg, oracle):
    """scene_planner aims at 10-50 % colliding configurations (the oracle decides)."""
    n_conf = 256
    ps = pkg.workloads.scene_planner(n_conf=n_conf, n_objects=16, seed=1)
    b = ps.expand()
    ref = oracle.collide_batch(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, pkg.abi.default_collision_request())
    summ = pkg.abi.fold_records(ref, len(ps.pairs), 0.0)
    share = float((summ["n_contacts"] > 0).mean())
    print("scene_planner(256, 16): %.1f %% of the configurations collide, %.2f %% of the queries" % (
        100 * share, 100 * float(pkg.abi.status_contact(ref["status"]).mean())))
    assert 0.10 <= share <= 0.50
