"""A height-field terrain under a scene's moving objects (include/hppfcl_amd_terrain.h) without a GPU: the exports and the refusals
without a device; the host build of hpp-fcl_amd/csrc/hfcl_terrain.hpp (tests/terrain_harness) against the numpy model
(tests/terrain_model.py) -- the expansion of whole calls and of a chunk that starts and ends mid-configuration, and the fold on synthetic
(bound, status) tables: ties, NaN bounds, every entry skipped, no contact / every entry a contact, more entries than a wave has lanes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import terrain_model as tm

ROOT = tm.ROOT
CONTACT, SKIPPED = tm.CONTACT_BIT, tm.SKIPPED_BIT


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return tm.build_harness(tmp_path_factory.mktemp("terrain_harness"))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings(pkg):
    pkg.engine.build_native()
    lib, e = pkg.engine.dll(), pkg.engine
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_terrain.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]*terrain[a-z0-9_]*)\s*\(", hdr)))
    assert syms == sorted(e.TERRAIN_SYMBOLS) and len(syms) == 5
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    older = (e.EXPORTED_SYMBOLS + e.CULL_SYMBOLS + e.NEAREST_SYMBOLS + e.PAIRS_SYMBOLS + e.GROUPS_SYMBOLS + e.NEAREST_SELF_SYMBOLS + e.ENV_SYMBOLS +
             e.NEAREST_ENV_SYMBOLS + e.HFIELD_SYMBOLS)
    assert not set(syms) & set(older)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert len(re.findall(r'#include "[./]*hppfcl_amd_terrain\.h"', main)) == 1
    assert main.index("hppfcl_amd_hfield.h") < main.index("hppfcl_amd_terrain.h") < main.index("hppfcl_amd_pairs.h")  # (the pairs header stays last)
    includes = re.findall(r'#include "[./]*(hppfcl_amd_[a-z_]+\.h)"', main)
    assert includes[includes.index("hppfcl_amd_hfield.h") + 1] == "hppfcl_amd_terrain.h"  # directly after the height-field header
    assert lib.hfcl_abi_version() == 5
    for m in ("set_terrain", "clear_terrain", "n_terrain_objects", "collide_terrain", "collide_terrain_device"):
        assert hasattr(e.Scene, m), m
    assert hasattr(pkg.compat, "collide_terrain") and hasattr(pkg.workloads, "scene_robot_terrain")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd.h")])
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd_terrain.h")])


def test_entry_points_without_a_device(pkg):
    """No CPU fallback: without a device the setter and the compute entry points say so; with one, a null scene is an invalid argument.
    Nothing is written."""
    d, abi = pkg.engine.dll(), pkg.abi
    req = abi.default_collision_request()
    tf = np.zeros((2, 12))
    ids = np.zeros(2, dtype=np.uint32)
    bounds = np.full(4, 7.5)
    n = C.c_size_t(7)
    one = C.c_size_t(1)
    calls = [
        (d.hfcl_scene_set_terrain, (None, C.c_uint32(0), abi.ptr(tf), abi.ptr(ids), one)),
        (d.hfcl_scene_clear_terrain, (None,)),
        (d.hfcl_scene_collide_terrain, (None, abi.ptr(tf), one, C.byref(req), None, abi.ptr(bounds), None, None, C.c_size_t(0), C.byref(n))),
        (d.hfcl_scene_collide_terrain_device, (None, None, one, C.byref(req), None, None, None, None, C.c_size_t(0), C.byref(n), None)),
    ]
    assert sorted([fn.__name__ for fn, _ in calls] + ["hfcl_scene_n_terrain_objects"]) == sorted(pkg.engine.TERRAIN_SYMBOLS)
    no_device = pkg.engine.device_count() == 0
    for fn, args in calls:
        assert fn(*args) == (abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT), fn.__name__
        assert ("no CPU fallback" if no_device else "null scene") in pkg.engine.last_error(), fn.__name__
    assert d.hfcl_scene_n_terrain_objects(None) == 0
    assert np.all(bounds == 7.5) and n.value == 7


def test_shim_methods_compile(tmp_path):
    src = tmp_path / "shim.cpp"
    src.write_text('#include "hppfcl_amd_compat.hpp"\n'
                   "size_t use(hpp::fcl::amd::Scene& s, const hpp::fcl::HeightField<hpp::fcl::AABB>& field, const hpp::fcl::Transform3f* moving,\n"
                   "           const hpp::fcl::CollisionRequest& creq) {\n"
                   "  s.setTerrain(&field, hpp::fcl::Transform3f(), {0, 2});\n"
                   "  s.setTerrain(&field, hpp::fcl::Transform3f());\n"
                   "  std::vector<hfcl_scene_summary> summaries;\n"
                   "  std::vector<hpp::fcl::CollisionResult> cres;\n"
                   "  s.collideTerrain(moving, 3, creq, &cres, &summaries);\n"
                   "  s.collideTerrain(moving, 3, creq, nullptr, &summaries);\n"
                   "  s.clearTerrain();\n"
                   "  return summaries.size() + s.numTerrainObjects();\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src)])


# ---- the expansion ------------------------------------------------------------------------------------------------------------------
def _expand(h, table, tf_terrain, objects, object_shape, hfield, q0, m):
    n_rows = table.shape[1]
    objects = np.ascontiguousarray(objects, dtype=np.uint32)
    guard = 3
    o_hf = np.full(m + guard, 0xAAAAAAAA, dtype=np.uint32)
    o_sh = np.full(m + guard, 0xAAAAAAAA, dtype=np.uint32)
    o_tfh = np.full((m + guard, 12), -9.0)
    o_tfs = np.full((m + guard, 12), -9.0)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h.th_expand(P(table), P(tf_terrain), P(objects) if len(objects) else None, P(object_shape), C.c_uint64(n_rows), C.c_uint32(len(objects)),
                C.c_uint32(hfield), C.c_uint64(q0), C.c_uint32(m), P(o_hf), P(o_sh), P(o_tfh), P(o_tfs))
    assert (o_hf[m:] == 0xAAAAAAAA).all() and (o_sh[m:] == 0xAAAAAAAA).all() and (o_tfh[m:] == -9.0).all() and (o_tfs[m:] == -9.0).all()
    return o_hf[:m], o_sh[:m], o_tfh[:m], o_tfs[:m]


@pytest.mark.parametrize("n_conf", [1, 3])
@pytest.mark.parametrize("n_t", [0, 1, 7, 65])
def test_expansion_equals_model(harness, n_t, n_conf):
    rng = np.random.default_rng(100 * n_t + n_conf)
    n_rows = max(n_t, 1) + 5
    table = rng.normal(size=(n_conf, n_rows, 12))
    tf_terrain = rng.normal(size=12)
    object_shape = rng.integers(0, 40, n_rows + 3).astype(np.uint32)  # (the scene may hold more objects than the table has rows)
    objects = np.sort(rng.choice(n_rows, n_t, replace=False)).astype(np.uint32)
    total = n_conf * n_t
    spans = [(0, total)]
    if total >= 3 and n_conf > 1:  # a chunk that starts and ends mid-configuration
        spans.append((n_t // 2 + (1 if n_t > 1 else 0), total - (n_t // 2 + 1) - (n_t // 2 + (1 if n_t > 1 else 0))))
        if n_t > 1:
            assert spans[-1][0] % n_t != 0 and (spans[-1][0] + spans[-1][1]) % n_t != 0
    if total > 2:
        spans += [(1, 1), (total - 1, 1)]
    for q0, m in spans:
        got = _expand(harness, table, tf_terrain, objects, object_shape, 4, q0, m)
        want = tm.expand(table, tf_terrain, objects, object_shape, 4, q0, m)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (n_t, n_conf, q0, m)


# ---- the fold -----------------------------------------------------------------------------------------------------------------------
def _fold(h, bounds, status, objects, n_conf):
    objects = np.ascontiguousarray(objects, dtype=np.uint32)
    bounds = np.ascontiguousarray(bounds, dtype=np.float64)
    status = np.ascontiguousarray(status, dtype=np.uint32)
    out = np.zeros(n_conf + 1, dtype=tm.SUMMARY_DTYPE)
    out[n_conf]["n_skipped"] = 77
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h.th_fold(P(bounds), P(status), P(objects), C.c_uint64(n_conf), C.c_uint32(len(objects)), P(out))
    assert out[n_conf]["n_skipped"] == 77 and out[n_conf]["min_distance"] == 0.0
    return out[:n_conf]


def _same(got, want):
    return got.tobytes() == want.tobytes()  # (every field, min_distance bit for bit)


@pytest.mark.parametrize("n_t", [1, 63, 64, 65, 130])
def test_fold_equals_model(harness, n_t):
    rng = np.random.default_rng(n_t)
    objects = np.sort(rng.choice(3 * n_t + 2, n_t, replace=False)).astype(np.uint32)
    confs = []
    # random bounds, a third of the entries a contact, a few skipped, a few NaN
    b = rng.normal(size=n_t)
    s = np.where(rng.uniform(size=n_t) < 0.33, CONTACT, 0).astype(np.uint32)
    sk = rng.uniform(size=n_t) < 0.1
    s[sk] = SKIPPED
    b[sk] = np.finfo(np.float64).max
    b[rng.uniform(size=n_t) < 0.1] = np.nan
    confs.append((b, s))
    # a tie between two objects (the lower index wins), placed in different lanes and, from 65 entries on, in different strides
    b = rng.uniform(1.0, 2.0, n_t)
    lo, hi = (0, n_t - 1) if n_t > 1 else (0, 0)
    b[[hi, lo]] = 0.25
    confs.append((b, np.zeros(n_t, dtype=np.uint32)))
    b = rng.uniform(1.0, 2.0, n_t)
    b[n_t // 2:] = b[n_t // 2]  # a long run of equal bounds
    confs.append((b, np.full(n_t, CONTACT, dtype=np.uint32)))  # ... and every entry a contact
    # NaN bounds: one (with a contact flag: it still counts), then all of them
    b = rng.uniform(-1.0, 1.0, n_t)
    b[n_t // 3] = np.nan
    s = np.zeros(n_t, dtype=np.uint32)
    s[n_t // 3] = CONTACT
    confs.append((b, s))
    confs.append((np.full(n_t, np.nan), np.zeros(n_t, dtype=np.uint32)))
    # every entry skipped
    confs.append((np.full(n_t, np.finfo(np.float64).max), np.full(n_t, SKIPPED, dtype=np.uint32)))
    # no contact at all; the minimum in the last entry; bounds of +inf and -0.0 / +0.0 (equal: the lower object wins)
    b = rng.uniform(0.5, 1.5, n_t)
    b[-1] = 0.125
    confs.append((b, np.zeros(n_t, dtype=np.uint32)))
    confs.append((np.full(n_t, np.inf), np.zeros(n_t, dtype=np.uint32)))
    b = np.full(n_t, 3.0)
    b[-1] = -0.0
    b[0] = 0.0
    confs.append((b, np.zeros(n_t, dtype=np.uint32)))
    bounds = np.concatenate([c[0] for c in confs])
    status = np.concatenate([c[1] for c in confs])
    got = _fold(harness, bounds, status, objects, len(confs))
    want = tm.fold(bounds, status, objects, len(confs))
    assert _same(got, want), (got, want)
    # what the model itself must say about the named cases
    assert want[1]["min_distance"] == 0.25 and want[1]["min_pair"] == objects[lo] and want[1]["n_contacts"] == 0 and want[1]["first_contact"] == tm.NONE
    assert want[2]["n_contacts"] == n_t and want[2]["first_contact"] == objects[0]
    assert want[3]["n_contacts"] == 1 and want[3]["first_contact"] == objects[n_t // 3] and (n_t == 1 or want[3]["min_pair"] != objects[n_t // 3])
    assert want[4]["min_distance"] == np.inf and want[4]["min_pair"] == tm.NONE
    assert want[5]["min_distance"] == np.inf and want[5]["min_pair"] == tm.NONE and want[5]["n_skipped"] == n_t and want[5]["n_contacts"] == 0
    assert want[6]["min_pair"] == objects[-1] and want[7]["min_pair"] == objects[0] and want[7]["min_distance"] == np.inf
    assert want[8]["min_pair"] == objects[0]


def test_fold_of_no_entries(harness):
    got = _fold(harness, np.zeros(0), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), 3)
    want = tm.fold(np.zeros(0), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), 3)
    assert _same(got, want) and (want["min_distance"] == np.inf).all() and (want["min_pair"] == tm.NONE).all() and (want["n_skipped"] == 0).all()
