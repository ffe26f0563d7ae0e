"""Culling a scene's pair list per configuration (include/hppfcl_amd_cull.h) without a GPU: the exports and null checks, and the cull
header (hpp-fcl_amd/csrc/hfcl_cull.hpp) built with g++ (tests/cull_harness) -- its boxes against engine.world_aabbs bit for bit, its
mark / scan / emit and its fold over a list against the numpy models of tests/cull_model.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cull_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cull_harness") / "libcull_harness.so")
    src = os.path.join(ROOT, "tests", "cull_harness", "cull_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-o", out, src])
    d = C.CDLL(out)
    d.ch_cull.restype = C.c_uint64
    return d


@pytest.fixture(scope="module")
def planner(pkg):
    """scene_planner(64, 16, seed 1) and its host boxes (engine.world_aabbs, configuration by configuration): shared, not modified."""
    ps = pkg.workloads.scene_planner(64, 16, seed=1)
    tf = ps.obj_tf
    boxes = np.stack([pkg.engine.world_aabbs(ps.lib, ps.obj_shape, tf[c]) for c in range(len(tf))])
    return ps, tf, boxes


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def _cull_symbols():
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_cull.h")).read()
    return sorted(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]+)\s*\(", hdr)))


def test_exports_and_bindings(pkg):
    pkg.engine.build_native()
    lib = pkg.engine.dll()
    syms = _cull_symbols()
    assert len(syms) == 16 and set(syms) == set(pkg.engine.CULL_SYMBOLS)
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert '#include "hppfcl_amd_cull.h"' in main  # (one header for a caller)
    assert lib.hfcl_abi_version() == 5
    assert "scene_cull_chunk" in pkg.engine.option_keys()
    for m in ("world_aabbs", "cull", "collide_culled", "distance_culled", "cull_device", "collide_listed_device", "distance_listed_device",
              "collide_listed_device_f32", "distance_listed_device_f32", "world_aabbs_device"):
        assert hasattr(pkg.engine.Scene, m), m
    # the header compiles as C
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd.h")])


def test_null_arguments_do_not_crash(pkg):
    d, abi = pkg.engine.dll(), pkg.abi
    creq, dreq = abi.default_collision_request(), abi.default_distance_request()
    n1, z, infl = C.c_size_t(1), C.c_size_t(0), C.c_double(0.0)
    n = C.c_size_t(7)
    tf = np.zeros((2, 12))
    calls = [
        (d.hfcl_scene_world_aabbs, (None, abi.ptr(tf), n1, abi.ptr(tf))),
        (d.hfcl_scene_world_aabbs_f32, (None, None, n1, None)),
        (d.hfcl_scene_world_aabbs_device, (None, None, n1, None, None)),
        (d.hfcl_scene_world_aabbs_device_f32, (None, None, n1, None, None)),
        (d.hfcl_scene_cull, (None, abi.ptr(tf), n1, infl, None, z, None, C.byref(n))),
        (d.hfcl_scene_cull_f32, (None, None, n1, infl, None, z, None, C.byref(n))),
        (d.hfcl_scene_cull_device, (None, None, n1, infl, None, z, None, None, None)),
        (d.hfcl_scene_cull_device_f32, (None, None, n1, infl, None, z, None, None, None)),
        (d.hfcl_scene_collide_listed_device, (None, None, n1, None, z, None, C.byref(creq), None, None, None, None, None)),
        (d.hfcl_scene_distance_listed_device, (None, None, n1, None, z, None, C.byref(dreq), None, None, None, None, None)),
        (d.hfcl_scene_collide_listed_device_f32, (None, None, n1, None, z, None, C.byref(creq), None, None, None)),
        (d.hfcl_scene_distance_listed_device_f32, (None, None, n1, None, z, None, C.byref(dreq), None, None, None)),
        (d.hfcl_scene_collide_culled, (None, abi.ptr(tf), n1, infl, C.byref(creq), None, z, None, None, None, None, None, C.byref(n))),
        (d.hfcl_scene_distance_culled, (None, abi.ptr(tf), n1, infl, C.byref(dreq), None, z, None, None, None, None, None, C.byref(n))),
        (d.hfcl_scene_collide_culled_f32, (None, None, n1, infl, C.byref(creq), None, z, None, None, None, C.byref(n))),
        (d.hfcl_scene_distance_culled_f32, (None, None, n1, infl, C.byref(dreq), None, z, None, None, None, C.byref(n))),
    ]
    assert sorted(fn.__name__ for fn, _ in calls) == sorted(pkg.engine.CULL_SYMBOLS)
    for fn, args in calls:
        assert fn(*args) == abi.ERR_INVALID_ARGUMENT, fn.__name__
        assert "null scene" in pkg.engine.last_error(), fn.__name__
    assert n.value == 7  # (a refused call writes nothing)


# ---- boxes ------------------------------------------------------------------------------------------------------------------------
def _every_kind_library(pkg):
    """The cfg5 mix (Box, Sphere, Capsule, Ellipsoid, Convex) plus Cone, Cylinder, TriangleP, Plane, Halfspace (aligned with an axis and
    not) and swept-sphere radii."""
    L = pkg.ShapeLibrary()
    rng = np.random.default_rng(4)
    L.add_box(0.6, 0.8, 1.0)
    L.add_sphere(0.5)
    L.add_capsule(0.3, 1.2)
    L.add_ellipsoid(0.4, 0.6, 0.8)
    L.add_convex(rng.normal(size=(32, 3)) * 0.5)
    L.add_cone(0.4, 1.1)
    L.add_cylinder(0.35, 0.9)
    L.add_triangle([0.1, 0, 0], [1, 0.2, 0], [0, 1, 0.3])
    L.add_plane([0, 0, 1], 0.25)
    L.add_plane([1, 2, -1], 0.5)
    L.add_halfspace([0, -1, 0], 0.75)
    L.add_halfspace([0.3, 0.1, 1], -0.2)
    L.add_box(0.2, 0.3, 0.4, swept_sphere_radius=0.05)
    L.add_convex(rng.normal(size=(9, 3)), swept_sphere_radius=0.125)
    L.add_capsule(0.2, 0.7, swept_sphere_radius=0.3)
    return L


def _poses_with_identity_edges(pkg, rng, n):
    """n random poses; then rotations that are exactly the identity, inside Eigen's isIdentity tolerance (1e-12), and just outside it."""
    tf = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, n), T=rng.uniform(-2, 2, (n, 3)))
    edge = []
    for off, diag in ((0.0, 1.0), (5e-13, 1.0), (2e-12, 1.0), (0.0, 1.0 + 5e-13), (0.0, 1.0 - 2e-12), (-9.9e-13, 1.0), (1.0000001e-12, 1.0)):
        R = np.eye(3)
        R[0, 1] = off
        R[2, 2] = diag
        edge.append(pkg.geometry.make_pose(R=R, T=rng.uniform(-2, 2, 3)))
    return np.concatenate([tf, np.stack(edge)]), len(edge)


def test_header_boxes_equal_the_host_broadphase(pkg, harness):
    abi = pkg.abi
    L = _every_kind_library(pkg)
    shapes, verts = np.ascontiguousarray(L.shapes_array()), np.ascontiguousarray(L.vertices_array())
    rng = np.random.default_rng(8)
    n_obj = 3 * len(L)
    obj_shape = (np.arange(n_obj) % len(L)).astype(np.uint32)
    tf, n_edge = _poses_with_identity_edges(pkg, rng, 4 * n_obj - 7)
    assert len(tf) == 4 * n_obj  # four configurations; the edge rotations fall on the last objects of the last one
    exp = np.concatenate([pkg.engine.world_aabbs(L, obj_shape, tf[c * n_obj:(c + 1) * n_obj]) for c in range(4)])
    got = np.full((len(tf), 6), np.nan)
    harness.ch_world_boxes(abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), abi.ptr(obj_shape), abi.ptr(tf), C.c_uint64(n_obj),
                           C.c_uint64(len(tf)), abi.ptr(got))
    assert got.tobytes() == exp.tobytes()
    ident = [harness.ch_is_identity(abi.ptr(np.ascontiguousarray(t[:9]))) for t in tf[-n_edge:]]
    assert ident == [1, 1, 0, 1, 0, 1, 0]  # exactly, inside and just outside the tolerance
    # the identity branch is the translation alone: L + T, no interval sums
    k = len(tf) - n_edge
    loc = pkg.engine.world_aabbs(L, obj_shape[k % n_obj:k % n_obj + 1], pkg.geometry.make_pose()[None])
    assert np.array_equal(got[k], loc[0] + np.tile(tf[k, 9:], 2))
    # unbounded boxes: a Plane not aligned with an axis is +-DBL_MAX in its frame, infinite after a rotation
    big = np.finfo(np.float64).max
    planes = np.flatnonzero(obj_shape == 9)
    assert np.all(np.isinf(got[planes[0]])) and not np.any(np.isnan(got))
    assert np.array_equal(pkg.engine.world_aabbs(L, [9], pkg.geometry.make_pose()[None])[0], [-big] * 3 + [big] * 3)


def test_header_boxes_fp32_form(pkg, harness):
    """7-float poses: widened to double, the rotation rebuilt in pose_from_quat's order of operations -- which geometry.quat_to_matrix
    restates in numpy, operation for operation -- then the fp64 arithmetic."""
    abi = pkg.abi
    L = _every_kind_library(pkg)
    shapes, verts = np.ascontiguousarray(L.shapes_array()), np.ascontiguousarray(L.vertices_array())
    rng = np.random.default_rng(9)
    n_obj = 2 * len(L)
    obj_shape = (np.arange(n_obj) % len(L)).astype(np.uint32)
    pose = pkg.geometry.pose_f32_from_quat(pkg.workloads.uniform_quaternions(rng, 3 * n_obj), rng.uniform(-2, 2, (3 * n_obj, 3)))
    pose[5, :4] = (1, 0, 0, 0)  # an exact identity
    wide = pkg.geometry.make_pose(quat=pose[:, :4].astype(np.float64), T=pose[:, 4:].astype(np.float64))
    exp = np.concatenate([pkg.engine.world_aabbs(L, obj_shape, wide[c * n_obj:(c + 1) * n_obj]) for c in range(3)])
    got = np.full((len(pose), 6), np.nan)
    harness.ch_world_boxes_f32(abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), abi.ptr(obj_shape), abi.ptr(pose), C.c_uint64(n_obj),
                               C.c_uint64(len(pose)), abi.ptr(got))
    assert got.tobytes() == exp.tobytes()


def test_mesh_local_box_is_the_box_of_the_vertices(pkg, harness):
    v, _ = pkg.bvh_builder.bumpy_sphere(7, 5, r=1.0, amp=0.2, freq=3, phase=0.4)
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64) + [0.3, -0.2, 0.1])
    out = np.zeros(6)
    harness.ch_mesh_box(pkg.abi.ptr(v), C.c_size_t(len(v)), pkg.abi.ptr(out))
    assert np.array_equal(out, np.concatenate([v.min(axis=0), v.max(axis=0)]))


# ---- the cull -----------------------------------------------------------------------------------------------------------------------
def _header_cull(harness, pkg, boxes, pairs, inflate, chunk, capacity=None):
    n_conf, n_obj = boxes.shape[:2]
    total = n_conf * len(pairs)
    cap = total if capacity is None else capacity
    ids = np.full(max(cap, 1), 0xABABABABABABABAB, dtype=np.uint64)
    cb = np.full(n_conf + 1, 0xABABABABABABABAB, dtype=np.uint64)
    b, p = np.ascontiguousarray(boxes), np.ascontiguousarray(pairs, dtype=np.uint32)
    n = harness.ch_cull(pkg.abi.ptr(b), pkg.abi.ptr(p), C.c_uint32(len(p)), C.c_uint64(n_obj), C.c_uint64(n_conf), C.c_double(inflate),
                        C.c_uint64(chunk), pkg.abi.ptr(ids), C.c_uint64(cap), pkg.abi.ptr(cb))
    return ids, cb, int(n)


@pytest.mark.parametrize("inflate", [0.0, 0.25])
def test_header_cull_equals_the_model(pkg, harness, planner, inflate):
    ps, _, boxes = planner
    exp_ids, exp_cb = cull_model.cull_queries(boxes, ps.pairs, inflate)
    total = 64 * len(ps.pairs)
    assert total == 6720 and len(ps.pairs) == 105
    # ... and the model is the definition, query by query
    plain = [q for q in range(total) if not any(
        boxes[q // 105, ps.pairs[q % 105, 0], k] - inflate > boxes[q // 105, ps.pairs[q % 105, 1], 3 + k] + inflate or
        boxes[q // 105, ps.pairs[q % 105, 0], 3 + k] + inflate < boxes[q // 105, ps.pairs[q % 105, 1], k] - inflate for k in range(3))]
    assert plain == list(exp_ids) and [int(np.searchsorted(exp_ids, c * 105)) for c in range(65)] == list(exp_cb)
    for chunk in (total, 1000, 256, 64, 105, 63, 1):
        ids, cb, n = _header_cull(harness, pkg, boxes, ps.pairs, inflate, chunk)
        assert n == len(exp_ids), chunk
        assert ids[:n].tobytes() == exp_ids.tobytes() and cb.tobytes() == exp_cb.tobytes(), chunk
    # a capacity one short: the count is true, the ids below the capacity are right, nothing is written past it
    ids, cb, n = _header_cull(harness, pkg, boxes, ps.pairs, inflate, 1000, capacity=len(exp_ids) - 1)
    assert n == len(exp_ids) and ids[:n - 1].tobytes() == exp_ids[:-1].tobytes() and cb.tobytes() == exp_cb.tobytes()


def test_header_cull_everything_nothing_and_nan(pkg, harness, planner):
    ps, _, boxes = planner
    ids, cb, n = _header_cull(harness, pkg, boxes, ps.pairs, 1e3, 1000)
    assert n == 6720 and np.array_equal(ids, np.arange(6720)) and np.array_equal(cb, np.arange(65) * 105)
    far = boxes.copy()
    far[..., :] += (np.arange(16) * 100.0)[None, :, None]  # the bodies spread out: no two boxes touch
    ids, cb, n = _header_cull(harness, pkg, far, ps.pairs, 0.0, 1000)
    assert n == 0 and not cb.any()
    nan = far.copy()
    nan[3, 5, 1] = np.nan  # a NaN makes its comparison false: where only that axis separates, the pair is kept
    ids, cb, n = _header_cull(harness, pkg, nan, ps.pairs, 0.0, 4096)
    e_ids, e_cb = cull_model.cull_queries(nan, ps.pairs, 0.0)
    assert ids[:n].tobytes() == e_ids.tobytes() and cb.tobytes() == e_cb.tobytes()
    touching = boxes[:1, :2].copy()
    touching[0, 1] = touching[0, 0]
    touching[0, 1, 0] = touching[0, 0, 3]  # closed intervals: a shared face counts
    touching[0, 1, 3] = touching[0, 0, 3] + 1.0
    assert _header_cull(harness, pkg, touching, np.array([[0, 1]]), 0.0, 1)[2] == 1


def test_counted_shares_of_the_planner_scene(pkg):
    """What the cull is for: the share of listed pairs whose boxes overlap, counted with the host boxes (workloads.scene_planner, seed 1)."""
    counted = {(64, 16): (3.4, 7.6, 10), (256, 16): (3.6, 8.1, 20), (64, 8): (6.6, 15.4, 22), (256, 32): (1.5, 3.6, 0)}
    for (n_conf, n_obj), (share0, share25, empty) in counted.items():
        ps = pkg.workloads.scene_planner(n_conf, n_obj, seed=1)
        tf = ps.obj_tf
        boxes = np.stack([pkg.engine.world_aabbs(ps.lib, ps.obj_shape, tf[c]) for c in range(n_conf)])
        total = n_conf * len(ps.pairs)
        ids0, cb0 = cull_model.cull_queries(boxes, ps.pairs, 0.0)
        ids25, _ = cull_model.cull_queries(boxes, ps.pairs, 0.25)
        s0, s25, e = 100.0 * len(ids0) / total, 100.0 * len(ids25) / total, int((np.diff(cb0.astype(np.int64)) == 0).sum())
        print("scene_planner(%d, %d): %d pairs / conf, %.1f %% overlap, %.1f %% with boxes grown by 0.25, %d configurations without a pair"
              % (n_conf, n_obj, len(ps.pairs), s0, s25, e))
        assert (round(s0, 1), round(s25, 1), e) == (share0, share25, empty)
        assert s0 < 10.0
        if (n_conf, n_obj) == (64, 16):
            assert e >= 1


def test_oracle_contacts_are_in_the_list(pkg, oracle, planner):
    """Every pair the oracle finds in contact (default request) has touching boxes: n_contacts and first_contact of a summary over the
    inflate-0 list equal the unculled ones (tests/test_scene_cull_gpu.py relies on it for this seed)."""
    ps, _, boxes = planner
    b = ps.expand()
    ref = oracle.collide_batch(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, pkg.abi.default_collision_request())
    contact = np.flatnonzero(pkg.abi.status_contact(ref["status"]) == 1)
    ids, _ = cull_model.cull_queries(boxes, ps.pairs, 0.0)
    print("scene_planner(64, 16): %d contacts among %d overlapping of %d listed pairs" % (len(contact), len(ids), len(ref)))
    assert len(contact) > 0 and np.all(np.isin(contact, ids.astype(np.int64)))


# ---- the fold over a list -----------------------------------------------------------------------------------------------------------
def _synthetic(pkg, rng, n, f32):
    rec = np.zeros(n, dtype=pkg.abi.RESULT_F32_DTYPE if f32 else pkg.abi.RESULT_DTYPE)
    t = rec["distance"].dtype.type
    d = rng.integers(-2, 3, n).astype(t) * t(0.37)  # few distinct values: ties are the rule
    d[rng.random(n) < 0.1] = np.nan
    d[rng.random(n) < 0.02] = np.inf
    rec["distance"] = d
    st = rng.integers(0, 1 << 23, n).astype(np.uint32) & ~np.uint32(1 << 7)
    st |= (rng.random(n) < 0.3).astype(np.uint32) << 7
    st |= (rng.random(n) < 0.15).astype(np.uint32) << 31
    rec["status"] = st
    return rec


@pytest.mark.parametrize("f32", [False, True])
def test_header_fold_over_a_list_equals_numpy(pkg, harness, f32):
    """Lists with empty configurations, with configurations of one record and of several pieces (more than 256 survivors), cut into
    chunks that end inside configurations: the fold of the gathered records, field by field."""
    abi = pkg.abi
    rng = np.random.default_rng(12)
    # (the last three: survivors in the first and last configuration only -- a chunk then spans more configurations than it has entries)
    for n_pairs, n_conf, p_keep in ((105, 40, 0.05), (7, 9, 0.5), (1, 30, 0.4), (700, 5, 0.9), (300, 6, 0.02), (64, 3, 1.0), (1, 3, -1), (100, 12, -1),
                                    (600, 12, -1)):
        keep = rng.random((n_conf, n_pairs)) < abs(p_keep)
        keep[n_conf // 2] = False
        if p_keep < 0:
            keep[1:-1] = False
            keep[0, :min(2, n_pairs)] = keep[-1, -1] = True
            keep[0, 2:] = keep[-1, :-1] = False
            assert keep.sum() < n_conf or n_conf == 3
        ids = np.flatnonzero(keep.reshape(-1)).astype(np.uint64)
        cb = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint64)
        rec = _synthetic(pkg, rng, len(ids), f32)
        for margin, collide in ((0.0, 0), (0.125, 1)):
            exp = cull_model.fold_listed(abi, rec, ids, n_conf, n_pairs, margin if collide else None)
            assert np.isposinf(exp["min_distance"][n_conf // 2]) and exp["min_pair"][n_conf // 2] == NONE and exp["n_skipped"][n_conf // 2] == 0
            for chunk in (max(len(ids), 1), 1, 37, 64, 255, 256, 257, 1000):
                got = np.full(n_conf, 0xAB, dtype=np.uint8).repeat(24).view(abi.SCENE_SUMMARY_DTYPE)  # (every summary must be written)
                fn = harness.ch_fold_listed_f32 if f32 else harness.ch_fold_listed
                fn(abi.ptr(rec), abi.ptr(ids), abi.ptr(cb), C.c_uint64(len(ids)), C.c_uint64(n_conf), C.c_uint32(n_pairs), C.c_double(margin),
                   C.c_int(collide), C.c_uint64(chunk), abi.ptr(got))
                assert got.tobytes() == exp.tobytes(), (n_pairs, chunk, margin)
