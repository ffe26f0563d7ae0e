"""Contact patches (hfcl_contact_patch_batch*) without a GPU: the C ABI's host-only parts, the reference's own cases through the
fp64 model (tests/patch_model.py), and the device header built with g++ (tests/patch_harness) against the model."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import oracle_binding as ob  # noqa: E402
import patch_model as pm  # noqa: E402

pkg = ge.load_pkg()
abi, engine, geometry, workloads = pkg.abi, pkg.engine, pkg.geometry, pkg.workloads

NEW_SYMBOLS = ["hfcl_contact_patch_request_init", "hfcl_patch_supported", "hfcl_contact_patch_max_points",
               "hfcl_contact_patch_max_points_shapes", "hfcl_contact_patch_batch", "hfcl_contact_patch_batch_device"]
PRIMS = [9, 10, 11, 12, 13, 14, 15, 16, 17, 19]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("patch_harness") / "libpatch_harness.so")
    src = os.path.join(ROOT, "tests", "patch_harness", "patch_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-Wno-unknown-pragmas", "-shared", "-o", out, src])
    return C.CDLL(out)


def test_new_symbols_exported():
    lib = engine.dll()
    for s in NEW_SYMBOLS:
        assert s in engine.EXPORTED_SYMBOLS
        getattr(lib, s)
    assert lib.hfcl_abi_version() == 5


def test_request_init_defaults():
    r = engine.contact_patch_request_init()
    assert (r.max_num_patch, r.num_samples_curved_shapes, r.patch_tolerance) == (1, 12, 1e-3)
    assert C.sizeof(abi.PatchRequest) == 16 and abi.PATCH_DTYPE.itemsize == 112


def test_patch_supported_matrix():
    for a in PRIMS + [5]:
        for b in PRIMS + [5]:
            assert engine.patch_supported(a, b), (a, b)
    for bad in (0, 1, 18, 20, 21, 22):
        assert not engine.patch_supported(bad, 9) and not engine.patch_supported(9, bad)


def test_max_points_bound_of_a_known_table():
    L = geometry.ShapeLibrary()
    L.add_box(1, 1, 1)
    L.add_capsule(0.2, 1.0)
    L.add_sphere(0.5)
    assert engine.contact_patch_max_points_shapes(L.shapes_array()) == 8
    L.add_cylinder(0.5, 1.0)
    assert engine.contact_patch_max_points_shapes(L.shapes_array()) == 24
    assert engine.contact_patch_max_points_shapes(L.shapes_array(), abi.default_patch_request(num_samples_curved_shapes=2)) == 8
    L.add_convex(workloads.fibonacci_sphere(40))
    assert engine.contact_patch_max_points_shapes(L.shapes_array()) == 80
    assert pm.table_bound(L.shapes_array(), 12) == 80


def test_entry_points_without_device():
    """No CPU fallback: without a device both entry points say so; with one, a null library is an invalid argument."""
    d = engine.dll()
    req = abi.default_patch_request()
    want = abi.ERR_NO_DEVICE if engine.device_count() == 0 else abi.ERR_INVALID_ARGUMENT
    one = np.zeros(1, dtype=np.uint32)
    rc = d.hfcl_contact_patch_batch(None, abi.ptr(one), abi.ptr(one), None, None, None, None, C.c_size_t(1), C.byref(req),
                                    C.c_uint32(8), None, None)
    assert rc == want
    rc = d.hfcl_contact_patch_batch_device(None, None, None, None, None, None, None, C.c_size_t(1), C.byref(req), C.c_uint32(8),
                                           None, None, None)
    assert rc == want


class _Pairs:
    """A few pairs in the shape of a workload batch (what _harness_patches reads)."""

    def __init__(self, lib, s1, s2, tf1, tf2):
        self.shapes, self.verts = lib.shapes_array(), lib.vertices_array()
        self.s1, self.s2 = np.asarray(s1, np.uint32), np.asarray(s2, np.uint32)
        self.tf1, self.tf2 = np.ascontiguousarray(tf1).reshape(-1, 12), np.ascontiguousarray(tf2).reshape(-1, 12)

    def __len__(self):
        return len(self.s1)


def _reference_case(name):
    lib, a, b, tf1, tf2, expect = pm.reference_cases(geometry)[name]
    pairs = _Pairs(lib, [a], [b], tf1, tf2)
    rec = ob.collide_batch(pairs.shapes, pairs.verts, pairs.s1, pairs.s2, pairs.tf1, pairs.tf2, abi.default_collision_request())
    return pairs, rec, expect


def _check_reference_case(rec, cls, tf, depth, pts, expect):
    if expect is None:
        assert rec["num_contacts"] == 0 and cls == pm.NONE and len(pts) == 0
        return
    assert rec["num_contacts"] == 1
    etf, edepth, epts = pm.expected_patch(rec, expect(rec))
    assert pm.is_same(etf, edepth, epts, tf, depth, pts, 1e-6), (pts, epts)  # expected.isSame(patch, tol), as the reference checks


@pytest.mark.parametrize("name", pm.REFERENCE_CASE_NAMES)
def test_model_reference_cases(name):
    """The reference's own cases (test/contact_patch.cpp) through the model; collision records from the oracle."""
    pairs, rec, expect = _reference_case(name)
    got = pm.patches(pairs.shapes, pairs.verts, pairs.s1, pairs.s2, pairs.tf1, pairs.tf2, rec)[0]
    _check_reference_case(rec[0], got[0], got[2], got[3], got[4], expect)


@pytest.mark.parametrize("name", pm.REFERENCE_CASE_NAMES)
def test_header_reference_cases(harness, name):
    """... and through the device header built with g++."""
    pairs, rec, expect = _reference_case(name)
    cap = pm.table_bound(pairs.shapes, 12)
    out, pts = _harness_patches(harness, pairs, rec, {}, cap)
    n = int(out["num_points"][0])
    _check_reference_case(rec[0], int(out["status"][0]) & 3, list(out["tf"][0]), float(out["penetration_depth"][0]),
                          [tuple(p) for p in pts[0, :n]], expect)


def test_reference_segment_cases_take_the_branches_named():
    """Which branch of computePatch the reference's edge cases reach in the model: the segment_segment cases' support sets are
    triangles (clipping); edge_case_vertex_vertex Case 3 is the one that reaches the two-segment branch, and its boolean
    `det` holds there (one point)."""
    want = {"edge_case_segment_segment/1": "clipping", "edge_case_segment_segment/2": "clipping",
            "edge_case_segment_segment/3": "clipping", "edge_case_vertex_vertex/3": "segment_segment_point",
            "edge_case_segment_face": "clipping"}
    for name, branch in want.items():
        pairs, rec, _ = _reference_case(name)
        pm.patches(pairs.shapes, pairs.verts, pairs.s1, pairs.s2, pairs.tf1, pairs.tf2, rec)
        assert pm.LAST_BRANCH[0] == branch, (name, pm.LAST_BRANCH[0])


def test_segment_segment_boolean_det_quirk(harness, monkeypatch):
    """Parallel segments (pm.parallel_capsules): the reference's boolean `det` gives the single point Contact::pos where a real
    determinant would give the overlap's two ends.  The model and the device header (g++) both give the quirk's answer."""
    L, tf1, tf2 = pm.parallel_capsules(geometry)
    pairs = _Pairs(L, [0], [1], tf1, tf2)
    rec = ob.collide_batch(pairs.shapes, pairs.verts, pairs.s1, pairs.s2, pairs.tf1, pairs.tf2, abi.default_collision_request())
    assert rec["num_contacts"][0] == 1 and list(rec["normal"][0]) == [0.0, 0.0, 1.0]
    quirk = pm.patches(pairs.shapes, pairs.verts, pairs.s1, pairs.s2, pairs.tf1, pairs.tf2, rec)[0][4]
    assert pm.LAST_BRANCH[0] == "segment_segment_point" and quirk == [(0.0, 0.0)]
    monkeypatch.setattr(pm, "SEGMENT_DET_QUIRK", False)
    real = pm.patches(pairs.shapes, pairs.verts, pairs.s1, pairs.s2, pairs.tf1, pairs.tf2, rec)[0][4]
    assert len(real) == 2  # the test tells the two rules apart
    out, pts = _harness_patches(harness, pairs, rec, {}, pm.table_bound(pairs.shapes, 12))
    assert out["num_points"][0] == 1 and out["status"][0] & 3 == pm.CLIPPED and tuple(pts[0, 0]) == (0.0, 0.0)


def test_stable_sort_restatement_equals_libstdcxx(harness):
    """The header's restatement of std::stable_sort orders ties (collinear points at equal distance) as libstdc++ does."""
    rng = np.random.default_rng(3)
    for k in range(2, 40):
        m = 300
        # points on a few rays from the pivot at a few radii: many comparator ties, duplicates included
        ang = rng.integers(0, 4, (m, k)) * 0.4
        rad = rng.integers(1, 4, (m, k)) * 0.5
        pts = np.stack([rad * np.cos(ang), 1.0 + rad * np.sin(ang)], axis=-1)
        piv = np.zeros((m, 2))
        piv[:, 1] = 1.0
        pts, piv = np.ascontiguousarray(pts), np.ascontiguousarray(piv)
        bad = harness.ph_sort_check(abi.ptr(pts), abi.ptr(piv), C.c_size_t(m), C.c_uint32(k))
        assert bad == 0, k


def _harness_patches(harness, b, rec, graphs, cap, ns=12, tol=1e-3, max_num_patch=1):
    n = len(b)
    base = np.full(len(b.shapes), 0xFFFFFFFF, dtype=np.uint32)
    offs, ids = [], []
    total = 0
    for sid, (o, i) in graphs.items():
        base[sid] = sum(len(x) for x in offs)
        offs.append(np.asarray(o, np.uint32) + total)
        ids.append(np.asarray(i, np.uint32))
        total += len(i)
    off = np.ascontiguousarray(np.concatenate(offs) if offs else np.zeros(1, np.uint32), dtype=np.uint32)
    idv = np.ascontiguousarray(np.concatenate(ids) if ids else np.zeros(1, np.uint32), dtype=np.uint32)
    out = np.zeros(n, dtype=abi.PATCH_DTYPE)
    pts = np.zeros((n, cap, 2))
    shapes = np.ascontiguousarray(b.shapes)
    verts = np.ascontiguousarray(b.verts, dtype=np.float64)
    harness.ph_patches(abi.ptr(shapes), C.c_uint32(len(shapes)), abi.ptr(verts), abi.ptr(base), abi.ptr(off), abi.ptr(idv),
                       abi.ptr(b.s1), abi.ptr(b.s2), abi.ptr(np.ascontiguousarray(b.tf1)), abi.ptr(np.ascontiguousarray(b.tf2)),
                       abi.ptr(rec), None, C.c_size_t(n), C.c_uint32(max_num_patch), C.c_uint32(ns), C.c_double(tol),
                       C.c_uint32(cap), abi.ptr(out), abi.ptr(pts))
    return out, pts


def test_header_on_host_equals_model_on_resting_pairs(harness):
    b = workloads.resting_contacts(n=20_000, seed=5)
    rec = ob.collide_batch(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, abi.default_collision_request())
    graphs = b.graphs()
    cap = pm.table_bound(b.shapes, 12)
    out, pts = _harness_patches(harness, b, rec, graphs, cap)
    model = pm.patches(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, rec, graphs=graphs)
    hard, ties = pm.split_mismatches(out, pts, model, 1e-12)
    assert not hard and not ties, "%d / %d of %d records differ, first %s" % (len(hard), len(ties), len(model), (hard + ties)[:10])
    cls = out["status"] & 3
    # the workload reaches every class and polygons of many sizes
    assert all((cls == c).sum() > 100 for c in range(4))
    assert len(np.unique(out["num_points"][cls == 3])) >= 6
