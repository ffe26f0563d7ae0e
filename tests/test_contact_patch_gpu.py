"""Contact patches on the GPU (hfcl_contact_patch_batch*): the reference's cases through the Python shim, 100k resting pairs
against the fp64 model (tests/patch_model.py), host form = device form, the capacity limit, the reproduced quirks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import patch_model as pm  # noqa: E402

pkg = ge.load_pkg()
abi, engine, geometry, workloads, compat = pkg.abi, pkg.engine, pkg.geometry, pkg.workloads, pkg.compat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def resting():
    b = workloads.resting_contacts(n=100_000, seed=11, mesh_frac=0.05)
    lib = workloads.make_library(pkg, b)
    graphs = b.graphs()
    for sid, (off, ids) in graphs.items():
        lib.set_convex_neighbors(sid, off, ids)
    rec, guess = lib.collide(b.s1, b.s2, b.tf1, b.tf2, abi.default_collision_request(), want_guess=True)
    yield b, lib, rec, guess, graphs
    lib.close()


def _compat_geometry(L, s):
    k, p = int(s["type"]), s["params"]
    if k == abi.GEOM_BOX:
        return compat.Box(2 * p[0], 2 * p[1], 2 * p[2])
    if k == abi.GEOM_SPHERE:
        return compat.Sphere(p[0])
    if k == abi.GEOM_HALFSPACE:
        return compat.Halfspace(p[:3], p[3])
    if k in (abi.GEOM_CAPSULE, abi.GEOM_CONE, abi.GEOM_CYLINDER):
        cls = {abi.GEOM_CAPSULE: compat.Capsule, abi.GEOM_CONE: compat.Cone, abi.GEOM_CYLINDER: compat.Cylinder}[k]
        return cls(p[0], 2 * p[1])
    if k == abi.GEOM_CONVEX:
        o, n = int(s["vertex_offset"]), int(s["num_points"])
        return compat.Convex(L.vertices_array()[o:o + n])
    raise ValueError(k)


@pytest.mark.parametrize("name", pm.REFERENCE_CASE_NAMES)
def test_reference_cases_through_compat(name):
    """The reference's own cases (test/contact_patch.cpp) through compat.computeContactPatch / ComputeContactPatch, checked as
    the reference checks them: expected.isSame(patch, 1e-6)."""
    L, a, b, tf1, tf2, expect = pm.reference_cases(geometry)[name]
    shapes = L.shapes_array()
    o1, o2 = _compat_geometry(L, shapes[a]), _compat_geometry(L, shapes[b])
    T1 = compat.Transform3f(tf1[:9].reshape(3, 3).T, tf1[9:])
    T2 = compat.Transform3f(tf2[:9].reshape(3, 3).T, tf2[9:])
    col_req, col_res = compat.CollisionRequest(), compat.CollisionResult()
    compat.collide(o1, T1, o2, T2, col_req, col_res)
    req = compat.ContactPatchRequest()
    res = compat.ContactPatchResult(req)
    compat.computeContactPatch(o1, T1, o2, T2, col_res, req, res)
    res2 = compat.ContactPatchResult(req)
    compat.ComputeContactPatch(o1, o2)(T1, T2, col_res, req, res2)
    if expect is None:
        assert not col_res.isCollision() and res.numContactPatches() == 0
        return
    assert res.numContactPatches() == 1 and res2.numContactPatches() == 1
    c = col_res.getContact(0)
    rec = np.zeros(1, dtype=abi.RESULT_DTYPE)[0]
    rec["normal"], rec["p1"], rec["p2"], rec["distance"] = c.normal, c.nearest_points[0], c.nearest_points[1], c.penetration_depth
    want = compat.ContactPatch()
    compat.constructContactPatchFrameFromContact(c, want)
    for w in expect(rec):
        want.addPoint(w)
    assert want.isSame(res.getContactPatch(0), 1e-6)
    assert want.isSame(res2.getContactPatch(0), 1e-6)


def test_resting_pairs_equal_model(resting):
    """100k resting pairs over the whole patch matrix, BVH rows included: class, swap bit, point count, frame bits and depth
    equal the model's in every record; points within 1e-9 in the model's order.  A record whose points are the model's in
    another order (a tie of the hull's sort) is counted and listed, at most 5."""
    b, lib, rec, guess, graphs = resting
    out, pts = lib.contact_patch(b.s1, b.s2, b.tf1, b.tf2, rec, guess)
    model = pm.patches(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, rec, guess, graphs=graphs)
    hard, ties = pm.split_mismatches(out, pts, model, 1e-9)
    for i in hard[:10] + ties:
        print("record", i, "shapes", b.shapes["type"][b.s1[i]], b.shapes["type"][b.s2[i]], "class", out["status"][i] & 3,
              model[i][0], "points", out["num_points"][i], len(model[i][4]), "tie" if i in ties else "MISMATCH")
    assert not hard, "%d of %d patches differ from the model: %s" % (len(hard), len(model), hard[:20])
    assert len(ties) <= 5, ties
    cls = out["status"] & 3
    assert all((cls == c).sum() > 1000 for c in range(4))
    # the BVH rows: point patches; GEOM x BVH mirrored, BVH x GEOM and BVH x BVH not
    k1, k2 = b.shapes["type"][b.s1], b.shapes["type"][b.s2]
    hit = rec["num_contacts"] > 0
    swapped = (out["status"] & abi.PATCH_SWAPPED) != 0
    for sel, sw in (((k1 != abi.BV_OBBRSS) & (k2 == abi.BV_OBBRSS), True), ((k1 == abi.BV_OBBRSS) & (k2 != abi.BV_OBBRSS), False),
                    ((k1 == abi.BV_OBBRSS) & (k2 == abi.BV_OBBRSS), False)):
        sel = sel & hit
        assert sel.sum() > 100
        assert (cls[sel] == abi.PATCH_CLASS_POINT).all() and (out["num_points"][sel] == 1).all() and (swapped[sel] == sw).all()


def test_host_equals_device_and_runs_repeat(resting):
    import torch
    b, lib, rec, guess, _ = resting
    req = abi.default_patch_request()
    cap = lib.contact_patch_max_points(req)
    out1, pts1 = lib.contact_patch(b.s1, b.s2, b.tf1, b.tf2, rec, guess, req, cap)
    out2, pts2 = lib.contact_patch(b.s1, b.s2, b.tf1, b.tf2, rec, guess, req, cap)
    assert out1.tobytes() == out2.tobytes() and pts1.tobytes() == pts2.tobytes()
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)  # noqa: E731
    n = len(b)
    d_out = torch.zeros(n * abi.PATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_pts = torch.zeros(n * cap * 2, dtype=torch.float64, device=dev)
    lib.contact_patch_device(t(b.s1), t(b.s2), t(b.tf1), t(b.tf2), t(rec), n, req, cap, d_out, d_pts, d_guesses=t(guess))
    torch.cuda.synchronize()
    out3 = d_out.cpu().numpy().view(abi.PATCH_DTYPE)
    pts3 = d_pts.cpu().numpy().reshape(n, cap, 2)
    assert out3.tobytes() == out1.tobytes()
    # the host form zeroes the rows past num_points; the device form leaves them alone (zeros here: torch.zeros)
    assert pts3.tobytes() == pts1.tobytes()
    for i in range(0, n, 997):
        assert not pts1[i, int(out1["num_points"][i]):].any()
    names = [k for k, _ in lib.last_kernel_breakdown()]
    assert "k_patch_classify" in names and "k_patch_sets<clipped>" in names


def test_capacity_one_below_need_is_refused(resting):
    b, lib, rec, guess, _ = resting
    m = 2000
    need = max(pm.set_bound(int(b.shapes[i]["type"]), int(b.shapes[i]["num_points"]), 12) +
               pm.set_bound(int(b.shapes[j]["type"]), int(b.shapes[j]["num_points"]), 12) for i, j in zip(b.s1[:m], b.s2[:m]))
    out, pts = lib.contact_patch(b.s1[:m], b.s2[:m], b.tf1[:m], b.tf2[:m], rec[:m], guess[:m], points_capacity=need)
    assert out["num_points"].max() <= need
    with pytest.raises(engine.EngineError) as e:
        lib.contact_patch(b.s1[:m], b.s2[:m], b.tf1[:m], b.tf2[:m], rec[:m], guess[:m], points_capacity=need - 1)
    assert e.value.code == abi.ERR_LIMIT
    # C level: the outputs stay untouched
    outb = np.full(m, 0, dtype=abi.PATCH_DTYPE)
    outb["status"] = 0xABCD
    ptsb = np.full((m, need - 1, 2), 5.0)
    req = abi.default_patch_request()
    rc = engine.dll().hfcl_contact_patch_batch(lib._h, abi.ptr(b.s1[:m].copy()), abi.ptr(b.s2[:m].copy()),
                                               abi.ptr(np.ascontiguousarray(b.tf1[:m])), abi.ptr(np.ascontiguousarray(b.tf2[:m])),
                                               abi.ptr(np.ascontiguousarray(rec[:m])), None, C.c_size_t(m), C.byref(req),
                                               C.c_uint32(need - 1), abi.ptr(outb), abi.ptr(ptsb))
    assert rc == abi.ERR_LIMIT and (outb["status"] == 0xABCD).all() and (ptsb == 5.0).all()
    # the device form holds points_capacity against the library's bound
    cap = lib.contact_patch_max_points()
    assert cap == pm.table_bound(b.shapes, 12) == engine.contact_patch_max_points_shapes(b.shapes)


def test_no_patch_cases(resting):
    b, lib, rec, guess, _ = resting
    out, pts = lib.contact_patch(b.s1, b.s2, b.tf1, b.tf2, rec, guess)
    none = rec["num_contacts"] == 0
    assert none.sum() > 1000 and (out["num_points"][none] == 0).all() and (out["status"][none] & 3 == 0).all()
    out0, _ = lib.contact_patch(b.s1, b.s2, b.tf1, b.tf2, rec, guess, abi.default_patch_request(max_num_patch=0))
    assert (out0["num_points"] == 0).all()
    skipped = rec[:100].copy()
    skipped["status"] |= np.uint32(1 << 31)
    outs, _ = lib.contact_patch(b.s1[:100], b.s2[:100], b.tf1[:100], b.tf2[:100], skipped)
    assert (outs["num_points"] == 0).all()


def test_geom_x_bvh_normal_is_flipped():
    b = workloads.mesh_vs_shapes(n=4000, seed=3)
    lib = workloads.make_library(pkg, b)
    try:
        rec = lib.collide(b.s1, b.s2, b.tf1, b.tf2)
        out, pts = lib.contact_patch(b.s1, b.s2, b.tf1, b.tf2, rec)
        k1, k2 = b.shapes["type"][b.s1], b.shapes["type"][b.s2]
        hit = rec["num_contacts"] > 0
        geom_bvh = hit & (k1 != abi.BV_OBBRSS) & (k2 == abi.BV_OBBRSS)
        bvh_any = hit & (k1 == abi.BV_OBBRSS)
        assert geom_bvh.sum() > 50 and bvh_any.sum() > 50
        n = rec["normal"] / np.linalg.norm(rec["normal"], axis=1, keepdims=True)
        assert np.allclose(out["tf"][geom_bvh, 6:9], -n[geom_bvh], atol=1e-12)
        assert (out["status"][geom_bvh] & abi.PATCH_SWAPPED).all()
        assert np.allclose(out["tf"][bvh_any, 6:9], n[bvh_any], atol=1e-12)
        assert (out["num_points"][geom_bvh | bvh_any] == 1).all()
        model = pm.patches(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, rec)
        hard, ties = pm.split_mismatches(out, pts, model, 1e-9)
        assert not hard and not ties
    finally:
        lib.close()


def test_segment_segment_boolean_det_quirk_on_device(monkeypatch):
    """Parallel segments (pm.parallel_capsules): the reference's boolean `det` holds and the patch is the single point
    Contact::pos; a real determinant would give the two ends of the overlap.  The device gives the quirk's answer."""
    L, tf1, tf2 = pm.parallel_capsules(geometry)
    lib = pkg.Library(L, device=0)
    try:
        s = np.zeros(1, np.uint32)
        rec = lib.collide(s, s + 1, tf1, tf2)
        assert rec["num_contacts"][0] == 1 and list(rec["normal"][0]) == [0.0, 0.0, 1.0]
        out, pts = lib.contact_patch(s, s + 1, tf1, tf2, rec)
        assert out["status"][0] & 3 == abi.PATCH_CLASS_CLIPPED
        assert out["num_points"][0] == 1 and tuple(pts[0, 0]) == (0.0, 0.0)
        model = pm.patches(L.shapes_array(), L.vertices_array(), s, s + 1, tf1, tf2, rec)[0]
        assert pm.LAST_BRANCH[0] == "segment_segment_point" and model[4] == [(0.0, 0.0)]
        monkeypatch.setattr(pm, "SEGMENT_DET_QUIRK", False)
        assert len(pm.patches(L.shapes_array(), L.vertices_array(), s, s + 1, tf1, tf2, rec)[0][4]) == 2
    finally:
        lib.close()


def test_cpp_shim_compute_contact_patch(tmp_path):
    """include/hppfcl_amd_compat.hpp: computeContactPatch / ComputeContactPatch on box-on-box and box-on-halfspace (g++ build)."""
    import subprocess
    exe = str(tmp_path / "test_contact_patch_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_patch", "test_contact_patch_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("same") == 2
