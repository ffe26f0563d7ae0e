"""HeightField<AABB> x convex solid collide() (include/hppfcl_amd_hfield.h) on the GPU.  The yardstick is the host build of the device
header (tests/hfield_harness, held against the fp64 model in tests/test_hfield_cpu.py): records, bounds and contacts of the device call
equal the harness's byte for byte, the host call equals the device call for two values of the chunk option, and the reference's own
cases (tests/golden/hfield_kat.json) pass through the C ABI, compat.collide and the C++ shim with the reference's tolerances.

Shapes: fields of 2 x 2 (the root is a leaf: no box test at all), 3 x 2 and 2 x 3 (one split along each axis), 5 x 7 (uneven halves) and
34 x 34 samples (1 089 cells: more items in one query than a workgroup has lanes); batches of 1, 63, 64, 65 and 257 queries, each a
cycle of: a solid far off the field (no item, the bound from the root's box), over one cell, on an edge, on a corner (the side faces),
one whose box covers the whole field (many items, between queries with none), and one below min_height -- all seven kinds, both operand
orders, identity and rotated field poses, the three margins, num_max_contacts in {1, 2, 5000}."""
import os
import subprocess

import numpy as np
import pytest

import hfield_cases as hc

pytestmark = pytest.mark.gpu
ROOT = hc.ROOT
SIZES = (1, 63, 64, 65, 257)
MARGINS = (0.0, 0.05, -0.02)
MAX_CONTACTS = (1, 2, 5000)
GRIDS = ((2, 2), (3, 2), (2, 3), (5, 7), (34, 34))  # (nx, ny)


@pytest.fixture(scope="module")
def world(pkg, torch_cuda, tmp_path_factory):
    rng = np.random.default_rng(7)
    fields = [("f%dx%d" % g, 3.0, 4.0, rng.uniform(0.2, 1.5, (g[1], g[0])), -0.3) for g in GRIDS]
    L, solids = hc.seven_solids(pkg, rng)
    cover = L.add_box(9.0, 9.0, 0.5)  # its box covers a whole field under any pose used here
    lib = pkg.Library(L)
    for _, x_dim, y_dim, h, mh in fields:
        lib.add_hfield(x_dim, y_dim, h, mh)
    assert lib.hfield_count() == len(fields)
    yield dict(lib=lib, L=L, solids=solids, cover=cover, fields=fields, tables=hc.HarnessFields(pkg, fields),
               harness=hc.build_harness(tmp_path_factory.mktemp("hfield_harness")))
    lib.close()


def _queries(pkg, w, f, n, rotated):
    """n queries on field f: the cycle of the module docstring"""
    geo = pkg.geometry
    _, x_dim, y_dim, h, mh = w["fields"][f]
    ny, nx = h.shape
    rng = np.random.default_rng(1000 * f + n)
    tfh1 = geo.make_pose(quat=hc.random_rotations(rng, 1)[0], T=np.array([0.4, -0.7, 0.3])) if rotated else geo.make_pose()
    shape = np.zeros(n, dtype=np.uint32)
    local = np.zeros((n, 3))
    for i in range(n):
        kind, solid = i % 6, w["solids"][(i // 6 + i) % 7]
        cx, cy = int(rng.integers(0, nx - 1)), int(rng.integers(0, ny - 1))
        x0, y0 = -x_dim / 2 + (cx + 0.5) * x_dim / (nx - 1), y_dim / 2 - (cy + 0.5) * y_dim / (ny - 1)
        top = h[cy:cy + 2, cx:cx + 2].mean()
        if kind == 0:  # far off the field
            p = (40.0 + i % 5, -35.0, 20.0)
        elif kind == 1:  # over one cell, about half of them touching
            p = (x0, y0, top + rng.uniform(0.0, 0.5))
        elif kind == 2:  # on an edge
            p = (x_dim / 2 + rng.uniform(-0.05, 0.25), y0, 0.3 * top)
        elif kind == 3:  # on a corner
            p = (-x_dim / 2 - rng.uniform(-0.05, 0.2), y_dim / 2 + rng.uniform(-0.05, 0.2), 0.2)
        elif kind == 4:  # its box covers the whole field; the slab dips into the highest samples
            solid, p = w["cover"], (0.0, 0.0, h.max() + 0.25 - rng.uniform(0.0, 0.3))
        else:  # below min_height
            p = (x0, y0, mh - 0.6)
        shape[i], local[i] = solid, p
    tfh = np.repeat(tfh1.reshape(1, 12), n, axis=0)
    rot = hc.random_rotations(rng, n)
    rot[shape == w["cover"]] = (1.0, 0.0, 0.0, 0.0)  # the slab lies flat in the field's frame ...
    tfs = geo.compose(tfh, geo.make_pose(quat=rot, T=local))  # ... and every solid is placed in it
    swapped = ((np.arange(n) // 3) % 2).astype(np.uint8)
    return np.full(n, f, dtype=np.uint32), shape, tfh, tfs, swapped


def _device(torch, lib, pkg, hf, sh, tfh, tfs, sw, req, cap):
    dev = torch.device("cuda:0")
    n = len(hf)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_hf, d_sh, d_tfh, d_tfs, d_sw = t(hf.view(np.int32)), t(sh.view(np.int32)), t(tfh), t(tfs), t(sw)
    d_out = torch.full((n * 96,), 0x5A, dtype=torch.uint8, device=dev)
    d_dlb = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    d_con = torch.full(((cap + 2) * 96,), 0x5A, dtype=torch.uint8, device=dev)  # (two guard records behind the capacity)
    nc = lib.hfield_collide_device(d_hf, d_sh, d_tfh, d_tfs, n, req, d_out, d_swapped=d_sw, d_bound=d_dlb, d_contacts=d_con, max_contacts=cap,
                                   want_count=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    con = d_con.cpu().numpy()
    assert (con[cap * 96:] == 0x5A).all(), "a contact was written past the capacity"
    return d_out.cpu().numpy().view(pkg.abi.RESULT_DTYPE), d_dlb.cpu().numpy(), con[:min(nc, cap) * 96].view(pkg.abi.CONTACT_DTYPE), nc


@pytest.mark.parametrize("f", range(len(GRIDS)))
def test_device_equals_harness_and_host_equals_device(pkg, torch_cuda, world, f):
    lib, abi = world["lib"], pkg.abi
    seen_contacts = seen_dropped = seen_free = 0
    for k, n in enumerate(SIZES):
        req = abi.default_collision_request()
        req.security_margin = MARGINS[(k + f) % 3]
        req.num_max_contacts = MAX_CONTACTS[k % 3]
        hf, sh, tfh, tfs, sw = _queries(pkg, world, f, n, rotated=(k % 2 == 1))
        want, want_dlb, want_con, want_nc, n_items = hc.harness_collide(pkg, world["harness"], world["tables"], world["L"], hf, sh, tfh, tfs, req,
                                                                      sw, cap=1 << 16)
        assert want_nc <= 1 << 16
        what = "field %s, %d queries, margin %g, num_max_contacts %d, %d items" % (GRIDS[f], n, req.security_margin, req.num_max_contacts, n_items)
        # a capacity below what is produced (where anything is): counted and dropped
        cap = want_nc // 2 if want_nc > 1 and k % 2 == 0 else want_nc
        # the device form: one chunk; chunks of 7 queries inside the call (the contact offsets and hfcl_contact::pair carried from chunk
        # to chunk); chunks cut down because they list more than 50 items (a chunk of one query is never cut)
        for chunk, items in ((0, 0), (7, 0), (0, 50)):
            lib.set_option("hfield_chunk", chunk)
            lib.set_option("hfield_items", items)
            got, dlb, con, nc = _device(torch_cuda, lib, pkg, hf, sh, tfh, tfs, sw, req, cap)
            assert nc == want_nc, (what, chunk, items)
            assert hc.compare_records(got, want) == [], (what, chunk, items)
            assert dlb.tobytes() == want_dlb.tobytes(), (what, chunk, items)
            assert con.tobytes() == want_con[:cap].tobytes(), (what, chunk, items)
        lib.set_option("hfield_items", 0)
        for chunk in (0, 7):  # the host form, whole and in chunks of 7 queries
            lib.set_option("hfield_chunk", chunk)
            h_out, h_dlb, h_con, h_nc = lib.hfield_collide(hf, sh, tfh, tfs, req, swapped=sw, max_contacts=cap)
            assert h_nc == nc and h_out.tobytes() == got.tobytes() and h_dlb.tobytes() == dlb.tobytes() and h_con.tobytes() == con.tobytes(), what
        lib.set_option("hfield_chunk", 0)
        seen_contacts += want_nc
        seen_dropped += want_nc - cap
        seen_free += int((want["num_contacts"] == 0).sum())
        assert (got["status"] & abi.STATUS_SWAPPED != 0).tolist() == sw.astype(bool).tolist()
    assert seen_contacts > 0 and seen_dropped > 0 and seen_free > 0


def test_requests_refused_before_any_work(pkg, torch_cuda, world):
    lib, abi = world["lib"], pkg.abi
    hf, sh, tfh, tfs, sw = _queries(pkg, world, 3, 6, rotated=False)

    def code(**kw):
        req = abi.default_collision_request()
        for k, v in kw.items():
            setattr(req.q if hasattr(req.q, k) else req, k, v)
        try:
            lib.hfield_collide(hf, sh, tfh, tfs, req, swapped=sw)
        except pkg.engine.EngineError as e:
            return e.code
        return abi.OK

    assert code() == abi.OK
    assert code(num_max_contacts=0) == abi.ERR_INVALID_ARGUMENT
    assert code(epa_max_iterations=65) == abi.ERR_LIMIT
    assert code(gjk_initial_guess=abi.CachedGuess) == abi.ERR_LIMIT
    assert code(gjk_initial_guess=abi.BoundingVolumeGuess) == abi.ERR_LIMIT
    assert code(distance_upper_bound=1.0) == abi.ERR_LIMIT
    # a solid without an evaluator, a field that is not there
    L2 = pkg.geometry.ShapeLibrary()
    L2.add_sphere(0.2)
    L2.add_halfspace((0, 0, 1), 0.0)
    lib2 = pkg.Library(L2)
    lib2.add_hfield(1.0, 1.0, np.ones((2, 2)), 0.0)
    tf = pkg.geometry.make_pose().reshape(1, 12)
    for ids, want in ((([0], [1]), abi.ERR_UNSUPPORTED_PAIR), (([1], [0]), abi.ERR_INVALID_ARGUMENT)):
        with pytest.raises(pkg.engine.EngineError) as e:
            lib2.hfield_collide(ids[0], ids[1], tf, tf)
        assert e.value.code == want
    # -inf margin: every record skipped
    req = abi.default_collision_request()
    req.security_margin = -np.inf
    out, dlb, con, nc = lib.hfield_collide(hf, sh, tfh, tfs, req, swapped=sw, max_contacts=4)
    assert nc == 0 and (abi.status_skipped(out["status"]) == 1).all() and (dlb == np.finfo(np.float64).max).all()
    assert np.array_equal(lib2.hfield_local_aabb(0), [-0.5, -0.5, 0.0, 0.5, 0.5, 1.0])
    lib2.close()


def test_clear_hfields_and_compat_pruning(pkg, torch_cuda):
    """hfcl_lib_clear_hfields: indices start over and the next registrations answer for themselves; compat: a field whose heights are
    updated every step keeps at most HFIELDS_MAX registrations, on the context and on the library."""
    L = pkg.geometry.ShapeLibrary()
    sphere = L.add_sphere(1.0)
    lib = pkg.Library(L)
    tf, at19 = pkg.geometry.make_pose().reshape(1, 12), pkg.geometry.make_pose(T=np.array([[0.0, 0.0, 1.9]]))
    for value, hit in ((1.0, 1), (0.5, 0), (1.0, 1)):
        lib.clear_hfields()
        assert lib.hfield_count() == 0 and lib.add_hfield(1.0, 2.0, np.full((2, 20), value), 0.0) == 0
        assert lib.hfield_collide([0], [sphere], tf, at19)[0]["num_contacts"][0] == hit
    lib.clear_hfields()
    with pytest.raises(pkg.engine.EngineError):
        lib.hfield_collide([0], [sphere], tf, at19)
    lib.close()
    fcl = pkg.compat
    field, ball = fcl.HeightFieldAABB(1.0, 2.0, np.full((2, 20), 1.0), 0.0), fcl.Sphere(1.0)
    ctx = fcl._context()
    for step in range(3 * ctx.HFIELDS_MAX):
        value = 1.0 if step % 2 == 0 else 0.5
        field.updateHeights(np.full((2, 20), value))
        res = fcl.CollisionResult()
        fcl.collide(field, fcl.Transform3f(), ball, fcl.Transform3f(np.eye(3), np.array([0.0, 0.0, 1.9])), fcl.CollisionRequest(), res)
        assert res.isCollision() == (value == 1.0), step
        assert len(ctx.hfields) <= ctx.HFIELDS_MAX and ctx.library().hfield_count() <= ctx.HFIELDS_MAX


def test_golden_cases_through_the_c_abi(pkg, torch_cuda):
    kat = hc.load_kat()
    fields, L, batches = hc.golden_batches(pkg, kat)
    lib = pkg.Library(L)
    for _, x_dim, y_dim, h, mh in fields:
        lib.add_hfield(x_dim, y_dim, h, mh)
    seen = 0
    for m, idx, hf, sh, tfh, tfs in batches:
        req = pkg.abi.default_collision_request()
        req.security_margin = m
        out, dlb, con, nc = lib.hfield_collide(hf, sh, tfh, tfs, req, max_contacts=len(idx))
        assert nc == int((out["num_contacts"] > 0).sum())
        for k, i in enumerate(idx):
            hc.check_golden(kat["cases"][i], int(out[k]["num_contacts"]), float(out[k]["distance"]), out[k]["normal"], float(dlb[k]))
            seen += 1
    assert seen == len(kat["cases"])
    lib.close()


def test_golden_cases_through_compat(pkg, torch_cuda):
    fcl = pkg.compat
    kat = hc.load_kat()
    made = {}
    for c in kat["cases"]:
        if c["field"] not in made:
            s = kat["fields"][c["field"]]
            made[c["field"]] = fcl.HeightFieldAABB(s["x_dim"], s["y_dim"], hc.field_heights(s), s["min_height"])
        field, sphere = made[c["field"]], fcl.Sphere(c["solid"]["radius"])
        for swapped in (False, True):
            req, res = fcl.CollisionRequest(), fcl.CollisionResult()
            req.security_margin = c["security_margin"]
            tfh, tfs = fcl.Transform3f(np.eye(3), np.array(c["tf_hfield"], dtype=float)), fcl.Transform3f(np.eye(3), np.array(c["tf_solid"], dtype=float))
            if swapped:
                fcl.ComputeCollision(sphere, field)(tfs, tfh, req, res)
            else:
                fcl.collide(field, tfh, sphere, tfs, req, res)
            sign = -1.0 if swapped else 1.0
            con = res.getContact(0) if res.isCollision() else None
            hc.check_golden(c, res.numContacts(), con.penetration_depth if con else 0.0, sign * con.normal if con else None, res.distance_lower_bound)
            if con is not None:
                assert (con.b1 == -1 and con.b2 >= 0) if swapped else (con.b1 >= 0 and con.b2 == -1)
    # updateHeights: building_constant_hfields' steps on ONE object
    s = kat["fields"]["const_20x2"]
    field, sphere = fcl.HeightFieldAABB(s["x_dim"], s["y_dim"], hc.field_heights(s), s["min_height"]), fcl.Sphere(1.0)
    tfs = fcl.Transform3f(np.eye(3), np.array([0.0, 0.0, 1.9]))
    for value, hit in ((1.0, True), (0.5, False), (1.0, True)):
        field.updateHeights(np.full((2, 20), value))
        res = fcl.CollisionResult()
        fcl.collide(field, fcl.Transform3f(), sphere, tfs, fcl.CollisionRequest(), res)
        assert res.isCollision() == hit
    with pytest.raises(ValueError):
        fcl.collide(field, fcl.Transform3f(), fcl.Halfspace((0, 0, 1), 0.0), tfs, fcl.CollisionRequest(), fcl.CollisionResult())


def test_cpp_shim(pkg, torch_cuda, tmp_path):
    exe = str(tmp_path / "test_hfield_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_hfield", "test_hfield_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        f.write(hc.kat_as_lines(hc.load_kat()))
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases passed: 40" in r.stdout and "FAILED" not in r.stdout and "updateHeights ok, halfspace refused" in r.stdout and "same address ok" in r.stdout
