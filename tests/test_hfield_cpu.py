"""HeightField<AABB> x convex solid collide() (include/hppfcl_amd_hfield.h) without a GPU: the C ABI's host-only parts, the builder
against the fp64 model (tests/hfield_model.py), the reference's own cases (tests/golden/hfield_kat.json) through the model, and the
device header built with g++ (tests/hfield_harness) against the model on the golden cases and on seeded random queries."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import hfield_cases as hc  # noqa: E402
import hfield_model as hm  # noqa: E402

pkg = ge.load_pkg()
abi, engine, geometry = pkg.abi, pkg.engine, pkg.geometry

MARGINS = (0.0, 0.05, -0.02)
MAX_CONTACTS = (1, 2, 1000)
N_RANDOM = 2016  # 224 queries for each (margin, num_max_contacts)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return hc.build_harness(tmp_path_factory.mktemp("hfield_harness"))


@pytest.fixture(scope="module")
def kat():
    return hc.load_kat()


# ---- 1. symbols ------------------------------------------------------------------------------------------------------------------
def test_symbols():
    lib = engine.dll()
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_hfield.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_[a-z0-9_]*hfield[a-z0-9_]*)\s*\(", hdr)))
    assert syms == sorted(engine.HFIELD_SYMBOLS) and len(syms) == 8
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    older = (engine.EXPORTED_SYMBOLS + engine.CULL_SYMBOLS + engine.NEAREST_SYMBOLS + engine.PAIRS_SYMBOLS + engine.GROUPS_SYMBOLS +
             engine.NEAREST_SELF_SYMBOLS + engine.ENV_SYMBOLS + engine.NEAREST_ENV_SYMBOLS)
    assert not set(syms) & set(older)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert len(re.findall(r'#include "[./]*hppfcl_amd_hfield\.h"', main)) == 1
    assert main.index("hppfcl_amd_nearest_env.h") < main.index("hppfcl_amd_hfield.h") < main.index("hppfcl_amd_pairs.h")  # (the pairs header stays last)
    assert lib.hfcl_abi_version() == 5
    for t in (abi.HF_GEOM_AABB, abi.HF_GEOM_OBBRSS):  # the height-field node types stay unsupported in the per-pair matrix
        for other in (9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 5, 20, 21):
            for for_distance in (0, 1):
                assert lib.hfcl_pair_supported(C.c_int32(t), C.c_int32(other), C.c_int(for_distance)) == 0
                assert lib.hfcl_pair_supported(C.c_int32(other), C.c_int32(t), C.c_int(for_distance)) == 0
    for t in (9, 10, 11, 12, 13, 14, 19):
        assert engine.hfield_pair_supported(t)
    for t in (15, 16, 17, 5, 0, 18, 20, 21, -1):
        assert not engine.hfield_pair_supported(t)
    assert "hfield_chunk" in engine.option_keys() and "hfield_items" in engine.option_keys()
    for m in ("clear_hfields", "add_hfield", "hfield_collide", "hfield_collide_device", "hfield_count", "hfield_local_aabb"):
        assert hasattr(engine.Library, m), m


# ---- 2. the builder -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(2, 2), (3, 2), (2, 3), (4, 3), (5, 7), (100, 100)])
def test_builder_equals_model(nx, ny):
    rng = np.random.default_rng(100 * nx + ny)
    h = rng.uniform(-0.4, 1.5, (ny, nx))  # some samples below min_height: clamped
    x_dim, y_dim, mh = 1.7, 2.9, -0.2
    # (a cell flat at min_height is refused: lift one corner of any such cell)
    c = np.maximum(h, mh)
    for y in range(ny - 1):
        for x in range(nx - 1):
            if (c[y:y + 2, x:x + 2] == mh).all():
                h[y + 1, x + 1] = c[y + 1, x + 1] = 0.3
    nodes, xg, yg = engine.hfield_build(x_dim, y_dim, h, mh)
    F = hm.Field(x_dim, y_dim, h, mh)
    assert len(nodes) == len(F.nodes) == 2 * (nx - 1) * (ny - 1) - 1
    assert xg.tobytes() == np.array(F.x_grid).tobytes() and yg.tobytes() == np.array(F.y_grid).tobytes()
    assert xg[0] == -x_dim / 2 and xg[-1] == x_dim / 2 and yg[0] == y_dim / 2 and yg[-1] == -y_dim / 2
    for a, b in zip(nodes, F.nodes):
        for k in ("first_child", "x_id", "x_size", "y_id", "y_size", "contact_active_faces"):
            assert int(a[k]) == b[k], (k, a, b)
        assert np.float64(a["max_height"]).tobytes() == np.float64(b["max_height"]).tobytes()
        assert a["aabb_min"].tobytes() == np.array(b["aabb_min"]).tobytes() and a["aabb_max"].tobytes() == np.array(b["aabb_max"]).tobytes()
    assert nodes[0]["max_height"] == np.maximum(h, mh).max()


def test_builder_refusals():
    d = engine.dll()
    n = C.c_size_t(0)

    def build(h, ny, nx, mh=0.0):
        h = np.ascontiguousarray(h, dtype=np.float64)
        return d.hfcl_hfield_build(C.c_double(1.0), C.c_double(1.0), abi.ptr(h), C.c_size_t(ny), C.c_size_t(nx), C.c_double(mh), None,
                                   C.byref(n), None, None)

    assert build(np.ones((2, 2)), 2, 2) == abi.OK and n.value == 1
    assert build(np.ones((3, 1)), 3, 1) == abi.ERR_INVALID_ARGUMENT
    assert build(np.ones((1, 3)), 1, 3) == abi.ERR_INVALID_ARGUMENT
    for bad in (np.nan, np.inf, -np.inf):
        h = np.ones((3, 3))
        h[1, 2] = bad
        assert build(h, 3, 3) == abi.ERR_INVALID_ARGUMENT
        assert "non-finite" in engine.last_error()
    h = np.ones((3, 3))
    h[1:, 1:] = -5.0  # the cell (1, 1) is flat at min_height after the clamp
    assert build(h, 3, 3, 0.0) == abi.ERR_INVALID_ARGUMENT
    assert "min_height" in engine.last_error()
    assert build(np.ones((3, 3)), 3, 3, 1.0) == abi.ERR_INVALID_ARGUMENT  # every cell flat
    one = np.ones(4)
    assert d.hfcl_hfield_build(C.c_double(1.0), C.c_double(1.0), abi.ptr(one), C.c_size_t(2), C.c_size_t(32769), C.c_double(0.0), None,
                               C.byref(n), None, None) == abi.ERR_LIMIT
    assert d.hfcl_hfield_build(C.c_double(1.0), C.c_double(1.0), None, C.c_size_t(2), C.c_size_t(2), C.c_double(0.0), None, C.byref(n), None,
                               None) == abi.ERR_INVALID_ARGUMENT


def test_golden_tree_facts(kat):
    """test_hfield_bin_active_faces (7 nodes, the faces per leaf) and the grid end points, through the builder and the model"""
    spec = kat["fields"][kat["bin_active_faces"]["field"]]
    h = hc.field_heights(spec)
    nodes, xg, yg = engine.hfield_build(spec["x_dim"], spec["y_dim"], h, spec["min_height"])
    F = hm.Field(spec["x_dim"], spec["y_dim"], h, spec["min_height"])
    assert len(nodes) == len(F.nodes) == kat["bin_active_faces"]["n_nodes"]
    want = {(l["x_id"], l["y_id"]): l["faces"] for l in kat["bin_active_faces"]["leaves"]}
    for tree in (nodes, F.nodes):
        leaves = {(int(n["x_id"]), int(n["y_id"])): int(n["contact_active_faces"]) for n in tree if n["x_size"] == 1 and n["y_size"] == 1}
        assert leaves == want
    for name, spec in kat["fields"].items():
        _, xg, yg = engine.hfield_build(spec["x_dim"], spec["y_dim"], hc.field_heights(spec), spec["min_height"])
        assert xg[0] == -spec["x_dim"] / 2 and xg[-1] == spec["x_dim"] / 2 and yg[0] == spec["y_dim"] / 2 and yg[-1] == -spec["y_dim"] / 2, name
    s = kat["fields"]["single_bin"]
    assert len(engine.hfield_build(s["x_dim"], s["y_dim"], hc.field_heights(s), s["min_height"])[0]) == kat["single_bin_nodes"]


# ---- 3. / 4. the golden cases: model, then harness against model -------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_runs(kat):
    """the model's answers on every golden case, computed once"""
    fields, L, batches = hc.golden_batches(pkg, kat)
    model_fields = [hm.Field(x, y, h, mh) for _, x, y, h, mh in fields]
    runs = []
    for m, idx, hf, sh, tfh, tfs in batches:
        req = abi.default_collision_request()
        req.security_margin = m
        runs.append((req, idx, hf, sh, tfh, tfs, hm.collide(model_fields, hf, L.shapes_array(), L.vertices_array(), sh, tfh, tfs, req)))
    return fields, L, runs


def test_model_passes_golden_cases(kat, golden_runs):
    _, _, runs = golden_runs
    seen = 0
    for req, idx, hf, sh, tfh, tfs, (recs, bounds, contacts, near) in runs:
        for k, i in enumerate(idx):
            hc.check_golden(kat["cases"][i], recs[k]["num_contacts"], recs[k]["distance"], recs[k]["normal"], bounds[k])
            seen += 1
    assert seen == len(kat["cases"]) == 40


def records_against_model(got, dlb, contacts, recs, bounds, model_contacts, keep, needed):
    """Integers and the contact order equal; floats bit-equal or within 1e-12 absolute (the reference's own length resolution: `prec` of
    binCorrection, collision_distance_threshold).  needed: the float fields that were not bit-equal somewhere."""
    def same(a, b, what):
        a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
        assert np.array_equal(np.isnan(a), np.isnan(b)), what
        if a.tobytes() != b.tobytes():
            ok = np.isnan(a) | (a == b) | (np.abs(a - b) <= 1e-12)
            assert ok.all(), (what, a, b)
            needed.add(what[0])

    for i in np.flatnonzero(keep):
        r = recs[i]
        assert int(got[i]["num_contacts"]) == r["num_contacts"], i
        assert (int(got[i]["b1"]), int(got[i]["b2"])) == (r["b1"], r["b2"]), i
        assert got[i]["status"] == (15 << 3) | (128 if r["num_contacts"] else 0) | (abi.STATUS_SWAPPED if r["swapped"] else 0), i
        for k in hc.FLOAT_FIELDS:
            same(got[i][k], r[k], ("record." + k, i))
        same(dlb[i], bounds[i], ("bound", i))
    mine = [c for c in contacts if keep[c["pair"]]]
    theirs = [c for c in model_contacts if keep[c["pair"]]]
    assert [(int(c["pair"]), int(c["b1"]), int(c["b2"])) for c in mine] == [(c["pair"], c["b1"], c["b2"]) for c in theirs]
    for a, b in zip(mine, theirs):
        same(a["penetration_depth"], b["depth"], ("contact.depth", b["pair"]))
        for k in ("normal", "p1", "p2"):
            same(a[k], b[k], ("contact." + k, b["pair"]))


def test_harness_equals_model_on_golden_cases(kat, harness, golden_runs):
    fields, L, runs = golden_runs
    hf_tables = hc.HarnessFields(pkg, fields)
    needed = set()
    for req, idx, hf, sh, tfh, tfs, (recs, bounds, contacts, near) in runs:
        got, dlb, con, n_con, _ = hc.harness_collide(pkg, harness, hf_tables, L, hf, sh, tfh, tfs, req, cap=len(idx))
        assert n_con == len(contacts)
        records_against_model(got, dlb, con, recs, bounds, contacts, np.ones(len(idx), dtype=bool), needed)  # (golden cases are never rejected)
        for k, i in enumerate(idx):
            hc.check_golden(kat["cases"][i], int(got[k]["num_contacts"]), float(got[k]["distance"]), got[k]["normal"], float(dlb[k]))
    print("golden cases: fields that needed the 1e-12 tolerance:", sorted(needed))


def test_harness_equals_model_on_random_queries(harness):
    rng = np.random.default_rng(20)
    fields = hc.random_fields(rng)
    L, solids = hc.seven_solids(pkg, rng)
    hf_tables = hc.HarnessFields(pkg, fields)
    model_fields = [hm.Field(x, y, h, mh) for _, x, y, h, mh in fields]
    per = N_RANDOM // (len(MARGINS) * len(MAX_CONTACTS))
    needed, rejected, total, in_contact, kinds, both_orders = set(), 0, 0, 0, set(), set()
    for margin in MARGINS:
        for nmax in MAX_CONTACTS:
            hf, sh, tfh, tfs, sw = hc.random_queries(pkg, rng, fields, solids, per)
            req = abi.default_collision_request()
            req.security_margin = margin
            req.num_max_contacts = nmax
            recs, bounds, contacts, near = hm.collide(model_fields, hf, L.shapes_array(), L.vertices_array(), sh, tfh, tfs, req, sw)
            got, dlb, con, n_con, n_items = hc.harness_collide(pkg, harness, hf_tables, L, hf, sh, tfh, tfs, req, sw, cap=64 * per)
            assert n_con <= 64 * per
            keep = ~np.array(near)
            records_against_model(got, dlb, con, recs, bounds, contacts, keep, needed)
            rejected += int((~keep).sum())
            total += per
            in_contact += int((got["num_contacts"] > 0).sum())
            kinds |= set(int(s) for s in sh)
            both_orders |= set(int(s) for s in sw)
    print("random queries: %d, in contact %d, rejected near a threshold %d; fields that needed the 1e-12 tolerance: %s"
          % (total, in_contact, rejected, sorted(needed)))
    assert total == N_RANDOM and len(kinds) == 7 and both_orders == {0, 1}
    assert rejected < 0.01 * total
    assert 0.25 * total < in_contact < 0.75 * total


def test_skipped_by_infinite_margin(harness):
    rng = np.random.default_rng(3)
    fields = hc.random_fields(rng)[:1]
    L, solids = hc.seven_solids(pkg, rng)
    hf, sh, tfh, tfs, sw = hc.random_queries(pkg, rng, fields, solids, 5)
    req = abi.default_collision_request()
    req.security_margin = -np.inf
    got, dlb, con, n_con, n_items = hc.harness_collide(pkg, harness, hc.HarnessFields(pkg, fields), L, hf, sh, tfh, tfs, req, sw, cap=8)
    assert n_con == 0 and n_items == 0 and (abi.status_skipped(got["status"]) == 1).all() and (got["num_contacts"] == 0).all()
    assert (dlb == np.finfo(np.float64).max).all()
    recs, bounds, contacts, _ = hm.collide([hm.Field(*fields[0][1:])], hf, L.shapes_array(), L.vertices_array(), sh, tfh, tfs, req, sw)
    assert all(r["skipped"] for r in recs) and not contacts


# ---- 5. entry points without a device ------------------------------------------------------------------------------------------------
def test_entry_points_without_device():
    """No CPU fallback: without a device both compute entry points say so; with one, a null library is an invalid argument.  The
    host-only calls take no device."""
    d = engine.dll()
    req = abi.default_collision_request()
    one = np.zeros(1, dtype=np.uint32)
    tf = geometry.make_pose().reshape(1, 12)
    out = np.zeros(1, dtype=abi.RESULT_DTYPE)
    n = C.c_size_t(7)
    no_device = engine.device_count() == 0
    want = abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT
    rc = d.hfcl_hfield_collide_batch(None, abi.ptr(one), abi.ptr(one), abi.ptr(tf), abi.ptr(tf), C.c_size_t(1), None, C.byref(req), abi.ptr(out),
                                     None, None, C.c_size_t(0), C.byref(n))
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    rc = d.hfcl_hfield_collide_batch_device(None, None, None, None, None, C.c_size_t(1), None, C.byref(req), None, None, None, C.c_size_t(0),
                                            C.byref(n), None)
    assert rc == want and ("no CPU fallback" if no_device else "null library") in engine.last_error()
    assert n.value == 7 and out["status"][0] == 0
    assert d.hfcl_lib_add_hfield(None, C.c_double(1.0), C.c_double(1.0), abi.ptr(np.ones(4)), C.c_size_t(2), C.c_size_t(2), C.c_double(0.0)) == -1
    assert d.hfcl_lib_hfield_count(None) == 0
    assert d.hfcl_lib_clear_hfields(None) == abi.ERR_INVALID_ARGUMENT
    assert d.hfcl_hfield_local_aabb(None, C.c_int(0), abi.ptr(np.zeros(6))) == abi.ERR_INVALID_ARGUMENT


def test_compat_surface_without_device():
    compat = pkg.compat
    h = np.array([[0.2, 0.4, 0.3], [0.5, -1.0, 0.1]])
    f = compat.HeightFieldAABB(2.0, 1.0, h, 0.0)
    assert f.getXDim() == 2.0 and f.getYDim() == 1.0 and f.getMinHeight() == 0.0 and f.getMaxHeight() == 0.5
    assert np.array_equal(f.getHeights(), np.maximum(h, 0.0)) and list(f.getXGrid()) == [-1.0, 0.0, 1.0] and list(f.getYGrid()) == [0.5, -0.5]
    assert len(f.getNodes()) == 3 and f.getNodeType() == abi.HF_GEOM_AABB
    F = hm.Field(2.0, 1.0, h, 0.0)
    f.computeLocalAABB()
    assert tuple(f.aabb_local) == F.local_aabb()
    f.updateHeights(np.array([[0.2, 0.4, 0.3], [0.5, 0.9, 0.1]]))
    assert f.getMaxHeight() == 0.9 and f.getNodes()[0]["max_height"] == 0.9
    with pytest.raises(ValueError):
        f.updateHeights(np.ones((3, 3)))
