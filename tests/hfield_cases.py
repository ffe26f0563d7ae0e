"""Shared pieces of the height-field tests (tests/test_hfield_cpu.py, tests/test_hfield_gpu.py): the golden cases of
tests/golden/hfield_kat.json as fields and queries, the host build of the device header (tests/hfield_harness), seeded random queries."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT_PATH = os.path.join(ROOT, "tests", "golden", "hfield_kat.json")
FLOAT_FIELDS = ("distance", "normal", "p1", "p2")


def load_kat():
    with open(KAT_PATH) as f:
        return json.load(f)


def linspaced(n, low, high):
    step = (high - low) / float(n - 1)
    return np.array([high if i == n - 1 else low + float(i) * step for i in range(n)])


def field_heights(spec):
    """the (ny, nx) heights a golden field describes"""
    h, nx, ny = spec["heights"], spec["nx"], spec["ny"]
    if h["kind"] == "constant":
        return np.full((ny, nx), float(h["value"]))
    X = np.tile(linspaced(nx, -h["extent"], h["extent"])[None, :], (ny, 1))
    Y = np.tile(linspaced(ny, h["extent"], -h["extent"])[:, None], (1, nx))
    if h["kind"] == "square_hole":
        hole = (np.abs(X) < h["dim"]) & (np.abs(Y) < h["dim"])
    elif h["kind"] == "circular_hole":
        hole = X * X + Y * Y <= h["dim"]
    else:
        raise ValueError(h["kind"])
    return np.ones((ny, nx)) - hole.astype(np.float64)


def golden_batches(pkg, kat):
    """The golden cases grouped by security margin: (fields, shape library, [(margin, case indices, hfield, shape, tf_h, tf_s)]).
    fields: [(name, x_dim, y_dim, heights, min_height)] in the order of their ids."""
    names = sorted(kat["fields"])
    fields = [(k, kat["fields"][k]["x_dim"], kat["fields"][k]["y_dim"], field_heights(kat["fields"][k]), kat["fields"][k]["min_height"])
              for k in names]
    L = pkg.geometry.ShapeLibrary()
    solid_id = {}
    for c in kat["cases"]:
        key = (c["solid"]["kind"], c["solid"]["radius"])
        assert key[0] == "sphere"
        if key not in solid_id:
            solid_id[key] = L.add_sphere(key[1])
    batches = []
    for m in sorted({c["security_margin"] for c in kat["cases"]}):
        idx = [i for i, c in enumerate(kat["cases"]) if c["security_margin"] == m]
        hf = np.array([names.index(kat["cases"][i]["field"]) for i in idx], dtype=np.uint32)
        sh = np.array([solid_id[(kat["cases"][i]["solid"]["kind"], kat["cases"][i]["solid"]["radius"])] for i in idx], dtype=np.uint32)
        tfh = pkg.geometry.make_pose(T=np.array([kat["cases"][i]["tf_hfield"] for i in idx], dtype=np.float64))
        tfs = pkg.geometry.make_pose(T=np.array([kat["cases"][i]["tf_solid"] for i in idx], dtype=np.float64))
        batches.append((m, idx, hf, sh, tfh, tfs))
    return fields, L, batches


def kat_as_lines(kat):
    """the golden cases as one line of numbers each, for tests/cpp_hfield/test_hfield_shim.cpp (the layout is in its header comment)"""
    kinds = {"constant": 0, "square_hole": 1, "circular_hole": 2}
    lines = []
    for c in kat["cases"]:
        f, e = kat["fields"][c["field"]], c["expect"]
        h = f["heights"]
        n = e.get("normal", [0.0, 0.0, 0.0])
        v = [f["x_dim"], f["y_dim"], f["nx"], f["ny"], f["min_height"], kinds[h["kind"]], h.get("value", 0.0), h.get("dim", 0.0),
             h.get("extent", 0.0), c["solid"]["radius"]] + list(c["tf_solid"]) + [c["security_margin"], int(e["is_collision"]),
             int("normal" in e)] + list(n) + [int("depth" in e), e.get("depth", 0.0), int("bound" in e), e.get("bound", 0.0)]
        lines.append(" ".join(repr(float(x)) if isinstance(x, float) else str(x) for x in v))
    return "\n".join(lines) + "\n"


def eigen_is_approx(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(((a - b) ** 2).sum()) <= 1e-12 * 1e-12 * min(float((a * a).sum()), float((b * b).sum()))


def check_golden(case, num_contacts, distance, normal, bound):
    """the reference's own assertions on one case: isCollision, and where the test states them the contact's normal (Eigen isApprox),
    its depth and the bound (its isApprox helper: 1e-6 absolute)"""
    e = case["expect"]
    assert (num_contacts > 0) == e["is_collision"], case["name"]
    if "normal" in e:
        assert eigen_is_approx(normal, e["normal"]), (case["name"], normal)
    if "depth" in e:
        assert abs(distance - e["depth"]) <= 1e-6, (case["name"], distance)
    if "bound" in e:
        assert abs(bound - e["bound"]) <= 1e-6, (case["name"], bound)


# ---- the host build of the device header ---------------------------------------------------------------------------------------
def build_harness(out_dir):
    out = os.path.join(str(out_dir), "libhfield_harness.so")
    src = os.path.join(ROOT, "tests", "hfield_harness", "hfield_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-shared", "-o", out, src])
    return C.CDLL(out)


class HarnessFields:
    """the tables of several fields one after the other, as the library keeps them (built by hfcl_hfield_build)"""

    def __init__(self, pkg, fields):
        table, nodes, hs, xs, ys, mins = [], [], [], [], [], []
        no = ho = xo = yo = 0
        for _, x_dim, y_dim, h, mh in fields:
            n, xg, yg = pkg.engine.hfield_build(x_dim, y_dim, h, mh)
            table.append([no, ho, xo, yo, len(n), h.shape[1], h.shape[0]])
            nodes.append(n)
            hs.append(np.maximum(np.asarray(h, dtype=np.float64), mh).ravel())
            xs.append(xg)
            ys.append(yg)
            mins.append(mh)
            no, ho, xo, yo = no + len(n), ho + h.size, xo + len(xg), yo + len(yg)
        self.n = len(fields)
        self.table = np.array(table, dtype=np.uint64)
        self.nodes = np.concatenate(nodes)
        self.heights = np.concatenate(hs)
        self.xgrid = np.concatenate(xs)
        self.ygrid = np.concatenate(ys)
        self.mins = np.array(mins, dtype=np.float64)


def harness_collide(pkg, hh, hf, L, hfield, shape, tfh, tfs, req, swapped=None, cap=0):
    """(records, bounds, contacts, n_produced, n_items) of the harness"""
    abi = pkg.abi
    shapes = np.ascontiguousarray(L.shapes_array())
    verts = np.ascontiguousarray(L.vertices_array(), dtype=np.float64)
    if len(verts) == 0:
        verts = np.zeros((1, 3))
    n = len(hfield)
    hfield = np.ascontiguousarray(hfield, dtype=np.uint32)
    shape = np.ascontiguousarray(shape, dtype=np.uint32)
    tfh = np.ascontiguousarray(tfh, dtype=np.float64).reshape(-1, 12)
    tfs = np.ascontiguousarray(tfs, dtype=np.float64).reshape(-1, 12)
    out = np.zeros(n, dtype=abi.RESULT_DTYPE)
    dlb = np.zeros(n)
    contacts = np.zeros(max(cap, 1), dtype=abi.CONTACT_DTYPE)
    nc, ni = C.c_size_t(0), C.c_size_t(0)
    sw = None if swapped is None else np.ascontiguousarray(swapped, dtype=np.uint8)
    rc = hh.hh_collide(abi.ptr(shapes), C.c_uint32(len(shapes)), abi.ptr(verts), C.c_uint32(hf.n), abi.ptr(hf.table), abi.ptr(hf.mins),
                       abi.ptr(hf.nodes), abi.ptr(hf.heights), abi.ptr(hf.xgrid), abi.ptr(hf.ygrid), abi.ptr(hfield), abi.ptr(shape),
                       abi.ptr(tfh), abi.ptr(tfs), C.c_size_t(n), abi.ptr(sw), C.byref(req), abi.ptr(out), abi.ptr(dlb), abi.ptr(contacts),
                       C.c_size_t(cap), C.byref(nc), None, C.c_size_t(0), C.byref(ni))
    assert rc == 0
    return out, dlb, contacts[:min(nc.value, cap)], int(nc.value), int(ni.value)


# ---- seeded random queries --------------------------------------------------------------------------------------------------------
def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def random_fields(rng):
    """a 5 x 7 and a 9 x 4 field with heights in [0.2, 1.5] over a min_height below them, and a 5 x 7 one with holes down to a lower level"""
    f0 = ("rand_5x7", 3.0, 4.0, rng.uniform(0.2, 1.5, (7, 5)), -0.3)
    f1 = ("rand_9x4", 4.0, 2.5, rng.uniform(0.2, 1.5, (4, 9)), -0.25)
    h = rng.uniform(0.6, 1.5, (7, 5))
    h[rng.uniform(size=h.shape) < 0.25] = 0.05
    f2 = ("holes_5x7", 3.0, 4.0, h, -0.3)
    return [f0, f1, f2]


def seven_solids(pkg, rng):
    """a shape library with one solid of each kind a height field collides with (the box carries a swept-sphere radius)"""
    L = pkg.geometry.ShapeLibrary()
    pts = rng.normal(size=(14, 3))
    pts = 0.3 * pts / np.linalg.norm(pts, axis=1, keepdims=True) * rng.uniform(0.7, 1.0, (14, 1))
    ids = [L.add_box(0.4, 0.3, 0.5, 0.03), L.add_sphere(0.25), L.add_capsule(0.15, 0.4), L.add_cone(0.2, 0.5), L.add_cylinder(0.2, 0.4),
           L.add_ellipsoid(0.3, 0.2, 0.15), L.add_convex(pts)]
    return L, np.array(ids, dtype=np.uint32)


def random_queries(pkg, rng, fields, solid_ids, n):
    """n queries: solids near the surface of a field (about half in contact), fields under rotated and translated poses (a third at the
    identity), every coordinate inside [-8, 8], both operand orders"""
    geo = pkg.geometry
    hfield = rng.integers(0, len(fields), n).astype(np.uint32)
    shape = solid_ids[rng.integers(0, len(solid_ids), n)]
    tfh = geo.make_pose(quat=random_rotations(rng, n), T=rng.uniform(-2.0, 2.0, (n, 3)))
    ident = rng.uniform(size=n) < 1.0 / 3.0
    tfh[ident] = geo.make_pose()
    local = np.zeros((n, 3))
    for i in range(n):
        _, x_dim, y_dim, h, _ = fields[int(hfield[i])]
        ny, nx = h.shape
        u, v = rng.uniform(-0.05, 1.05), rng.uniform(-0.05, 1.05)
        cx, cy = min(max(int(u * (nx - 1)), 0), nx - 2), min(max(int(v * (ny - 1)), 0), ny - 2)
        local[i] = ((u - 0.5) * x_dim, (0.5 - v) * y_dim, h[cy:cy + 2, cx:cx + 2].mean() + rng.uniform(-0.05, 0.85))
    world = geo.transform_point(tfh, local)
    tfs = geo.make_pose(quat=random_rotations(rng, n), T=world)
    swapped = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    assert np.abs(world).max() < 8.0
    return hfield, shape, tfh, tfs, swapped


def compare_records(got, want, fields=FLOAT_FIELDS + ("b1", "b2", "status", "num_contacts")):
    """names of the fields in which two record arrays differ in any byte"""
    return [k for k in fields if got[k].tobytes() != want[k].tobytes()]
