"""Every tuning option (hfcl_lib_set_option) held to the default form, byte for byte: the rows of tests/options_table.py on small fixed-seed
batches.

1. Each family's records WITHOUT any option against the fp64 oracle, with the checker the family's own tests use.
2. One case per (key, value): the family's calls with the option at that value against the same calls with the row's base options alone --
   records, guesses and contact lists byte for byte, every call twice (the two runs byte-equal), and the row's witness (an observable read after
   the call) different from the default run's in at least one of the row's calls: the other form ran.  Size thresholds are set to a value t inside
   the batch and run at n = t - 1, t, t + 1: the witness must switch where the documentation puts it.
3. hfcl_lib_set_option refuses what include/hppfcl_amd.h says it refuses, and a refused call changes nothing; the environment fallback.

Figures are printed before they are asserted (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import fp32_judge
import options_table as ot
from compare import boundary_band, check_parity
from test_bvh_shape import _check_shape_distance_records
from test_gpu_dispatch import mixed_library  # noqa: F401  (the fixture itself: the dispatch tests' mixed library, not a copy)
from test_gpu_parity import _check_bvh_records, _check_distance_records

pytestmark = pytest.mark.gpu

N_SOLIDS, N_HULLS, N_MESH = 2049, 4097, 1025
# call -> (batch, kind, mode).  mode: f64g records and guesses, f64 records (a mesh walk that returns its guess stays in one piece: another form),
# f32 the fp32 entry points, contacts collide() with a contact list (num_max_contacts above every count), after the mixed batch behind a batch of
# mesh pairs alone (what mesh_beside = 2 looks at)
CALLS = {
    "prim_collide": ("prim", "collide", "f64g"), "prim_distance": ("prim", "distance", "f64g"),
    "mix_collide": ("mix", "collide", "f64g"), "mix_distance": ("mix", "distance", "f64g"),
    "prim_collide_f32": ("prim", "collide", "f32"), "prim_distance_f32": ("prim", "distance", "f32"),
    "mix_collide_f32": ("mix", "collide", "f32"), "mix_distance_f32": ("mix", "distance", "f32"),
    "hulls_distance_f32": ("hulls", "distance", "f32"),
    "large_distance": ("large", "distance", "f64g"), "large_collide": ("large", "collide", "f64g"),
    "mm_collide": ("mmc", "collide", "f64"), "mm_distance": ("mmd", "distance", "f64"),
    "ms_collide": ("ms", "collide", "f64"), "ms_contacts": ("ms", "collide", "contacts"), "ms_distance": ("ms", "distance", "f64"),
    "mixed_collide": ("mixed", "collide", "f64"), "mixed_distance": ("mixed", "distance", "f64"), "mixed_after_meshes": ("mixed", "collide", "after"),
    "host_collide": ("mix", "collide", "f64g"), "host_distance": ("prim", "distance", "f64g"),
    "ties_mm_distance": ("ties_mm", "distance", "f64"), "ties_ms_distance": ("ties_ms", "distance", "f64"),
}
assert all(c in CALLS for calls in ot.FAMILIES.values() for c in calls)


def _mmc_batch(pkg):
    """Two 200-triangle meshes against each other (trees of 10 levels: the lanes' stacks hold their walks)."""
    return pkg.workloads.cfg4_mesh_mesh(n=N_MESH, n_variants=2, seg=10, ring=10)


def _ms_batch(pkg):
    """The two 200-triangle meshes against four each of box / sphere / capsule / cone / cylinder / convex, both operand orders."""
    wl, g = pkg.workloads, pkg.geometry
    rng = np.random.default_rng(5)
    meshes = wl.mesh_variants(2, 10, 10)
    L = g.ShapeLibrary()
    for k, m in enumerate(meshes):
        L.add_bvh(k, len(m.vertices))
    for _ in range(4):
        L.add_box(*map(float, rng.uniform(0.2, 0.9, 3)))
        L.add_sphere(float(rng.uniform(0.1, 0.6)))
        L.add_capsule(float(rng.uniform(0.1, 0.4)), float(rng.uniform(0.2, 1.0)))
        L.add_cone(float(rng.uniform(0.1, 0.5)), float(rng.uniform(0.2, 1.0)))
        L.add_cylinder(float(rng.uniform(0.1, 0.5)), float(rng.uniform(0.2, 1.0)))
        L.add_convex(wl.fibonacci_sphere(24) * rng.uniform(0.1, 0.7, 3))
    n = N_MESH
    mesh, solid, swap = rng.integers(0, 2, n), rng.integers(2, len(L), n), rng.random(n) < 0.5
    q1, T1, q2, T2 = wl._poses(rng, n, 1.2)
    b = wl.Batch("options_mesh_x_solid", L, np.where(swap, solid, mesh), np.where(swap, mesh, solid), q1, T1, q2, T2, "collide")
    b.meshes = meshes
    return b


def _ties_batch(pkg, solids):
    """Exact ties, where the forms of a distance() walk can part ways: a UV sphere -- every ring of triangles is the same distance from the axis,
    the triangles around a pole share it -- at the origin, identity rotations, against boxes ON its axis (solids; the batch of
    test_bvh_shape.py::test_gpu_mesh_solid_ties_forms_agree) or against itself further up the axis.  352 queries."""
    wl, g, bb = pkg.workloads, pkg.geometry, pkg.bvh_builder
    mesh = bb.Mesh(*bb.uv_sphere(24, 24, 1.0))
    L = g.ShapeLibrary()
    L.add_bvh(0, len(mesh.vertices))
    radii = [0.05, 0.2, 0.35, 0.5]
    for r in radii:
        L.add_box(r, 0.8 * r, 0.6 * r)
    zs = np.linspace(-0.25, 0.25, 11) if solids else np.linspace(2.05, 3.0, 11)
    n = len(radii) * len(zs)
    ident = np.tile(np.array([1.0, 0, 0, 0]), (8 * n, 1))
    T1, T2 = np.zeros((8 * n, 3)), np.zeros((8 * n, 3))
    T2[:, 2] = np.tile(np.repeat(zs, len(radii)), 8)
    s2 = np.tile(1 + np.tile(np.arange(len(radii)), len(zs)), 8) if solids else np.zeros(8 * n, dtype=np.int64)
    b = wl.Batch("options_ties", L, np.zeros(8 * n, dtype=np.int64), s2, ident, T1, ident, T2, "distance")
    b.meshes = [mesh]
    return b


class Families:
    """The batches (made on first use, never modified), the runs without the option under test (kept: one per call, size and base), and run()."""

    def __init__(self, pkg, mixed_b):
        self.pkg, self.mixed_b, self.batches, self.kept = pkg, mixed_b, {}, {}

    def batch(self, name):
        if name not in self.batches:
            wl = self.pkg.workloads
            self.batches[name] = {
                "prim": lambda: wl.all_primitives(n=N_SOLIDS), "mix": lambda: wl.cfg5_mixed(n=N_SOLIDS, nper=32),
                "hulls": lambda: wl.cfg3_convex_convex(n=N_HULLS, nlib=256), "large": lambda: wl.large_convex(n=N_MESH),
                "mmc": lambda: _mmc_batch(self.pkg),
                "mmd": lambda: wl.cfg4_mesh_mesh_distance(n=N_MESH, n_variants=2, seg=10, ring=10),
                "ms": lambda: _ms_batch(self.pkg), "mixed": lambda: self.mixed_b,
                "ties_mm": lambda: _ties_batch(self.pkg, False), "ties_ms": lambda: _ties_batch(self.pkg, True)}[name]()
        return self.batches[name]

    def request(self, call):
        bname, kind, mode = CALLS[call]
        abi, b = self.pkg.abi, self.batch(bname)
        req = abi.default_distance_request() if kind == "distance" else abi.default_collision_request()
        if bname == "hulls":
            req = self.pkg.workloads.make_request(b, abi)  # (cfg3's request: NesterovAcceleration)
        if mode == "contacts":
            req.num_max_contacts = 10 ** 6
        return req

    def run(self, call, options, n=None, capfd=None, then=None):
        """A fresh library with `options`, the call twice on the first n pairs; {"rec", "guess", "contacts", "obs"} of the second run."""
        pkg = self.pkg
        bname, kind, mode = CALLS[call]
        b = self.batch(bname)
        n = len(b) if n is None else n
        req = self.request(call)
        lib = pkg.workloads.make_library(pkg, b, options=options)
        pkg.engine.dll().hfcl_debug_note_forms(lib._h, C.c_int(1))
        try:
            if bname == "large":
                assert pkg.workloads.register_adjacency(lib, b.shapes, b.verts) == b.n_large
            outs = [self._once(lib, b, n, kind, mode, req) for _ in range(2)]
            obs = observe(pkg, lib)
            if capfd is not None:
                obs["stderr"] = sum(line.startswith("[hfcl pipe]") for line in capfd.readouterr().err.splitlines())
            for f in ("rec", "guess", "contacts"):
                assert _bytes(outs[0][f]) == _bytes(outs[1][f]), "%s %s: two runs of the same call differ in %s" % (call, options, f)
            assert not np.any((outs[1]["rec"]["status"] >> 31) & 1), (call, options)
            if then is not None:
                then(lib, outs[1], obs)
            return dict(outs[1], obs=obs)
        finally:
            lib.close()

    def _once(self, lib, b, n, kind, mode, req):
        s1, s2 = b.s1[:n], b.s2[:n]
        if mode == "f32":
            fn = lib.distance_f32 if kind == "distance" else lib.collide_f32
            return dict(rec=fn(s1, s2, b.pose1_f32[:n], b.pose2_f32[:n], req), guess=None, contacts=None)
        tf1, tf2 = b.tf1[:n], b.tf2[:n]
        fn = lib.distance if kind == "distance" else lib.collide
        if mode == "f64g":
            rec, guess = fn(s1, s2, tf1, tf2, req, want_guess=True)
            return dict(rec=rec, guess=guess, contacts=None)
        if mode == "contacts":
            rec, contacts, produced = lib.collide_contacts(s1, s2, tf1, tf2, req, 64 * n)
            assert produced == len(contacts)
            # (the list is appended to by whichever wave finds a contact first: its order is no part of the result; held in the order
            # of (pair, b1, b2), which names a contact)
            return dict(rec=rec, guess=None, contacts=contacts[np.lexsort((contacts["b2"], contacts["b1"], contacts["pair"]))])
        if mode == "after":
            import torch
            abi, dev = self.pkg.abi, torch.device("cuda:0")
            kinds = b.shapes["type"]
            mm = np.flatnonzero((kinds[s1] == abi.BV_OBBRSS) & (kinds[s2] == abi.BV_OBBRSS))
            rec = None
            for idx in (mm, np.arange(n)):  # the mesh pairs alone, then the whole batch: what the second batch's order follows
                d = [torch.from_numpy(np.ascontiguousarray(x[idx])).to(dev) for x in (s1.astype(np.int32), s2.astype(np.int32), tf1, tf2)]
                out = torch.zeros(len(idx) * 24, dtype=torch.int32, device=dev)
                lib.collide_device(*d, len(idx), req, out)
                torch.cuda.synchronize()
                rec = out.cpu().numpy().view(abi.RESULT_DTYPE).copy()
            return dict(rec=rec, guess=None, contacts=None)
        return dict(rec=fn(s1, s2, tf1, tf2, req), guess=None, contacts=None)

    def default(self, call, base, n=None):
        key = (call, n, tuple(sorted(base.items())))
        if key not in self.kept:
            self.kept[key] = self.run(call, dict(base), n)
        return self.kept[key]


def _bytes(a):
    return None if a is None else a.tobytes()


def observe(pkg, lib):
    """What can be read after a call: forms (the dispatcher's plan, hfcl_debug_last_forms: name -> the values noted under it, in order), kernels,
    buckets, reruns, handed, parts, walk_mm / walk_ms (hfcl_debug_walk_counters)."""
    dll = pkg.engine.dll()
    dll.hfcl_debug_last_forms.restype = C.c_char_p
    forms = {}
    for item in (dll.hfcl_debug_last_forms(lib._h) or b"").decode().split(";"):
        if item:
            k, v = item.split("=")
            forms.setdefault(k, []).append(v)
    obs = dict(forms=forms, kernels=[k for k, _ in lib.last_kernel_breakdown()], buckets=lib.last_bucket_counts(), reruns=lib.last_ordered_reruns(),
               handed=lib.last_epa_handed_over(), parts=lib.last_split_parts())
    for solid, name in ((0, "walk_mm"), (1, "walk_ms")):
        out = (C.c_uint32 * 34)()
        assert dll.hfcl_debug_walk_counters(lib._h, C.c_int(solid), out) == 0
        obs[name] = tuple(int(v) for v in out)
        # of the split tables behind the walk: queries that suspended (the same in every run) and tasks made (varies with the order the waves take
        # them in: compared with zero only)
        obs[name[5:] + "_tasks"], obs[name[5:] + "_suspended"] = int(out[32]), int(out[33])
        obs[name[5:] + "_round_counters"] = obs[name][:32]  # (per round of walk / leaves / resolve: queries, leaves listed, hand-overs, ...)
    return obs


def witness(obs, paths):
    """The observables a row names, as one comparable value ("forms.x": entry x of the plan, None where the plan has no such entry)."""
    out = []
    for p in paths:
        if isinstance(p, tuple):  # (several entries that make ONE observable)
            out.append(witness(obs, p))
            continue
        v = obs
        for part in p.split("."):
            v = v.get(part) if isinstance(v, dict) else None
        out.append(v)
    return out


@pytest.fixture(scope="module")
def fam(pkg, mixed_library):  # noqa: F811
    return Families(pkg, mixed_library)


# ---- 1. the default records of every family against the oracle --------------------------------------------------------------------------
def _sub(b, idx):
    """The pairs idx of batch b, for the checkers that read b.s1 / b.s2 / b.tf1 / b.tf2 / b.shapes / b.verts."""
    class Sub:
        pass
    s = Sub()
    s.shapes, s.verts, s.s1, s.s2, s.tf1, s.tf2 = b.shapes, b.verts, b.s1[idx], b.s2[idx], b.tf1[idx], b.tf2[idx]
    return s


def _check_ms_collide(abi, b, got, ref, what, margin=0.0, allowed=0):
    """mesh x solid collide() records against the oracle's, as tests/test_bvh_shape.py::test_gpu_mesh_vs_shapes holds them: the decision and the
    first contact's triangle exact away from the decision boundary (d = margin, the request's security_margin; `allowed` oracle records within
    1e-9 of it: compare.boundary_band); the depth of a contact, and the bound of a contact-free query against a solid
    whose fitted box is well defined, to 4e-6; against a solid of revolution a positive bound."""
    kinds = b.shapes["type"]
    mixed = (kinds[b.s1] == abi.BV_OBBRSS) != (kinds[b.s2] == abi.BV_OBBRSS)
    assert not ((got["status"] >> 30) & 1).any(), what
    near = boundary_band(ref, margin, allowed=allowed, name=what)
    ok = (got["num_contacts"] == ref["num_contacts"]) | near
    assert ok[mixed].all(), (what, int((~ok[mixed]).sum()))
    m = mixed & ~near & (got["num_contacts"] == ref["num_contacts"])
    assert np.array_equal(got["b1"][m], ref["b1"][m]) and np.array_equal(got["b2"][m], ref["b2"][m]), what
    solid = np.where(kinds[b.s1] == abi.BV_OBBRSS, kinds[b.s2], kinds[b.s1])
    round_solid = np.isin(solid, [abi.GEOM_SPHERE, abi.GEOM_CAPSULE, abi.GEOM_CONE, abi.GEOM_CYLINDER])
    fin = m & (np.abs(ref["distance"]) < 1e300)
    strict = fin & ((ref["num_contacts"] > 0) | ~round_solid)
    err = float(np.abs(got["distance"][strict] - ref["distance"][strict]).max())
    print("    %s: %d mesh x solid records, %d with contacts, max |d - oracle| %.3g" % (what, int(mixed.sum()), int((ref["num_contacts"][mixed] > 0).sum()), err))
    assert err < 4e-6, what
    assert (got["distance"][fin & ~strict] > 0).all(), what
    assert np.array_equal(np.isnan(got["p1"][strict]), np.isnan(ref["p1"][strict])), what
    return mixed, near


def _contact_keys(contacts, keep):
    return sorted((int(p), int(x), int(y)) for p, x, y in zip(contacts["pair"], contacts["b1"], contacts["b2"]) if keep[p])


@pytest.mark.parametrize("family", sorted(ot.FAMILIES))
def test_default_records_match_the_oracle(pkg, oracle, fam, family):
    abi, wl, bb = pkg.abi, pkg.workloads, pkg.bvh_builder
    for call in ot.FAMILIES[family]:
        bname, kind, mode = CALLS[call]
        b, req = fam.batch(bname), fam.request(call)
        got = fam.default(call, {})
        rec = got["rec"]
        what = "%s default" % call
        if family in ("solids64", "host", "large"):
            fn = oracle.distance_batch if kind == "distance" else oracle.collide_batch
            if family == "large":
                oracle.register_hull_neighbors(b.shapes, b.verts)
            try:
                ref = fn(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, req, n_threads=8)
            finally:
                if family == "large":
                    oracle.lib().orc_clear_neighbors()
            if family == "large":  # (tests/test_gpu_parity.py::test_large_hulls_gpu)
                st = check_parity(abi, rec, ref, dist_tol=1e-6, point_tol=1e-5, flag_band=1e-9, name=what)
            else:
                st = check_parity(abi, rec, ref, dist_tol=1e-15, point_tol=1e-9, flag_band=0.0, name=what)
            print("    %s: %s" % (what, st))
            assert 0.05 < st["contact_frac"] < 0.95
        elif family in ("solids32", "hulls32"):
            tf1, tf2 = b.tf_from_f32()
            fn = oracle.distance_batch if kind == "distance" else oracle.collide_batch
            ref = fn(b.shapes, b.verts, b.s1, b.s2, tf1, tf2, req, n_threads=8)
            fp32_judge.judge(pkg, b, req, rec, ref, tf1, tf2, name=what)
            if family == "hulls32":
                assert (ref["distance"] < 0).mean() >= 0.2  # (the EPA tiers have work)
        elif family == "mm":
            ML = bb.MeshLibrary(b.meshes)
            if kind == "collide":
                ref = oracle.bvh_collide_batch(ML, b.s1, b.s2, b.tf1, b.tf2, req, n_threads=8)
                _check_bvh_records(abi, rec, ref, what)
                assert 0.2 < (ref["num_contacts"] > 0).mean() < 0.8
            else:
                ref = oracle.bvh_distance_batch(ML, b.s1, b.s2, b.tf1, b.tf2, n_threads=8)
                _check_distance_records(oracle, ML, b, rec, ref, what)
                assert call.startswith("ties") or 0.2 < (ref["distance"] > 1e-9).mean() < 0.95
        else:  # ms, mixed
            ML = bb.MeshLibrary(b.meshes)
            kinds = b.shapes["type"]
            is_mesh1, is_mesh2 = kinds[b.s1] == abi.BV_OBBRSS, kinds[b.s2] == abi.BV_OBBRSS
            mm, ss = np.flatnonzero(is_mesh1 & is_mesh2), np.flatnonzero(~is_mesh1 & ~is_mesh2)
            if kind == "collide":
                if mode == "contacts":
                    ref, cref = oracle.mixed_collide_batch(b.shapes, b.verts, ML, b.s1, b.s2, b.tf1, b.tf2, req, max_contacts=64 * len(b), n_threads=8)
                else:
                    ref = oracle.mixed_collide_batch(b.shapes, b.verts, ML, b.s1, b.s2, b.tf1, b.tf2, req, n_threads=8)
                mixed, near = _check_ms_collide(abi, b, rec, ref, what)
                frac = (ref["num_contacts"][mixed] > 0).mean()
                assert 0.2 < frac < 0.9, frac
                if mode == "contacts":
                    keep = mixed & ~near & (rec["num_contacts"] == ref["num_contacts"])
                    assert _contact_keys(cref, keep) == _contact_keys(got["contacts"], keep), what
                    assert int(rec["num_contacts"].max()) > 1
                if len(mm):
                    _check_bvh_records(abi, rec[mm], ref[mm], what + " (mesh x mesh)")
                if len(ss):
                    check_parity(abi, rec[ss], ref[ss], dist_tol=1e-15, point_tol=1e-9, flag_band=0.0, name=what + " (solids)")
            else:
                ref = oracle.mixed_distance_batch(b.shapes, b.verts, ML, b.s1, b.s2, b.tf1, b.tf2, req, n_threads=8)
                _check_shape_distance_records(pkg, oracle, ML, b, rec, ref, what, req)
                if len(mm):
                    _check_distance_records(oracle, ML, _sub(b, mm), rec[mm], ref[mm], what + " (mesh x mesh)")
                if len(ss):
                    check_parity(abi, rec[ss], ref[ss], dist_tol=1e-15, point_tol=1e-9, flag_band=0.0, name=what + " (solids)")


# ---- 2. the rows -------------------------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    for row in ot.ROWS:
        if isinstance(row, ot.Covered):
            continue
        if row.threshold is not None:
            out.append(pytest.param(row, None, id="%s~%s[%s]" % (row.key, row.threshold.t, row.family)))
        for v in row.values:
            out.append(pytest.param(row, v, id="%s=%s[%s]" % (row.key, v, row.family)))
    return out


def _differences(x, y, batch=None):
    """Where two arrays of records differ, in words: the fields, the records, the largest difference per float field, the first records' kinds."""
    if len(x) != len(y):
        return "lengths %d / %d" % (len(x), len(y))
    fields = [k for k in x.dtype.names if x[k].tobytes() != y[k].tobytes()]
    rows = np.flatnonzero(np.any([(x[k].reshape(len(x), -1).view(np.uint8) != y[k].reshape(len(y), -1).view(np.uint8)).any(axis=1) for k in fields], axis=0))
    detail = "fields %s, %d of %d records (first %s)" % (fields, len(rows), len(x), rows[:6].tolist())
    for k in fields:
        if x[k].dtype.kind == "f":
            with np.errstate(invalid="ignore", over="ignore"):
                dd = np.abs(x[k].astype(np.float64) - y[k].astype(np.float64))
                detail += "; max |%s difference| %.3g, NaN patterns %s" % (k, float(np.nanmax(dd)) if np.isfinite(dd).any() else 0.0,
                                                                          "equal" if np.array_equal(np.isnan(x[k]), np.isnan(y[k])) else "differ")
    if batch is not None and "num_contacts" in x.dtype.names:
        kinds = batch.shapes["type"]
        detail += "; (record, kind 1, kind 2, contacts, distance, default's): %s" % [
            (int(r), int(kinds[batch.s1[r]]), int(kinds[batch.s2[r]]), int(x["num_contacts"][r]), float(x["distance"][r]), float(y["distance"][r])) for r in rows[:8]]
    return detail


def _count(obs, path):
    v = witness(obs, [path])[0]
    assert isinstance(v, int), path
    return v


def check_expectations(row, value, got, ref, what):
    """The device's own counts of the run at `value` (got) against the run at the row's base (ref): options_table.py, `expect` and `work`."""
    for path in row.work:
        print("    %s: %s = %d (must be above zero: the path had work)" % (what, path, _count(got["obs"], path)))
        assert _count(got["obs"], path) > 0, "%s: %s is zero: the path the option tunes had no work on this batch" % (what, path)
    for path, op in row.expect.get(value, ()):
        x, d = _count(got["obs"], path), _count(ref["obs"], path)
        print("    %s: %s = %d, default %d, expected %s" % (what, path, x, d, op))
        if op.endswith("default"):
            ok = {">default": x > d, "<default": x < d, "!=default": x != d}[op]
        elif op[:2] in ("==", "<=") and not op[2:].lstrip("-").isdigit():
            y = _count(got["obs"], op[2:])
            ok = x == y if op[:2] == "==" else x <= y
        else:
            y = int(op.lstrip("<>=!"))
            ok = {">": x > y, "==": x == y, "<=": x <= y}[op[:len(op) - len(str(y))]]
        assert ok, "%s: %s = %d (default %d): expected %s" % (what, path, x, d, op)


def _same_bytes(a, b, what, batch=None):
    for f in ("rec", "guess", "contacts"):
        if _bytes(a[f]) != _bytes(b[f]):
            raise AssertionError("%s: %s differ from the default form's: %s" % (what, f, _differences(a[f], b[f], batch if f == "rec" else None)))


def _same_decisions(a, b, what):
    """The one exception (options_table.py: decisions_at), fp64 mesh x mesh collide(): every decision byte for byte, the numbers to twice the
    oracle tolerance of test_gpu_parity._check_bvh_records.  Returns the largest differences (distance, witness fields)."""
    x, y = a["rec"], b["rec"]
    for f in ("status", "num_contacts", "b1", "b2"):
        assert x[f].tobytes() == y[f].tobytes(), "%s: %s differs from the default form's" % (what, f)
    worst = []
    for fields, tol in ((("distance",), 2e-6), (("p1", "p2", "normal"), 2e-5)):
        w = 0.0
        for f in fields:
            assert np.array_equal(np.isnan(x[f]), np.isnan(y[f])), "%s: the NaN pattern of %s differs" % (what, f)
            fin = ~np.isnan(x[f]) & (np.abs(y[f]) < 1e300)
            assert np.array_equal(x[f][~fin & ~np.isnan(x[f])], y[f][~fin & ~np.isnan(x[f])]), "%s: %s" % (what, f)
            w = max(w, float(np.abs(x[f][fin] - y[f][fin]).max(initial=0.0)))
        assert w <= tol, "%s: %s differ by %g > %g" % (what, fields, w, tol)
        worst.append(w)
    print("    %s: decisions byte-equal; largest difference: distance %.3g, p1 / p2 / normal %.3g; %d of %d records differ in a byte" % (
        what, worst[0], worst[1], int((x.view(np.uint8).reshape(len(x), -1) != y.view(np.uint8).reshape(len(y), -1)).any(axis=1).sum()), len(x)))
    return worst


def _refused(pkg, lib, key, value):
    with pytest.raises(pkg.EngineError) as e:
        lib.set_option(key, value)
    assert e.value.code == pkg.abi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("row,value", _cases())
def test_option_forms_are_byte_equal(pkg, fam, capfd, row, value):
    """One case per (key, value), one per size threshold.

    The "decisions" values (bvh_coop=0, bvh_walk_rounds=0, bvh_force_wide=1 in mm_collide) measured: distance differs by at most 8.95e-16 in
    158, 66 and 158 of 1025 records; p1 / p2 / normal, status, num_contacts, b1, b2 byte-equal."""
    calls = row.calls or ot.FAMILIES[row.family]
    cap = capfd if row.witness == ("stderr",) else None
    if row.needs_ab and not pkg.engine.has_ab_forms():
        # the product build refuses the form (row.refused), and the refused call leaves the library as it was: the call after it gives the
        # default form's bytes and plan -- also with the row's own option set, where that is another one (a threshold of the refused form)
        key, v = row.refused
        base = {k: x for k, x in row.base.items() if k != key}
        for call in calls:
            n = row.threshold.t if row.threshold else None
            ref = fam.default(call, base, n)
            options = dict(base)
            if row.key != key:
                options[row.key] = row.threshold.t
            after = {}

            def refuse(lib, out, obs):
                _refused(pkg, lib, key, v)
                bname, kind, mode = CALLS[call]
                after.update(fam._once(lib, fam.batch(bname), len(ref["rec"]), kind, mode, fam.request(call)), obs=observe(pkg, lib))

            fam.run(call, options, n, then=refuse)
            _same_bytes(after, ref, "%s after a refused %s=%s" % (call, key, v))
            assert witness(after["obs"], row.witness) == witness(ref["obs"], row.witness)
        return
    if row.threshold is not None:
        t, kind, off = row.threshold
        switched = []
        for n in (t - 1, t, t + 1):
            on = n <= t if kind == "max" else n >= t
            seen = False
            for call in calls:
                ref = fam.default(call, row.base, n)
                at_t = fam.run(call, dict(row.base, **{row.key: t}), n)
                at_off = fam.run(call, dict(row.base, **{row.key: off}), n)
                what = "%s, %d pairs, %s" % (call, n, row.key)
                _same_bytes(at_t, ref, "%s=%s" % (what, t))
                _same_bytes(at_off, ref, "%s=%s" % (what, off))
                w_t, w_off = witness(at_t["obs"], row.witness), witness(at_off["obs"], row.witness)
                print("    %s=%s: %s; =%s: %s" % (what, t, w_t, off, w_off))
                assert on or w_t == w_off, "%s=%s: the form is on at a size where the documentation has it off" % (what, t)
                seen = seen or w_t != w_off
            switched.append(seen)
            assert seen == on, "%s=%s at %d pairs: form %s, documented %s (witness %s)" % (row.key, t, n, seen, on, row.witness)
        return
    differs, failed = [False] * len(row.witness or ()), []
    for call in calls:
        ref = fam.default(call, row.base) if cap is None else fam.run(call, dict(row.base), capfd=cap)
        got = fam.run(call, dict(row.base, **{row.key: value}), capfd=cap)
        what = "%s, %s=%s" % (call, row.key, value)
        changed = [k for k in ("forms", "kernels", "reruns", "walk_mm", "walk_ms", "handed", "parts", "buckets") if got["obs"][k] != ref["obs"][k]]
        if "forms" in changed:
            changed += ["forms." + k for k in sorted(set(got["obs"]["forms"]) | set(ref["obs"]["forms"])) if got["obs"]["forms"].get(k) != ref["obs"]["forms"].get(k)]
        print("    %s: observables that differ from the default run: %s" % (what, changed))
        counts = lambda o: dict(o["reruns"], handed=o["handed"], epa_queue=o["buckets"]["epa_queue"], epa_overflow=o["buckets"]["epa_overflow"],
                                **{k: o[k] for k in ("mm_tasks", "mm_suspended", "ms_tasks", "ms_suspended")})
        print("    %s: device counts %s, default %s" % (what, counts(got["obs"]), counts(ref["obs"])))
        if row.witness is not None:
            w_got, w_ref = witness(got["obs"], row.witness), witness(ref["obs"], row.witness)
            print("    %s: witness %s: %s, default %s" % (what, row.witness, w_got, w_ref))
            differs = [d or x != y for d, x, y in zip(differs, w_got, w_ref)]
        if call == calls[0]:
            check_expectations(row, value, got, ref, what)
        try:  # (every call of the row is run and reported)
            if value in row.decisions_at and call == "mm_collide":
                _same_decisions(got, ref, what)
            else:
                _same_bytes(got, ref, what, fam.batch(CALLS[call][0]))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    if row.witness is None:
        assert row.why, "a row without a witness says why"
    else:
        assert all(differs), "%s=%s: of the witness %s the components %s are the default run's in every call: the other form did not run (a vacuous row)" % (
            row.key, value, row.witness, [p for p, d in zip(row.witness, differs) if not d])


# ---- 3. hfcl_lib_set_option refuses what the header says it refuses, and changes nothing then ------------------------------------------------
def _block(pkg, lib):
    dll = pkg.engine.dll()
    dll.hfcl_debug_options_block.restype = C.c_size_t
    size = dll.hfcl_debug_options_block(lib._h, None, C.c_size_t(0))
    buf = (C.c_uint8 * size)()
    assert dll.hfcl_debug_options_block(lib._h, buf, C.c_size_t(size)) == size
    return bytes(buf)


def _bad_values(key):
    bad = list(ot.GARBAGE)
    bad.append(str(ot.ABOVE[key]))
    if key in ot.BELOW:
        bad.append(str(ot.BELOW[key]))
    bad += [str(v) for v in ot.INSIDE_BUT_REFUSED.get(key, ())]
    bad += list(ot.LISTS.get(key, ()))
    return bad


@pytest.mark.parametrize("key", sorted(ot.TABLE))
def test_set_option_refuses_and_changes_nothing(pkg, fam, key):
    """Garbage, a negative number, a value above (below) the range, a hole of an enumeration, a bad list: HFCL_ERR_INVALID_ARGUMENT each, the
    library's options block the same bytes before and after; and for a key with a row of its own the witness of a setting made before the
    refused calls is still there after them (the call between them is the row's first call at the row's first value)."""
    abi, dll = pkg.abi, pkg.engine.dll()
    valid = "0" if key in ("cvx_w", "bvh_filter", "epa_general_staged") else "1"
    L = pkg.geometry.ShapeLibrary()
    L.add_sphere(0.5)
    lib = pkg.Library(L)
    try:
        before = _block(pkg, lib)
        for bad in _bad_values(key):
            for spelling in (key, "HFCL_" + key.upper()):
                rc = dll.hfcl_lib_set_option(lib._h, spelling.encode(), bad.encode())
                assert rc == abi.ERR_INVALID_ARGUMENT, "%s=%r was not refused (rc %d)" % (spelling, bad, rc)
                assert _block(pkg, lib) == before, "%s=%r was refused but changed the options" % (spelling, bad)
        for spelling in (key, key.upper(), "HFCL_" + key.upper(), "hfcl_" + key, "Hfcl_" + key.capitalize()):  # any letter case, with or without the prefix
            assert dll.hfcl_lib_set_option(lib._h, spelling.encode(), valid.encode()) == abi.OK, spelling
        assert dll.hfcl_lib_set_option(lib._h, (key + "_").encode(), valid.encode()) == abi.ERR_INVALID_ARGUMENT  # (no such key)
    finally:
        lib.close()
    row = next((r for r in ot.TABLE[key] if isinstance(r, ot.Row) and not (r.needs_ab and not pkg.engine.has_ab_forms())), None)
    # (the dispatcher's plan and the kernel list: the device counters of a split walk vary from run to run with the order its waves take tasks in)
    flat = lambda w: [q for p in w for q in (flat(p) if isinstance(p, tuple) else [p])]
    paths = [p for p in (flat(row.witness or ()) if row is not None else ()) if p.startswith("forms.") or p == "kernels"]
    if not paths:
        return
    call = (row.calls or ot.FAMILIES[row.family])[0]
    value, n = (row.threshold.t, row.threshold.t) if row.threshold else (row.values[0], None)
    first = fam.run(call, dict(row.base, **{row.key: value}), n)
    seen = {}

    def refuse_all(lib, out, obs):
        for bad in _bad_values(key):
            assert dll.hfcl_lib_set_option(lib._h, key.encode(), bad.encode()) == abi.ERR_INVALID_ARGUMENT, bad
        bname, kind, mode = CALLS[call]
        b = fam.batch(bname)
        m = len(b) if n is None else n
        seen["again"] = fam._once(lib, b, m, kind, mode, fam.request(call))
        seen["obs"] = observe(pkg, lib)

    fam.run(call, dict(row.base, **{row.key: value}), n, then=refuse_all)
    plain = fam.default(call, row.base, n)
    print("    %s=%s: witness %s before %s, after the refused calls %s, default %s" % (key, value, paths, witness(first["obs"], paths), witness(seen["obs"], paths),
                                                                                    witness(plain["obs"], paths)))
    assert witness(seen["obs"], paths) == witness(first["obs"], paths), key
    assert row.threshold is not None or witness(first["obs"], paths) != witness(plain["obs"], paths), key  # (a threshold's default may be on the same side)
    if not (value in row.decisions_at):
        assert _bytes(seen["again"]["rec"]) == _bytes(first["rec"]), key


def test_environment_fallback_and_a_later_set_option(pkg, fam, monkeypatch):
    """HFCL_<KEY> is read once, when the library is created; hfcl_lib_set_option after that wins.  One boolean and one threshold."""
    b = fam.batch("prim")
    n = 1024
    req = pkg.abi.default_collision_request()

    def forms(lib):
        pkg.engine.dll().hfcl_debug_note_forms(lib._h, C.c_int(1))
        lib.collide(b.s1[:n], b.s2[:n], b.tf1[:n], b.tf2[:n], req)
        return observe(pkg, lib)["forms"]

    lib = pkg.Library(b.lib)
    try:
        plain = forms(lib)
    finally:
        lib.close()
    assert plain["closed_staged"] == ["1"] and plain["epa_direct"] == ["1"]
    monkeypatch.setenv("HFCL_CLOSED_STAGED", "0")
    monkeypatch.setenv("HFCL_EPA_DIRECT_MAX", "1023")
    monkeypatch.setenv("HFCL_CVX_W", "3")  # (a refused value in the environment: ignored, the option stays at its default)
    lib = pkg.Library(b.lib)
    try:
        monkeypatch.delenv("HFCL_CLOSED_STAGED")
        monkeypatch.delenv("HFCL_EPA_DIRECT_MAX")
        monkeypatch.delenv("HFCL_CVX_W")
        env = forms(lib)
        assert env["closed_staged"] == ["0"] and env["epa_direct"] == ["0"] and env["cvx_w_cc"] == plain["cvx_w_cc"]
        lib.set_option("closed_staged", 1)
        lib.set_option("HFCL_EPA_DIRECT_MAX", 1024)
        later = forms(lib)
        assert later["closed_staged"] == ["1"] and later["epa_direct"] == ["1"]
    finally:
        lib.close()
