"""Culling a scene's pair list per configuration on the GPU (include/hppfcl_amd_cull.h).  The yardsticks: the host broadphase's boxes
(engine.world_aabbs) bit for bit, the numpy model of the cull (tests/cull_model.py, held against the definition and the g++ build of the
header in tests/test_scene_cull_cpu.py) exactly, the unculled scene call's records byte for byte, and the numpy fold of those records."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cull_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
FILL = 0x5A5A5A5A5A5A5A5A


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _same(a, b, what):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def _host_boxes(pkg, lib, obj_shape, tf):
    return np.stack([pkg.engine.world_aabbs(lib, obj_shape, tf[c]) for c in range(len(tf))])


def _wide(pkg, pose):
    """7-float poses as the device widens them: doubles, the rotation in pose_from_quat's order of operations (geometry.quat_to_matrix
    restates it; tests/test_scene_cull_cpu.py holds the g++ build of the header against it)."""
    p = pose.reshape(-1, 7)
    return pkg.geometry.make_pose(quat=p[:, :4].astype(np.float64), T=p[:, 4:].astype(np.float64)).reshape(pose.shape[:-1] + (12,))


@pytest.fixture(scope="module")
def planner(pkg, torch_cuda):
    """scene_planner(64, 16): 6 720 queries, 105 pairs per configuration straddle every wave and workgroup boundary.  Its library and
    scene, the host boxes, and the unculled records / guesses / summaries of collide and distance in both precisions, computed once."""
    ps = pkg.workloads.scene_planner(64, 16, seed=1)
    lib = pkg.Library(ps.lib)
    scene = lib.scene(ps.obj_shape, ps.pairs)
    tf, pose = ps.obj_tf, ps.obj_pose_f32
    d = dict(ps=ps, lib=lib, scene=scene, tf=tf, pose=pose, boxes=_host_boxes(pkg, ps.lib, ps.obj_shape, tf),
             boxes32=_host_boxes(pkg, ps.lib, ps.obj_shape, _wide(pkg, pose)))
    creq, dreq = pkg.abi.default_collision_request(), pkg.abi.default_distance_request()
    d["req"] = {"collide": creq, "distance": dreq}
    d["full"] = {("collide", False): scene.collide(tf, creq, want_guess=True), ("distance", False): scene.distance(tf, dreq, want_guess=True),
                 ("collide", True): scene.collide_f32(pose, creq), ("distance", True): scene.distance_f32(pose, dreq)}
    yield d
    scene.close()
    lib.close()


def _cull_device(torch, scene, table, inflate, capacity, f32=False):
    dev = torch.device("cuda:0")
    n_conf = table.shape[0]
    d_tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    d_ids = torch.full((max(capacity, 1),), FILL, dtype=torch.int64, device=dev)
    d_cb = torch.full((n_conf + 1,), FILL, dtype=torch.int64, device=dev)
    d_n = torch.full((1,), FILL, dtype=torch.int64, device=dev)
    scene.cull_device(d_tab, n_conf, inflate, d_ids, capacity, d_cb, d_n, f32=f32, stream=_stream(torch))
    torch.cuda.synchronize()
    return d_ids.cpu().numpy().view(np.uint64), d_cb.cpu().numpy().view(np.uint64), int(d_n.cpu().numpy()[0]), (d_tab, d_ids, d_cb)


# ---- 1. boxes ---------------------------------------------------------------------------------------------------------------------
def test_boxes_equal_the_host_broadphase(pkg, torch_cuda, planner):
    sc = planner["scene"]
    got = sc.world_aabbs(planner["tf"])
    assert got.shape == (64, 16, 6)
    for c in range(64):
        assert got[c].tobytes() == planner["boxes"][c].tobytes(), c
    got32 = sc.world_aabbs(planner["pose"])
    for c in range(64):
        assert got32[c].tobytes() == planner["boxes32"][c].tobytes(), c
    # the device form, on a table that is not 16-byte aligned
    torch = torch_cuda
    d_tab = torch.zeros(64 * 16 * 12 + 1, dtype=torch.float64, device="cuda:0")
    d_tab[1:] = torch.from_numpy(planner["tf"].reshape(-1)).to("cuda:0")
    d_out = torch.zeros(64 * 16 * 6, dtype=torch.float64, device="cuda:0")
    sc.world_aabbs_device(d_tab[1:], 64, d_out, stream=_stream(torch))
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == planner["boxes"].tobytes()


def _mesh_scene(pkg, n_conf=6, seed=5):
    """One BVHModel<OBBRSS> object, a Plane (not aligned with an axis), a Plane aligned with z, and nine solids; all pairs."""
    wl = pkg.workloads
    mesh = wl.mesh_variants(1, 12, 10)[0]
    rng = np.random.default_rng(seed)
    sizes = rng.uniform(0.2, 0.5, 3), rng.uniform(0.2, 0.6, (3, 3)), rng.uniform(0.2, 0.5, (3, 2))
    L, L_host = pkg.ShapeLibrary(), pkg.ShapeLibrary()  # (L_host: without the mesh, for hfcl_world_aabbs, which refuses libraries with one)
    L.add_bvh(0, len(mesh.vertices))
    for lib in (L, L_host):
        lib.add_plane([1, 2, -1], 0.5)
        lib.add_plane([0, 0, 1], -0.75)
        for r in sizes[0]:
            lib.add_sphere(float(r))
        for s in sizes[1]:
            lib.add_box(*map(float, s))
        for s in sizes[2]:
            lib.add_capsule(*map(float, s))
    n_obj = len(L)
    obj_shape = np.arange(n_obj, dtype=np.uint32)
    tf = pkg.geometry.make_pose(quat=wl.uniform_quaternions(rng, n_conf * n_obj), T=rng.uniform(-1.5, 1.5, (n_conf * n_obj, 3))).reshape(n_conf, n_obj, 12)
    tf[1, :, :9] = pkg.geometry.make_pose()[:9]  # a configuration of identity rotations
    i, j = np.triu_indices(n_obj, 1)
    keep = ~((i == 1) & (j == 2))  # (Plane x Plane has no function)
    return mesh, L, L_host, obj_shape, tf, np.stack([i[keep], j[keep]], axis=1).astype(np.uint32)


def _numpy_world_box(lo, hi, tf):
    """CollisionObject::computeAABB in numpy, the operations in hfcl_world_aabbs' order (rotations that are not the identity)."""
    R = tf[:9].reshape(3, 3).T
    out = np.zeros(6)
    for k in range(3):
        a, c = R[k] * lo, R[k] * hi
        mn, mx = np.minimum(a, c), np.maximum(a, c)
        out[k] = tf[9 + k] + ((mn[0] + mn[1]) + mn[2])
        out[3 + k] = tf[9 + k] + ((mx[0] + mx[1]) + mx[2])
    return out


def test_boxes_of_a_mesh_and_a_plane(pkg, torch_cuda):
    mesh, L, L_host, obj_shape, tf, pairs = _mesh_scene(pkg)
    lib = pkg.Library(L)
    lib.add_bvh(mesh)
    scene = lib.scene(obj_shape, pairs)
    try:
        got = scene.world_aabbs(tf)
        v = np.asarray(mesh.vertices, dtype=np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        for c in range(len(tf)):
            exp = np.concatenate([lo + tf[c, 0, 9:], hi + tf[c, 0, 9:]]) if c == 1 else _numpy_world_box(lo, hi, tf[c, 0])
            assert got[c, 0].tobytes() == exp.tobytes(), c
            host = pkg.engine.world_aabbs(L_host, obj_shape[1:] - 1, tf[c, 1:])  # (the other objects)
            assert got[c, 1:].tobytes() == host.tobytes(), c
        assert np.all(np.isinf(got[0, 1])) and np.any(np.isinf(got[0, 2]))  # unbounded after a rotation
        big = np.finfo(np.float64).max
        assert np.array_equal(got[1, 1], [-big] * 3 + [big] * 3) and got[1, 2, 2] == got[1, 2, 5] == -0.75 + tf[1, 2, 11]
        # every pair of a Plane survives in every configuration
        ids, cb = scene.cull(tf, 0.0)
        e_ids, e_cb = cull_model.cull_queries(got, pairs, 0.0)
        _same(ids, e_ids, "mesh / plane scene ids")
        _same(cb, e_cb, "mesh / plane scene conf_begin")
        plane_pairs = np.flatnonzero((pairs == 1).any(axis=1))
        for c in range(len(tf)):
            assert np.all(np.isin(c * len(pairs) + plane_pairs, ids.astype(np.int64))), c
    finally:
        scene.close()
        lib.close()


# ---- 2. the cull equals the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
def test_cull_equals_the_model(pkg, torch_cuda, planner, f32):
    sc, lib, pairs = planner["scene"], planner["lib"], planner["ps"].pairs
    table = planner["pose"] if f32 else planner["tf"]
    boxes = planner["boxes32"] if f32 else planner["boxes"]
    try:
        for inflate in (0.0, 0.25, 1e3):
            e_ids, e_cb = cull_model.cull_queries(boxes, pairs, inflate)
            runs = []
            for chunk in (0, 1000, 0):  # one chunk, chunks that are a multiple of neither 64 nor 105, one chunk again
                lib.set_option("scene_cull_chunk", chunk)
                runs.append(sc.cull(table, inflate))
                ids, cb, n, _ = _cull_device(torch_cuda, sc, table, inflate, 6720, f32)
                runs.append((ids[:n], cb))
            for ids, cb in runs:
                _same(ids, e_ids, "ids, inflate %g" % inflate)
                _same(cb, e_cb, "conf_begin, inflate %g" % inflate)
            if inflate == 1e3:
                assert len(e_ids) == 6720
            else:
                assert 0 < len(e_ids) < 0.1 * 6720 and (inflate > 0 or (np.diff(e_cb.astype(np.int64)) == 0).any())
        lib.set_option("scene_cull_chunk", 1000)
        # a capacity one short.  Host form: HFCL_ERR_LIMIT, the count set, the buffers untouched
        e_ids, e_cb = cull_model.cull_queries(boxes, pairs, 0.25)
        cap = len(e_ids) - 1
        ids = np.full(cap, FILL, dtype=np.uint64)
        cb = np.full(65, FILL, dtype=np.uint64)
        n = C.c_size_t(0)
        tab = np.ascontiguousarray(table)
        fn = pkg.engine.dll().hfcl_scene_cull_f32 if f32 else pkg.engine.dll().hfcl_scene_cull
        rc = fn(sc._h, pkg.abi.ptr(tab), C.c_size_t(64), C.c_double(0.25), pkg.abi.ptr(ids), C.c_size_t(cap), pkg.abi.ptr(cb), C.byref(n))
        assert rc == pkg.abi.ERR_LIMIT and n.value == len(e_ids) and np.all(ids == FILL) and np.all(cb == FILL)
        # device form: the count is true, the ids below the capacity are right, nothing is written past it
        ids, cb, n, _ = _cull_device(torch_cuda, sc, table, 0.25, cap, f32)
        assert n == len(e_ids) and len(ids) == cap
        _same(ids, e_ids[:-1], "ids below the capacity")
        _same(cb, e_cb, "conf_begin with a short capacity")
        # count only
        n = C.c_size_t(0)
        assert fn(sc._h, pkg.abi.ptr(tab), C.c_size_t(64), C.c_double(0.25), None, C.c_size_t(0), None, C.byref(n)) == 0 and n.value == len(e_ids)
    finally:
        lib.set_option("scene_cull_chunk", 0)


def test_cull_nothing_survives(pkg, torch_cuda, planner):
    ps = planner["ps"]
    tf = planner["tf"].copy()
    tf[:, :, 9] += np.arange(16) * 100.0  # the bodies spread out
    sc = planner["scene"]
    ids, cb = sc.cull(tf, 0.0)
    assert len(ids) == 0 and cb.shape == (65,) and not cb.any()
    ids, cb, n, _ = _cull_device(torch_cuda, sc, tf, 0.0, 16)
    assert n == 0 and not cb.any() and np.all(ids == FILL)
    rec, ids, cb, summ = sc.collide_culled(tf)
    assert len(rec) == 0 and len(ids) == 0 and not cb.any()
    assert np.all(np.isposinf(summ["min_distance"])) and np.all(summ["min_pair"] == NONE) and np.all(summ["first_contact"] == NONE)
    assert not summ["n_contacts"].any() and not summ["n_skipped"].any()
    assert len(ps.pairs) == 105


# ---- 3. records --------------------------------------------------------------------------------------------------------------------
def _listed_device(torch, pkg, scene, d_tab, n_conf, d_ids, n, d_cb, kind, req, f32, records=True, summary=True):
    dev = torch.device("cuda:0")
    d_out = torch.zeros(max(n, 1) * (11 if f32 else 24), dtype=torch.int32, device=dev) if records else None
    d_sum = torch.full((n_conf * 6,), 0x7F7F7F7F, dtype=torch.int32, device=dev) if summary else None  # (every summary must be written)
    d_g = None
    if f32:
        fn = scene.distance_listed_device_f32 if kind == "distance" else scene.collide_listed_device_f32
        fn(d_tab, n_conf, d_ids, n, d_cb, req, d_out, d_sum, stream=_stream(torch))
    else:
        d_g = torch.zeros(max(n, 1) * 8, dtype=torch.int32, device=dev) if records else None
        fn = scene.distance_listed_device if kind == "distance" else scene.collide_listed_device
        fn(d_tab, n_conf, d_ids, n, d_cb, req, d_out, d_sum, None, d_g, stream=_stream(torch))
    torch.cuda.synchronize()
    rec = d_out.cpu().numpy().view(pkg.abi.RESULT_F32_DTYPE if f32 else pkg.abi.RESULT_DTYPE)[:n] if records else None
    summ = d_sum.cpu().numpy().view(pkg.abi.SCENE_SUMMARY_DTYPE) if summary else None
    g = d_g.cpu().numpy().view(pkg.abi.GUESS_DTYPE)[:n] if d_g is not None else None
    return rec, summ, g


@pytest.mark.parametrize("kind,f32", [("collide", False), ("distance", False), ("collide", True), ("distance", True)])
def test_records_and_summaries(pkg, torch_cuda, planner, kind, f32):
    """rec_culled[k] is rec_unculled[ids[k]] byte for byte (guesses too in fp64), in the host form and the device form, in one chunk
    and in chunks of 50 and 7 list entries that end inside configurations; the summaries are the numpy fold of the gathered records,
    the summary-only call gives the same, and at inflate 0 n_contacts / first_contact are the unculled summary's."""
    abi = pkg.abi
    sc, lib, req = planner["scene"], planner["lib"], planner["req"][kind]
    table = planner["pose"] if f32 else planner["tf"]
    full = planner["full"][(kind, f32)]
    full_rec, full_summ = full[0], full[1]
    full_g = None if f32 else full[2]
    margin = None if kind == "distance" else 0.0
    culled = sc.distance_culled if kind == "distance" else sc.collide_culled
    try:
        for inflate in (0.0, 0.25):
            e_ids, e_cb = cull_model.cull_queries(planner["boxes32"] if f32 else planner["boxes"], planner["ps"].pairs, inflate)
            k = e_ids.astype(np.int64)
            exp_summ = cull_model.fold_listed(abi, full_rec[k], e_ids, 64, 105, margin)
            empty = np.diff(e_cb.astype(np.int64)) == 0
            assert (empty.any() or inflate > 0) and np.all(np.isposinf(exp_summ["min_distance"][empty])) and np.all(exp_summ["min_pair"][empty] == NONE)
            ids_d, cb_d, n, (d_tab, d_ids, d_cb) = _cull_device(torch_cuda, sc, table, inflate, 6720, f32)
            for chunk in (0, 50, 7):
                lib.set_option("scene_chunk", chunk)
                what = "%s%s inflate %g chunk %d" % (kind, " f32" if f32 else "", inflate, chunk)
                res = culled(table, inflate, req, want_guess=not f32)
                _same(res[1], e_ids, "ids: " + what)
                _same(res[2], e_cb, "conf_begin: " + what)
                _same(res[0], full_rec[k], "host form records: " + what)
                _same(res[3], exp_summ, "host form summaries: " + what)
                if not f32:
                    _same(res[4], full_g[k], "host form guesses: " + what)
                only = culled(table, inflate, req, records=False, want_ids=False)  # (out == NULL, no ids: nothing per query leaves the device)
                assert only[0] is None and only[1] is None
                _same(only[2], e_cb, "summary-only host form conf_begin: " + what)
                _same(only[3], exp_summ, "summary-only host form: " + what)
                rec, summ, g = _listed_device(torch_cuda, pkg, sc, d_tab, 64, d_ids, n, d_cb, kind, req, f32)
                _same(rec, full_rec[k], "device form records: " + what)
                _same(summ, exp_summ, "device form summaries: " + what)
                if not f32:
                    _same(g, full_g[k], "device form guesses: " + what)
                _, summ, _ = _listed_device(torch_cuda, pkg, sc, d_tab, 64, d_ids, n, d_cb, kind, req, f32, records=False)
                _same(summ, exp_summ, "summary-only device form: " + what)
            if inflate == 0.0 and kind == "collide":
                bad = np.flatnonzero((exp_summ["n_contacts"] != full_summ["n_contacts"]) | (exp_summ["first_contact"] != full_summ["first_contact"]))
                boxes = planner["boxes32"] if f32 else planner["boxes"]
                for c in bad:  # a computed contact across a positive box gap: admissible only below the request's gjk_tolerance
                    for p in np.flatnonzero(abi.status_contact(full_rec["status"][c * 105:(c + 1) * 105]) == 1):
                        if c * 105 + p in k:
                            continue
                        a, b = boxes[c, planner["ps"].pairs[p, 0]], boxes[c, planner["ps"].pairs[p, 1]]
                        gap = float(np.max(np.maximum(a[:3] - b[3:], b[:3] - a[3:])))
                        print("configuration %d pair %d: contact across a box gap of %g" % (c, p, gap))
                        assert gap < req.q.gjk_tolerance
                if not f32:
                    assert len(bad) == 0  # (the oracle finds none at this seed: tests/test_scene_cull_cpu.py)
                assert int(exp_summ["n_contacts"].sum()) > 0
    finally:
        lib.set_option("scene_chunk", 0)


def test_mesh_scene_records(pkg, torch_cuda):
    """mesh x solid and solid x solid pairs (and the Planes' pairs, which always survive) in one list: the same identity."""
    mesh, L, L_host, obj_shape, tf, pairs = _mesh_scene(pkg)
    lib = pkg.Library(L)
    lib.add_bvh(mesh)
    scene = lib.scene(obj_shape, pairs)
    try:
        req = pkg.abi.default_collision_request()
        full, full_summ, full_g = scene.collide(tf, req, want_guess=True)
        e_ids, e_cb = cull_model.cull_queries(scene.world_aabbs(tf), pairs, 0.0)
        k = e_ids.astype(np.int64)
        assert 0 < len(k) < len(full) and (pairs[k % len(pairs)] == 0).any() and (pairs[k % len(pairs)] > 2).all(axis=1).any()
        for chunk in (0, 11):
            lib.set_option("scene_chunk", chunk)
            rec, ids, cb, summ, g = scene.collide_culled(tf, 0.0, req, want_guess=True)
            _same(ids, e_ids, "mesh scene ids")
            _same(rec, full[k], "mesh scene records, chunk %d" % chunk)
            _same(g, full_g[k], "mesh scene guesses, chunk %d" % chunk)
            _same(summ, cull_model.fold_listed(pkg.abi, full[k], e_ids, len(tf), len(pairs), 0.0), "mesh scene summaries")
            assert np.array_equal(summ["n_contacts"], full_summ["n_contacts"]) and np.array_equal(summ["first_contact"], full_summ["first_contact"])
    finally:
        lib.set_option("scene_chunk", 0)
        scene.close()
        lib.close()


def test_long_lists_fold_in_pieces(pkg, torch_cuda):
    """A pair list of more than one fold piece (600 pairs, nearly all surviving): the two-launch fold, chunks that cut pieces."""
    rng = np.random.default_rng(31)
    L = pkg.ShapeLibrary()
    for r in rng.uniform(0.3, 0.6, 6):
        L.add_sphere(float(r))
    n_obj, n_conf = 40, 3
    obj_shape = rng.integers(0, 6, n_obj).astype(np.uint32)
    tf = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, n_conf * n_obj), T=rng.uniform(-0.9, 0.9, (n_conf * n_obj, 3))).reshape(n_conf, n_obj, 12)
    tf[1, :, 9] += np.arange(n_obj) * 50.0  # the middle configuration has no survivor
    i, j = np.triu_indices(n_obj, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)[:600]
    lib = pkg.Library(L)
    scene = lib.scene(obj_shape, pairs)
    try:
        req = pkg.abi.default_collision_request()
        req.security_margin = 0.05
        full = scene.collide(tf, req, summary=False)
        e_ids, e_cb = cull_model.cull_queries(_host_boxes(pkg, L, obj_shape, tf), pairs, 0.0)
        assert e_cb[1] > 256 and e_cb[1] == e_cb[2] and e_cb[3] - e_cb[2] > 256
        exp = cull_model.fold_listed(pkg.abi, full[e_ids.astype(np.int64)], e_ids, n_conf, 600, 0.05)
        for chunk in (0, 300, 257, 64):
            lib.set_option("scene_chunk", chunk)
            rec, ids, cb, summ = scene.collide_culled(tf, 0.0, req)
            _same(ids, e_ids, "ids")
            _same(rec, full[e_ids.astype(np.int64)], "records, chunk %d" % chunk)
            _same(summ, exp, "summaries, chunk %d" % chunk)
    finally:
        lib.set_option("scene_chunk", 0)
        scene.close()
        lib.close()


@pytest.mark.parametrize("n_pairs", [100, 600])
def test_sparse_list_spans_more_configurations_than_it_has_entries(pkg, torch_cuda, n_pairs):
    """Twelve configurations, survivors in the first and the last only (three pairs each), empty ones between: a chunk of the list -- the
    whole list of six by default -- spans more configurations than it has entries.  Pair lists of one fold piece (100 pairs) and of
    several (600).  Every configuration's summary is the fold of its records; the device form and the host form agree."""
    abi = pkg.abi
    rng = np.random.default_rng(41)
    L = pkg.ShapeLibrary()
    for r in rng.uniform(0.3, 0.6, 6):
        L.add_sphere(float(r))
    n_obj, n_conf = 40, 12
    obj_shape = rng.integers(0, 6, n_obj).astype(np.uint32)
    T = rng.uniform(-0.1, 0.1, (n_conf, n_obj, 3))  # (spheres of radius >= 0.3 this close are in contact)
    T[:, :, 0] += np.arange(n_obj) * 50.0          # every body far from every other ...
    T[0, 1:3, 0] -= np.arange(1, 3) * 50.0         # ... but bodies 0, 1, 2 together in the first
    T[-1, 1:3, 0] -= np.arange(1, 3) * 50.0        # and the last configuration
    tf = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, n_conf * n_obj), T=T.reshape(-1, 3)).reshape(n_conf, n_obj, 12)
    i, j = np.triu_indices(n_obj, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)[:n_pairs]  # (holds (0, 1), (0, 2), (1, 2))
    lib = pkg.Library(L)
    scene = lib.scene(obj_shape, pairs)
    try:
        req = abi.default_collision_request()
        full, full_summ = scene.collide(tf, req)
        e_ids, e_cb = cull_model.cull_queries(_host_boxes(pkg, L, obj_shape, tf), pairs, 0.0)
        assert len(e_ids) == 6 < n_conf and e_cb[1] == 3 == e_cb[-2] and e_cb[-1] == 6
        k = e_ids.astype(np.int64)
        exp = cull_model.fold_listed(abi, full[k], e_ids, n_conf, n_pairs, 0.0)
        assert exp["n_contacts"][0] > 0 and exp["n_contacts"][-1] > 0
        ids_d, cb_d, n, (d_tab, d_ids, d_cb) = _cull_device(torch_cuda, scene, tf, 0.0, 64)
        assert n == 6
        for chunk in (0, 4, 1):
            lib.set_option("scene_chunk", chunk)
            rec, ids, cb, summ = scene.collide_culled(tf, 0.0, req)
            _same(ids, e_ids, "ids")
            _same(rec, full[k], "records, chunk %d" % chunk)
            _same(summ, exp, "host form summaries, chunk %d" % chunk)
            _, summ_d, _ = _listed_device(torch_cuda, pkg, scene, d_tab, n_conf, d_ids, n, d_cb, "collide", req, False)
            _same(summ_d, exp, "device form summaries, chunk %d" % chunk)
            assert np.array_equal(summ["n_contacts"], full_summ["n_contacts"]) and np.array_equal(summ["first_contact"], full_summ["first_contact"])
    finally:
        lib.set_option("scene_chunk", 0)
        scene.close()
        lib.close()


def test_default_capacity_outgrown_by_the_list(pkg, torch_cuda, planner):
    """No capacity named: the outputs are sized by a guess (an eighth of the queries); a list that outgrows it -- here every query
    survives -- is refused with its length and the call made once more."""
    sc = planner["scene"]
    full = planner["full"][("collide", False)]
    assert sc._list_guess(64) < 6720
    rec, ids, cb, summ, g = sc.collide_culled(planner["tf"], 1e3, planner["req"]["collide"], want_guess=True)
    assert np.array_equal(ids, np.arange(6720)) and np.array_equal(cb, np.arange(65) * 105)
    _same(rec, full[0], "records when everything survives")
    _same(summ, full[1], "summaries when everything survives")
    _same(g, full[2], "guesses when everything survives")


# ---- 5. errors and lifecycle ----------------------------------------------------------------------------------------------------------
def test_errors_and_lifecycle(pkg, torch_cuda, planner):
    abi, d = pkg.abi, pkg.engine.dll()
    ps = planner["ps"]
    lib = pkg.Library(ps.lib)
    scene = lib.scene(ps.obj_shape, ps.pairs)
    try:
        tab = np.ascontiguousarray(planner["tf"])
        req = abi.default_collision_request()
        e_ids, _ = cull_model.cull_queries(planner["boxes"], ps.pairs, 0.0)
        n = C.c_size_t(123)
        out = np.full(len(e_ids), 0x5A, dtype=np.uint8).repeat(96).view(abi.RESULT_DTYPE)
        ids = np.full(len(e_ids), FILL, dtype=np.uint64)
        summ = np.full(64, 0x5A, dtype=np.uint8).repeat(24).view(abi.SCENE_SUMMARY_DTYPE)
        before = out.tobytes(), ids.tobytes(), summ.tobytes()
        untouched = lambda: (out.tobytes(), ids.tobytes(), summ.tobytes()) == before  # noqa: E731

        def culled(inflate, capacity, r=req):
            return d.hfcl_scene_collide_culled(scene._h, abi.ptr(tab), C.c_size_t(64), C.c_double(inflate), C.byref(r), abi.ptr(out),
                                               C.c_size_t(capacity), abi.ptr(ids), None, abi.ptr(summ), None, None, C.byref(n))
        for bad in (-1e-9, -np.inf, np.nan):
            assert culled(bad, len(e_ids)) == abi.ERR_INVALID_ARGUMENT and "inflate" in pkg.engine.last_error()
            assert d.hfcl_scene_cull(scene._h, abi.ptr(tab), C.c_size_t(64), C.c_double(bad), None, C.c_size_t(0), None, C.byref(n)) == abi.ERR_INVALID_ARGUMENT
            d_real = torch_cuda.from_numpy(tab).to("cuda:0")  # (a real table and count: it is `inflate` that is refused)
            d_cnt = torch_cuda.zeros(1, dtype=torch_cuda.int64, device="cuda:0")
            assert d.hfcl_scene_cull_device(scene._h, C.c_void_p(d_real.data_ptr()), C.c_size_t(64), C.c_double(bad), None, C.c_size_t(0), None,
                                            C.c_void_p(d_cnt.data_ptr()), None) == abi.ERR_INVALID_ARGUMENT
            assert "inflate" in pkg.engine.last_error()
        assert untouched() and sum(lib.last_bucket_counts().values()) == 0
        r0 = abi.default_collision_request()
        r0.num_max_contacts = 0
        assert culled(0.0, len(e_ids), r0) == abi.ERR_INVALID_ARGUMENT and untouched()
        # out_capacity too small: refused before any narrow-phase work, the count set
        assert culled(0.0, len(e_ids) - 1) == abi.ERR_LIMIT and n.value == len(e_ids)
        assert untouched() and sum(lib.last_bucket_counts().values()) == 0
        # d_summary without d_conf_begin
        torch = torch_cuda
        ids_d, cb_d, n_d, (d_tab, d_ids, d_cb) = _cull_device(torch, scene, tab, 0.0, 6720)
        d_sum = torch.zeros(64 * 6, dtype=torch.int32, device="cuda:0")
        with pytest.raises(pkg.EngineError) as e:
            scene.collide_listed_device(d_tab, 64, d_ids, n_d, None, req, None, d_sum, stream=_stream(torch))
        assert e.value.code == abi.ERR_INVALID_ARGUMENT and "conf_begin" in str(e.value)
        with pytest.raises(pkg.EngineError):
            scene.collide_listed_device(d_tab, 64, d_ids, n_d, d_cb, req, None, None, stream=_stream(torch))  # records and summaries both NULL
        assert culled(0.0, len(e_ids)) == abi.OK and n.value == len(e_ids) and not untouched()
        _same(ids, e_ids, "ids of the host form")
        _same(out, planner["full"][("collide", False)][0][e_ids.astype(np.int64)], "records of the host form")
        # hfcl_lib_set_shapes invalidates the library's scenes
        shapes, verts = np.ascontiguousarray(ps.lib.shapes_array()), np.ascontiguousarray(ps.lib.vertices_array(), dtype=np.float64)
        assert d.hfcl_lib_set_shapes(lib._h, abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), C.c_size_t(len(verts))) == abi.OK
        after = out.tobytes(), ids.tobytes(), summ.tobytes()
        assert culled(0.0, len(e_ids)) == abi.ERR_INVALID_ARGUMENT and "hfcl_lib_set_shapes" in pkg.engine.last_error()
        assert (out.tobytes(), ids.tobytes(), summ.tobytes()) == after
        for fn in (lambda: scene.cull(tab), lambda: scene.world_aabbs(tab),
                   lambda: scene.collide_listed_device(d_tab, 64, d_ids, n_d, d_cb, req, None, d_sum, stream=_stream(torch))):
            with pytest.raises(pkg.EngineError) as e:
                fn()
            assert "hfcl_lib_set_shapes" in str(e.value)
        fresh = lib.scene(ps.obj_shape, ps.pairs)  # a new scene works again (and the local boxes were rebuilt)
        i2, _ = fresh.cull(tab)
        fresh.close()
        _same(i2, e_ids, "a scene made after hfcl_lib_set_shapes")
    finally:
        scene.close()
        lib.close()


def test_unsupported_pair_among_survivors_and_among_culled(pkg, torch_cuda):
    """distance() has no TriangleP entries.  A triangle pair that survives: HFCL_ERR_UNSUPPORTED_PAIR after all chunks, its record with
    bit 31 and counted, every other record complete.  The same kind only among the culled pairs: not reported, HFCL_OK."""
    abi, d = pkg.abi, pkg.engine.dll()
    L = pkg.ShapeLibrary()
    L.add_sphere(0.5)
    L.add_box(0.4, 0.5, 0.6)
    L.add_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0])
    obj_shape = np.array([0, 1, 2, 0, 1], dtype=np.uint32)
    rng = np.random.default_rng(9)
    tf = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, 10), T=rng.uniform(-0.4, 0.4, (10, 3))).reshape(2, 5, 12)
    i, j = np.triu_indices(5, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    lib = pkg.Library(L)
    scene = lib.scene(obj_shape, pairs)
    try:
        req = abi.default_distance_request()

        def run(table, chunk):
            lib.set_option("scene_chunk", chunk)
            out = np.zeros(2 * len(pairs), dtype=abi.RESULT_DTYPE)
            ids = np.zeros(2 * len(pairs), dtype=np.uint64)
            summ = np.zeros(2, dtype=abi.SCENE_SUMMARY_DTYPE)
            n = C.c_size_t(0)
            tab = np.ascontiguousarray(table)
            rc = d.hfcl_scene_distance_culled(scene._h, abi.ptr(tab), C.c_size_t(2), C.c_double(0.0), C.byref(req), abi.ptr(out), C.c_size_t(len(out)),
                                              abi.ptr(ids), None, abi.ptr(summ), None, None, C.byref(n))
            return rc, out[:n.value], ids[:n.value], summ
        tri = ((obj_shape[i] == 2) | (obj_shape[j] == 2))
        for chunk in (0, 3):
            rc, out, ids, summ = run(tf, chunk)  # everything close together: the triangle's pairs survive
            assert rc == abi.ERR_UNSUPPORTED_PAIR, chunk
            is_tri = tri[ids.astype(np.int64) % len(pairs)]
            assert is_tri.any() and np.array_equal(abi.status_skipped(out["status"]) == 1, is_tri)
            assert int(summ["n_skipped"].sum()) == int(is_tri.sum())
            _same(summ, cull_model.fold_listed(abi, out, ids, 2, len(pairs), None), "summaries beside unsupported pairs")
            assert np.all(np.isfinite(out["distance"][~is_tri]))
        away = tf.copy()
        away[:, 2, 9] += 100.0  # the triangle far from everything: its pairs are culled
        for chunk in (0, 3):
            rc, out, ids, summ = run(away, chunk)
            assert rc == abi.OK, (chunk, pkg.engine.last_error())
            assert len(ids) > 0 and not tri[ids.astype(np.int64) % len(pairs)].any() and not summ["n_skipped"].any()
    finally:
        lib.set_option("scene_chunk", 0)
        scene.close()
        lib.close()


# ---- 6. front ends --------------------------------------------------------------------------------------------------------------------
def test_compat_collide_scene_with_broadphase(pkg, torch_cuda):
    """compat.collide_scene(..., broadphase=True): per configuration, the results of the listed pairs whose boxes overlap -- what
    collide() gives for the pairs a broadphase filter keeps."""
    fcl = pkg.compat
    rng = np.random.default_rng(21)
    geoms = [fcl.Box(0.6, 0.8, 1.0), fcl.Sphere(0.5), fcl.Capsule(0.3, 1.2), fcl.Ellipsoid(0.4, 0.6, 0.8)]
    objs = []
    for k in range(24):
        t = fcl.Transform3f()
        t.setTranslation(rng.uniform(-2.5, 2.5, 3))
        objs.append(fcl.CollisionObject(geoms[k % 4], t))
    i, j = np.triu_indices(24, 1)
    pr = np.stack([i, j], axis=1)
    req = fcl.CollisionRequest()
    got, summ = fcl.collide_scene(objs, pr, req)
    culled, summ_c = fcl.collide_scene(objs, pr, req, broadphase=True)
    mgr, collect = fcl.DynamicAABBTreeCollisionManager(), fcl.CollisionCallBackCollect(10 ** 6)
    mgr.registerObjects(objs)
    mgr.setup()
    mgr.collide(collect)  # the pairs whose boxes overlap, as the manager reports them
    index = {id(o): k for k, o in enumerate(objs)}
    kept = {tuple(sorted((index[id(a)], index[id(b)]))) for a, b in collect.getCollisionPairs()}
    keep = [k for k, (a, b) in enumerate(pr) if (a, b) in kept]
    assert len(keep) == len(kept)
    assert 0 < len(keep) < len(pr) and [k for k, _ in culled] == keep
    expected = fcl.collide_pairs([(objs[pr[k][0]], objs[pr[k][1]]) for k in keep], req)
    n_col = 0
    for (k, g), e, u in zip(culled, expected, [got[k] for k in keep]):
        assert g.numContacts() == e.numContacts() == u.numContacts() and g.distance_lower_bound == e.distance_lower_bound
        for c in range(g.numContacts()):
            a, b = g.getContact(c), e.getContact(c)
            assert a.o1 is b.o1 and a.o2 is b.o2 and a.penetration_depth == b.penetration_depth and np.array_equal(a.pos, b.pos)
        n_col += g.isCollision()
    assert n_col > 0 and summ_c["n_contacts"][0] == n_col == summ["n_contacts"][0] and summ_c["first_contact"][0] == summ["first_contact"][0]
    dist, ids, dsumm = fcl.distance_scene(objs, pr, fcl.DistanceRequest(), broadphase=True, inflate=0.5)
    full, _, fsumm = fcl.distance_scene(objs, pr, fcl.DistanceRequest())
    assert len(dist) == 1 and len(keep) < len(ids[0]) < len(pr) and np.array_equal(dist[0], full[0][ids[0]])
    assert dsumm["min_distance"][0] == dist[0].min() >= fsumm["min_distance"][0]


def test_cpp_shim_cull(tmp_path):
    """include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene::cull / collideCulled / distanceCulled against the unculled Scene (g++ build)."""
    exe = str(tmp_path / "test_cull_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_cull", "test_cull_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("same") == 3 and "DIFFERENT" not in r.stdout
