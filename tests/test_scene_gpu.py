"""Scene queries (hfcl_scene_*) on the GPU.  The yardstick for records is the per-pair entry points (pinned to the oracle elsewhere):
a scene's records are right when they are the per-pair call's records, byte for byte; a summary is right when it is the numpy fold
(abi.fold_records, held against the definition in tests/test_scene_cpu.py) of those records, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _pairs_device(torch, pkg, lib, s1, s2, p1, p2, kind, req, f32=False):
    """The per-pair device call on host-expanded arrays: (records, guesses or None)."""
    abi = pkg.abi
    dev = torch.device("cuda:0")
    n = len(s1)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s1.astype(np.int32), s2.astype(np.int32), p1, p2)]
    d_out = torch.zeros(n * (11 if f32 else 24), dtype=torch.int32, device=dev)
    if f32:
        fn = lib.distance_device_f32 if kind == "distance" else lib.collide_device_f32
        fn(*d, n, req, d_out, stream=_stream(torch))
        torch.cuda.synchronize()
        return d_out.cpu().numpy().view(abi.RESULT_F32_DTYPE), None
    d_g = torch.zeros(n * 8, dtype=torch.int32, device=dev)
    fn = lib.distance_device if kind == "distance" else lib.collide_device
    fn(*d, n, req, d_out, d_gout=d_g, stream=_stream(torch))
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(abi.RESULT_DTYPE), d_g.cpu().numpy().view(abi.GUESS_DTYPE)


def _scene_device(torch, pkg, scene, table, kind, req, f32=False, records=True, summary=True):
    """The scene's device form: (records or None, summaries or None, guesses or None)."""
    abi = pkg.abi
    dev = torch.device("cuda:0")
    n_conf = table.shape[0]
    n = n_conf * scene.n_pairs
    d_tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    d_out = torch.zeros(n * (11 if f32 else 24), dtype=torch.int32, device=dev) if records else None
    d_sum = torch.full((n_conf * 6,), 0x7F7F7F7F, dtype=torch.int32, device=dev) if summary else None  # (every summary must be written)
    d_g = None
    if f32:
        fn = scene.distance_device_f32 if kind == "distance" else scene.collide_device_f32
        fn(d_tab, n_conf, req, d_out, d_sum, stream=_stream(torch))
    else:
        d_g = torch.zeros(n * 8, dtype=torch.int32, device=dev) if records else None
        fn = scene.distance_device if kind == "distance" else scene.collide_device
        fn(d_tab, n_conf, req, d_out, d_sum, None, d_g, stream=_stream(torch))
    torch.cuda.synchronize()
    rec = d_out.cpu().numpy().view(abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE) if records else None
    summ = d_sum.cpu().numpy().view(abi.SCENE_SUMMARY_DTYPE) if summary else None
    g = d_g.cpu().numpy().view(abi.GUESS_DTYPE) if d_g is not None else None
    return rec, summ, g


def _scene_host(scene, table, kind, req, f32=False, records=True, summary=True):
    if f32:
        fn = scene.distance_f32 if kind == "distance" else scene.collide_f32
        res = fn(table, req, records=records, summary=summary)
        res = res if isinstance(res, tuple) else (res,)
        rec = res[0] if records else None
        summ = res[-1] if summary else None
        return rec, summ, None
    fn = scene.distance if kind == "distance" else scene.collide
    res = fn(table, req, records=records, summary=summary, want_guess=records)
    res = res if isinstance(res, tuple) else (res,)
    it = iter(res)
    rec = next(it) if records else None
    summ = next(it) if summary else None
    g = next(it) if records else None
    return rec, summ, g


def _request(pkg, kind, **kw):
    req = pkg.abi.default_distance_request() if kind == "distance" else pkg.abi.default_collision_request()
    for k, v in kw.items():
        setattr(req, k, v)
    return req


def _margin(kind, req):
    return None if kind == "distance" else float(req.security_margin)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def _check_scene(torch, pkg, lib, scene, table, expanded, kind, req, chunks, f32=False, forms=("device", "host")):
    """Every form and chunk size: records and guesses equal to the per-pair device call's, the summary equal to the numpy fold of
    the records, the summary-only call equal to that."""
    s1, s2, p1, p2 = expanded
    ref, ref_g = _pairs_device(torch, pkg, lib, s1, s2, p1, p2, kind, req, f32)
    exp_summ = pkg.abi.fold_records(ref, scene.n_pairs, _margin(kind, req))
    for chunk in chunks:
        lib.set_option("scene_chunk", chunk)
        for form in forms:
            run = (lambda **kw: _scene_device(torch, pkg, scene, table, kind, req, f32, **kw)) if form == "device" else \
                  (lambda **kw: _scene_host(scene, table, kind, req, f32, **kw))
            what = "%s %s form chunk %d%s" % (kind, form, chunk, " f32" if f32 else "")
            rec, summ, g = run()
            _same(rec, ref, "records differ: " + what)
            if not f32:
                _same(g, ref_g, "guesses differ: " + what)
            _same(summ, exp_summ, "summaries differ from the fold of the records: " + what)
            _, summ_only, _ = run(records=False)
            _same(summ_only, exp_summ, "summary-only call differs: " + what)
    lib.set_option("scene_chunk", 0)
    return ref, exp_summ


# ---- 1. records of solids, byte for byte (+ 3. their folds) ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg5(pkg):
    b = pkg.workloads.cfg5_broadphase_scene()
    sc = b.scene
    i, j = sc["pairs"][:, 0], sc["pairs"][:, 1]
    return dict(b=b, obj_shape=sc["obj_shape"], pairs=sc["pairs"], table=sc["obj_tf"].reshape(1, -1, 12),
                expanded=(sc["obj_shape"][i], sc["obj_shape"][j], sc["obj_tf"][i], sc["obj_tf"][j]))


@pytest.mark.parametrize("kind", ["collide", "distance"])
def test_cfg5_scene_records_and_folds(pkg, torch_cuda, cfg5, kind):
    """cfg5's broadphase scene (100 000 objects, ~1 M pairs, one configuration): the default chunk, a chunk that does not divide the
    pair count, and a chunk below one wave's share of the fold (256 records)."""
    lib = pkg.Library(cfg5["b"].lib)
    scene = lib.scene(cfg5["obj_shape"], cfg5["pairs"])
    try:
        assert scene.n_pairs > 500_000 and scene.n_objects == 100_000
        assert cfg5["expanded"][2].tobytes() == cfg5["b"].tf1.tobytes()  # (the scene's table expands to the batch bench.py times)
        req = _request(pkg, kind)
        ref, summ = _check_scene(torch_cuda, pkg, lib, scene, cfg5["table"], cfg5["expanded"], kind, req, (0, 100_003, 200))
        print("cfg5 scene %s: %d pairs, %d contacts, min %.6g at pair %d" % (kind, scene.n_pairs, summ["n_contacts"][0],
                                                                          summ["min_distance"][0], summ["min_pair"][0]))
        assert summ["n_contacts"][0] == int(pkg.abi.status_contact(ref["status"]).sum()) > 0
        # a second identical call: identical bytes
        a = _scene_device(torch_cuda, pkg, scene, cfg5["table"], kind, req)
        b = _scene_device(torch_cuda, pkg, scene, cfg5["table"], kind, req)
        for x, y in zip(a, b):
            _same(x, y, "a second identical call differs")
    finally:
        scene.close()
        lib.close()


@pytest.mark.parametrize("kind", ["collide", "distance"])
def test_cfg5_scene_f32(pkg, torch_cuda, cfg5, kind):
    b = cfg5["b"]
    sc = b.scene
    # 7-float poses (quaternion w, x, y, z + translation) from the objects' own quaternions / translations: recover them from the batch (object i's pose is any pair's first pose with that i)
    n_obj = len(sc["obj_shape"])
    quat, T = np.zeros((n_obj, 4)), np.zeros((n_obj, 3))
    quat[:, 0] = 1.0
    quat[sc["pairs"][:, 0]], T[sc["pairs"][:, 0]] = b.quat1, b.T1
    quat[sc["pairs"][:, 1]], T[sc["pairs"][:, 1]] = b.quat2, b.T2
    pose = pkg.geometry.pose_f32_from_quat(quat, T)
    i, j = sc["pairs"][:, 0], sc["pairs"][:, 1]
    assert pose[i].tobytes() == b.pose1_f32.tobytes() and pose[j].tobytes() == b.pose2_f32.tobytes()
    lib = pkg.Library(b.lib)
    scene = lib.scene(sc["obj_shape"], sc["pairs"])
    try:
        req = _request(pkg, kind, **({"security_margin": 0.01} if kind == "collide" else {}))
        _check_scene(torch_cuda, pkg, lib, scene, pose.reshape(1, -1, 7), (sc["obj_shape"][i], sc["obj_shape"][j], pose[i], pose[j]),
                     kind, req, (0, 100_003, 200), f32=True)
    finally:
        scene.close()
        lib.close()


@pytest.mark.parametrize("kind,f32", [("collide", False), ("distance", False), ("collide", True), ("distance", True)])
def test_planner_scene_chunks_straddle_configurations(pkg, torch_cuda, kind, f32):
    """scene_planner(2048 configurations, 16 bodies): 105 pairs per configuration; chunks of 50 000 and 1000 queries start and end
    inside configurations, the default chunk holds them all."""
    ps = pkg.workloads.scene_planner(2048, 16)
    e = ps.expand()
    lib = pkg.Library(ps.lib)
    scene = lib.scene(ps.obj_shape, ps.pairs)
    try:
        assert scene.n_pairs == 105
        req = _request(pkg, kind, **({"security_margin": 0.02} if kind == "collide" else {}))
        table = ps.obj_pose_f32 if f32 else ps.obj_tf
        i, j = ps.pairs[:, 0], ps.pairs[:, 1]
        expanded = (e.s1, e.s2, table[:, i].reshape(len(e), -1), table[:, j].reshape(len(e), -1))
        if not f32:
            assert expanded[2].tobytes() == e.tf1.tobytes() and expanded[3].tobytes() == e.tf2.tobytes()
        ref, summ = _check_scene(torch_cuda, pkg, lib, scene, table, expanded, kind, req, (0, 50_000, 1000), f32=f32)
        share = float((summ["n_contacts"] > 0).mean())
        print("scene_planner %s%s: %.1f %% of 2048 configurations collide" % (kind, " f32" if f32 else "", 100 * share))
        assert 0.05 < share < 0.6
    finally:
        scene.close()
        lib.close()


# ---- 2. meshes ------------------------------------------------------------------------------------------------------------------
def test_mesh_scene_one_chunk_and_slices(pkg, torch_cuda):
    """A cfgmix-style scene (solids and the cfg4 meshes, 4000 pairs).  One chunk: byte-equal to the per-pair device call of the same
    n.  Several chunks: byte-equal to per-pair device calls on the same slices (mesh x mesh depths are not promised identical across
    batch sizes; this test does not depend on that)."""
    torch, abi, wl = torch_cuda, pkg.abi, pkg.workloads
    b = wl.mixed_scene(n=64)  # (for its library and meshes)
    rng = np.random.default_rng(17)
    n_lib, n_obj, n_pairs = len(b.lib), 600, 4000
    obj_shape = np.where(rng.random(n_obj) < 0.3, rng.integers(0, 8, n_obj), rng.integers(8, n_lib, n_obj)).astype(np.uint32)
    table = pkg.geometry.make_pose(quat=wl.uniform_quaternions(rng, n_obj), T=rng.uniform(-1.6, 1.6, (n_obj, 3))).reshape(1, n_obj, 12)
    pairs = rng.integers(0, n_obj, (n_pairs, 2)).astype(np.uint32)
    i, j = pairs[:, 0], pairs[:, 1]
    expanded = (obj_shape[i], obj_shape[j], table[0][i], table[0][j])
    lib = wl.make_library(pkg, b)
    scene = lib.scene(obj_shape, pairs)
    try:
        req = abi.default_collision_request()
        ref, _ = _pairs_device(torch, pkg, lib, *expanded, "collide", req)
        kinds = {(int(b.shapes["type"][a]), int(b.shapes["type"][c])) for a, c in zip(expanded[0][:400], expanded[1][:400])}
        assert any(x == abi.BV_OBBRSS and y == abi.BV_OBBRSS for x, y in kinds) and any(x != abi.BV_OBBRSS and y != abi.BV_OBBRSS for x, y in kinds)
        for form in (_scene_device, None):
            rec, summ, _ = form(torch, pkg, scene, table, "collide", req) if form else _scene_host(scene, table, "collide", req)
            _same(rec, ref, "mesh scene, one chunk")
            _same(summ, abi.fold_records(ref, n_pairs, 0.0), "mesh scene, one chunk: fold")
        chunk = 1500
        sliced = np.concatenate([_pairs_device(torch, pkg, lib, *[x[lo:lo + chunk] for x in expanded], "collide", req)[0]
                                 for lo in range(0, n_pairs, chunk)])
        lib.set_option("scene_chunk", chunk)
        for form in (_scene_device, None):
            rec, summ, _ = form(torch, pkg, scene, table, "collide", req) if form else _scene_host(scene, table, "collide", req)
            _same(rec, sliced, "mesh scene, chunks of 1500 against per-pair calls on the same slices")
            _same(summ, abi.fold_records(sliced, n_pairs, 0.0), "mesh scene, chunks: fold")
        print("mesh scene: %d contacts of %d pairs" % (int(abi.status_contact(ref["status"]).sum()), n_pairs))
    finally:
        scene.close()
        lib.close()


# ---- 3. folds: forced ties, all skipped, unsupported pairs -----------------------------------------------------------------------
def _small_scene(pkg, n_obj=40, seed=3):
    L = pkg.ShapeLibrary()
    rng = np.random.default_rng(seed)
    for r in rng.uniform(0.2, 0.6, 5):
        L.add_sphere(float(r))
    for s in rng.uniform(0.2, 0.8, (5, 3)):
        L.add_box(*map(float, s))
    obj_shape = rng.integers(0, 10, n_obj).astype(np.uint32)
    table = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, 3 * n_obj), T=rng.uniform(-1.5, 1.5, (3 * n_obj, 3))).reshape(3, n_obj, 12)
    i, j = np.triu_indices(n_obj, 1)
    return L, obj_shape, table, np.stack([i, j], axis=1).astype(np.uint32)


def test_forced_ties_and_all_skipped(pkg, torch_cuda):
    L, obj_shape, table, pairs = _small_scene(pkg)
    twice = np.repeat(pairs, 2, axis=0)  # every pair appears twice: equal values at neighbouring indices
    lib = pkg.Library(L)
    scene = lib.scene(obj_shape, twice)
    try:
        req = _request(pkg, "collide", security_margin=0.1)
        rec, summ, _ = _scene_device(torch_cuda, pkg, scene, table, "collide", req)
        _same(rec[0::2], rec[1::2], "the two copies of a pair")
        _same(summ, pkg.abi.fold_records(rec, len(twice), 0.1), "forced ties")
        assert np.all(summ["min_pair"] % 2 == 0) and np.all(summ["first_contact"] % 2 == 0) and np.all(summ["n_contacts"] % 2 == 0)
        assert np.all(summ["n_contacts"] > 0)
        for chunk in (1, 77):
            lib.set_option("scene_chunk", chunk)
            _, s2, _ = _scene_host(scene, table, "collide", req, records=False)
            _same(s2, summ, "forced ties, chunk %d" % chunk)
        lib.set_option("scene_chunk", 0)
        # security_margin = -inf: every record skipped (src/collision.cpp:73-76)
        req = _request(pkg, "collide", security_margin=-np.inf)
        for form in ("device", "host"):
            rec, summ, _ = _scene_device(torch_cuda, pkg, scene, table, "collide", req) if form == "device" else \
                _scene_host(scene, table, "collide", req)
            assert np.all(pkg.abi.status_skipped(rec["status"]) == 1), form
            assert np.all(summ["n_skipped"] == len(twice)) and np.all(summ["n_contacts"] == 0), form
            assert np.all(np.isposinf(summ["min_distance"])) and np.all(summ["min_pair"] == NONE) and np.all(summ["first_contact"] == NONE)
            _same(summ, pkg.abi.fold_records(rec, len(twice), -np.inf), "all skipped: " + form)
    finally:
        scene.close()
        lib.close()


def test_unsupported_pair_kind(pkg, torch_cuda):
    """distance() has no TriangleP entries: the batch call returns HFCL_ERR_UNSUPPORTED_PAIR with those records flagged; so does the
    scene's host form, after every chunk has run -- every other record and the summaries are complete."""
    abi = pkg.abi
    L = pkg.ShapeLibrary()
    L.add_sphere(0.5)
    L.add_box(0.4, 0.5, 0.6)
    L.add_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0])
    obj_shape = np.array([0, 1, 2, 0, 1, 2, 0], dtype=np.uint32)
    rng = np.random.default_rng(9)
    table = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, 14), T=rng.uniform(-1, 1, (14, 3))).reshape(2, 7, 12)
    i, j = np.triu_indices(7, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    lib = pkg.Library(L)
    scene = lib.scene(obj_shape, pairs)
    try:
        req = abi.default_distance_request()
        s1, s2 = np.tile(obj_shape[i], 2), np.tile(obj_shape[j], 2)
        tf1, tf2 = table[:, i].reshape(-1, 12), table[:, j].reshape(-1, 12)
        with pytest.raises(pkg.EngineError) as e:
            lib.distance(s1, s2, tf1, tf2, req)
        assert e.value.code == abi.ERR_UNSUPPORTED_PAIR
        ref, _ = _pairs_device(torch_cuda, pkg, lib, s1, s2, tf1, tf2, "distance", req)
        n_tri = int(((obj_shape[i] == 2) | (obj_shape[j] == 2)).sum())
        assert int(abi.status_skipped(ref["status"]).sum()) == 2 * n_tri > 0
        for chunk in (0, 5):
            lib.set_option("scene_chunk", chunk)
            out = np.zeros(2 * len(pairs), dtype=abi.RESULT_DTYPE)
            summ = np.zeros(2, dtype=abi.SCENE_SUMMARY_DTYPE)
            tab = np.ascontiguousarray(table)
            rc = pkg.engine.dll().hfcl_scene_distance(scene._h, abi.ptr(tab), C.c_size_t(2), C.byref(req), abi.ptr(out), abi.ptr(summ), None, None)
            assert rc == abi.ERR_UNSUPPORTED_PAIR, (chunk, rc)
            _same(out, ref, "records beside unsupported pairs, chunk %d" % chunk)
            assert list(summ["n_skipped"]) == [n_tri, n_tri]
            _same(summ, abi.fold_records(ref, len(pairs), None), "summaries beside unsupported pairs")
            rec, s2_, _ = _scene_device(torch_cuda, pkg, scene, table, "distance", req)  # (the device form reads nothing back: no error code)
            _same(rec, ref, "device form")
            _same(s2_, summ, "device form summaries")
    finally:
        scene.close()
        lib.close()


# ---- 4. errors --------------------------------------------------------------------------------------------------------------------
def test_errors_before_any_work(pkg, torch_cuda):
    abi = pkg.abi
    L, obj_shape, table, pairs = _small_scene(pkg, n_obj=10)
    lib = pkg.Library(L)
    d = pkg.engine.dll()
    try:
        bad = pairs.copy()
        bad[3, 1] = 10
        with pytest.raises(pkg.EngineError) as e:
            lib.scene(obj_shape, bad)
        assert e.value.code == abi.ERR_INVALID_ARGUMENT and "outside" in str(e.value)
        ids = obj_shape.copy()
        ids[2] = 10
        with pytest.raises(pkg.EngineError) as e:
            lib.scene(ids, pairs)
        assert "outside the library" in str(e.value)
        scene = lib.scene(obj_shape, pairs)
        with pytest.raises(pkg.EngineError):
            scene.set_pairs(bad)
        assert scene.n_pairs == len(pairs)  # nothing changed
        n = 3 * len(pairs)
        out = np.full(n, 0x5A, dtype=np.uint8).repeat(96).view(abi.RESULT_DTYPE)
        summ = np.full(3, 0x5A, dtype=np.uint8).repeat(24).view(abi.SCENE_SUMMARY_DTYPE)
        before = out.tobytes(), summ.tobytes()
        tab = np.ascontiguousarray(table)
        req = abi.default_collision_request()
        call = lambda r, o, s: d.hfcl_scene_collide(scene._h, abi.ptr(tab), C.c_size_t(3), C.byref(r), abi.ptr(o), abi.ptr(s), None, None)  # noqa: E731
        untouched = lambda: (out.tobytes(), summ.tobytes()) == before  # noqa: E731  (a refused call launches nothing and writes nothing)
        assert call(req, None, None) == abi.ERR_INVALID_ARGUMENT and "both NULL" in pkg.engine.last_error()
        assert untouched()
        assert d.hfcl_scene_collide_device(scene._h, None, C.c_size_t(3), C.byref(req), None, None, None, None, None) == abi.ERR_INVALID_ARGUMENT
        r0 = abi.default_collision_request()
        r0.num_max_contacts = 0
        assert call(r0, out, summ) == abi.ERR_INVALID_ARGUMENT and "max contacts" in pkg.engine.last_error()
        assert untouched()
        r1 = abi.default_collision_request()
        r1.q.epa_max_iterations = 65
        assert call(r1, out, summ) == abi.ERR_LIMIT
        assert untouched()
        counts_before = lib.last_bucket_counts()
        assert sum(counts_before.values()) == 0  # (no batch has run on this library: the refused calls launched none)
        assert call(req, out, summ) == abi.OK  # (the scene works)
        ok_bytes = out.tobytes()
        assert ok_bytes != before[0]
        scene.set_pairs(pairs[:7])  # a new broadphase pass over the same objects
        out7 = np.zeros(3 * 7, dtype=abi.RESULT_DTYPE)
        assert d.hfcl_scene_collide(scene._h, abi.ptr(tab), C.c_size_t(3), C.byref(req), abi.ptr(out7), None, None, None) == abi.OK
        _same(out7.reshape(3, 7), out.reshape(3, -1)[:, :7].copy(), "records after set_pairs")
        # n_conf == 0: nothing written
        assert d.hfcl_scene_collide(scene._h, abi.ptr(tab), C.c_size_t(0), C.byref(req), abi.ptr(out), abi.ptr(summ), None, None) == abi.OK
        assert out.tobytes() == ok_bytes
        # hfcl_lib_set_shapes invalidates the library's scenes
        shapes, verts = np.ascontiguousarray(L.shapes_array()), np.ascontiguousarray(L.vertices_array(), dtype=np.float64)
        assert d.hfcl_lib_set_shapes(lib._h, abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), C.c_size_t(len(verts))) == abi.OK
        out[:] = np.full(n, 0x5A, dtype=np.uint8).repeat(96).view(abi.RESULT_DTYPE)
        summ_ok = summ.tobytes()
        assert call(req, out, summ) == abi.ERR_INVALID_ARGUMENT and "hfcl_lib_set_shapes" in pkg.engine.last_error()
        assert out.tobytes() == before[0] and summ.tobytes() == summ_ok
        scene.close()
        fresh = lib.scene(obj_shape, pairs)  # a new scene works again
        rec = fresh.collide(table, records=True, summary=False)
        assert rec.tobytes() == ok_bytes
        fresh.close()
    finally:
        lib.close()


# ---- 5. front ends ------------------------------------------------------------------------------------------------------------------
def test_compat_collide_scene_equals_collide_pairs(pkg, torch_cuda):
    fcl = pkg.compat
    rng = np.random.default_rng(21)
    geoms = [fcl.Box(0.6, 0.8, 1.0), fcl.Sphere(0.5), fcl.Capsule(0.3, 1.2), fcl.Ellipsoid(0.4, 0.6, 0.8)]
    objs = []
    for k in range(30):
        t = fcl.Transform3f()
        t.setTranslation(rng.uniform(-1.5, 1.5, 3))
        objs.append(fcl.CollisionObject(geoms[k % 4], t))
    i, j = np.triu_indices(30, 1)
    pr = np.stack([i, j], axis=1)
    req = fcl.CollisionRequest()
    req.security_margin = 0.05
    expected = fcl.collide_pairs([(objs[a], objs[b]) for a, b in pr], req)
    got, summ = fcl.collide_scene(objs, pr, req)
    assert len(got) == len(expected) == len(pr)
    n_col = 0
    for g, e in zip(got, expected):
        assert g.numContacts() == e.numContacts() and g.distance_lower_bound == e.distance_lower_bound
        for k in range(g.numContacts()):
            a, b = g.getContact(k), e.getContact(k)
            assert a.o1 is b.o1 and a.o2 is b.o2 and a.penetration_depth == b.penetration_depth
            assert np.array_equal(a.normal, b.normal) and np.array_equal(a.pos, b.pos)
        n_col += g.isCollision()
    assert 0 < n_col < len(pr)
    assert summ["n_contacts"][0] == n_col and summ["min_distance"][0] == min(e.distance_lower_bound for e in expected)
    # two configurations as tables of Transform3f: the objects' own, and the same again
    rows = [[o.getTransform() for o in objs]] * 2
    got2, summ2 = fcl.collide_scene(objs, pr, req, transforms=rows)
    assert len(got2) == 2 and summ2[0].tobytes() == summ2[1].tobytes() == summ[0].tobytes()
    dist, _, dsumm = fcl.distance_scene(objs, pr, fcl.DistanceRequest())
    assert dist.shape == (1, len(pr)) and dsumm["min_distance"][0] == dist.min()


def test_cpp_shim_scene(tmp_path):
    """include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene against amd::collide on the pairs of a CollisionCallBackCollect (g++ build)."""
    exe = str(tmp_path / "test_scene_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_scene", "test_scene_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("same") == 3 and "DIFFERENT" not in r.stdout
