"""Object groups and a group matrix on the device-made pair lists (include/hppfcl_amd_groups.h) on the GPU.  The yardsticks: the numpy model
(tests/groups_model.py: the model of the list without groups, filtered by the header's rule; held against the host broadphase and the
g++ build of the kernels' arithmetic in tests/test_scene_groups_cpu.py) byte for byte, for every group layout of groups_model.layouts;
and, for records and summaries, the culled calls on a second scene that holds the allowed pairs as an explicit list.

The scenes are pairs_model.PairScene (configuration 0 without a touching pair, configuration 1 with every pair touching, the others
1-30 %), so configuration 1 lists exactly the allowed pairs.  Every test makes and closes its own device scenes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import groups_model
import pairs_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
FILL = 0x5A5A5A5A5A5A5A5A
FILL32 = 0x5A5A5A5A
OBJECTS = [5, 63, 64, 65, 130, 257, 600]
CONFS = [3, 37]
NO_PAIRS = np.zeros((0, 2), dtype=np.uint32)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _same(a, b, what):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


@pytest.fixture(scope="module")
def world(pkg, torch_cuda):
    """One library (cfg5's mix) and, per (n_objects, n_conf), the model's scene: made once, shared, not modified.  No device scene."""
    L = pairs_model.mixed_library(pkg)
    lib = pkg.Library(L)
    made = {}

    def get(n_objects, n_conf):
        key = (n_objects, n_conf)
        if key not in made:
            made[key] = pairs_model.PairScene(pkg, L, n_objects, n_conf)
            made[key].check_shares()
        return made[key]

    yield dict(lib=lib, L=L, get=get)
    lib.close()


def _pairs_device(torch, scene, table, inflate, capacity, f32=False):
    dev = torch.device("cuda:0")
    n_conf = table.shape[0]
    d_tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    d_pairs = torch.full((2 * (capacity + 4),), FILL32, dtype=torch.int32, device=dev)  # (four guard entries behind the capacity)
    d_cb = torch.full((n_conf + 1,), FILL, dtype=torch.int64, device=dev)
    d_n = torch.full((1,), FILL, dtype=torch.int64, device=dev)
    scene.self_pairs_device(d_tab, n_conf, inflate, d_pairs, capacity, d_cb, d_n, f32=f32, stream=_stream(torch))
    torch.cuda.synchronize()
    pairs = d_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2)
    return pairs, d_cb.cpu().numpy().view(np.uint64), int(d_n.cpu().numpy()[0])


def _expected(ps, f32, inflate, group, words):
    return groups_model.filter_list(*ps.expected(f32, inflate), group, words)


# ---- 1. the lists ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_conf", CONFS)
@pytest.mark.parametrize("n_objects", OBJECTS)
def test_list_equals_the_model(pkg, torch_cuda, world, n_objects, n_conf):
    """Host form and device form, fp64 and fp32 tables, inflate 0 and 0.25, every layout: the model's bytes, conf_begin and count; the
    guard entries behind the capacity intact."""
    ps = world["get"](n_objects, n_conf)
    scene = world["lib"].scene(ps.obj_shape, NO_PAIRS)
    all_pairs = n_objects * (n_objects - 1) // 2
    try:
        for name, group, words in groups_model.layouts(n_objects):
            groups_model.check_layout(name, group, words)
            scene.set_groups(group, words)
            assert scene.n_groups == len(words)
            allowed = groups_model.n_allowed(group, words)
            for f32 in (False, True):
                table = ps.pose if f32 else ps.tf
                for inflate in (0.0, 0.25):
                    what = "layout %s, %d objects, %d configurations, f32 %d, inflate %g" % (name, n_objects, n_conf, f32, inflate)
                    exp, exp_cb = _expected(ps, f32, inflate, group, words)
                    assert exp_cb[1] == 0 and exp_cb[2] - exp_cb[1] == allowed, what  # (no pair touches; every pair touches)
                    if name == "d":
                        assert allowed == all_pairs and exp.tobytes() == ps.expected(f32, inflate)[0].tobytes()
                    if name == "e":
                        assert len(exp) == 0 and not exp_cb.any()
                    pairs, cb = scene.self_pairs(table, inflate)
                    _same(pairs, exp, "host form pairs: " + what)
                    _same(cb, exp_cb, "host form conf_begin: " + what)
                    got, cb, n = _pairs_device(torch_cuda, scene, table, inflate, len(exp), f32)
                    assert n == len(exp), what
                    _same(np.ascontiguousarray(got[:n]), exp, "device form pairs: " + what)
                    _same(cb, exp_cb, "device form conf_begin: " + what)
                    assert np.all(got[n:] == FILL32), what
    finally:
        scene.close()


@pytest.mark.parametrize("n_objects", [65, 130, 257, 600])
def test_list_does_not_depend_on_the_chunks(pkg, torch_cuda, world, n_objects):
    """Options 0 (the whole call), 1 (a row block a chunk) and 40 (two and a half row blocks: chunks start inside configurations)."""
    lib = world["lib"]
    ps = world["get"](n_objects, 3)
    scene = lib.scene(ps.obj_shape, NO_PAIRS)
    try:
        for name, group, words in groups_model.layouts(n_objects):
            scene.set_groups(group, words)
            for f32, inflate in ((False, 0.0), (True, 0.25)):
                exp, exp_cb = _expected(ps, f32, inflate, group, words)
                for chunk in (0, 1, 40):
                    lib.set_option("scene_cull_chunk", chunk)
                    pairs, cb = scene.self_pairs(ps.pose if f32 else ps.tf, inflate)
                    _same(pairs, exp, "pairs, layout %s chunk %d" % (name, chunk))
                    _same(cb, exp_cb, "conf_begin, layout %s chunk %d" % (name, chunk))
    finally:
        lib.set_option("scene_cull_chunk", 0)
        scene.close()


@pytest.mark.parametrize("n_objects", [5, 63, 64])
def test_both_forms_write_the_same_bytes(pkg, torch_cuda, world, n_objects):
    """Option scene_pairs_small_max 64 (the wave-per-configuration form) and 0 (the tiled form) on the same scenes, whole and in chunks."""
    lib = world["lib"]
    try:
        for n_conf in CONFS:
            ps = world["get"](n_objects, n_conf)
            scene = lib.scene(ps.obj_shape, NO_PAIRS)
            try:
                for name, group, words in groups_model.layouts(n_objects):
                    scene.set_groups(group, words)
                    exp, exp_cb = _expected(ps, False, 0.25, group, words)
                    for small_max, chunk in ((64, 0), (0, 0), (64, 40), (0, 40)):
                        lib.set_option("scene_pairs_small_max", small_max)
                        lib.set_option("scene_cull_chunk", chunk)
                        pairs, cb = scene.self_pairs(ps.tf, 0.25)
                        _same(pairs, exp, "pairs, layout %s small_max %d chunk %d" % (name, small_max, chunk))
                        _same(cb, exp_cb, "conf_begin, layout %s small_max %d chunk %d" % (name, small_max, chunk))
            finally:
                scene.close()
    finally:
        lib.set_option("scene_pairs_small_max", 32)
        lib.set_option("scene_cull_chunk", 0)


def test_count_only_and_short_capacity(pkg, torch_cuda, world):
    ps = world["get"](130, 3)
    scene = world["lib"].scene(ps.obj_shape, NO_PAIRS)
    try:
        group, words = groups_model.random_matrix(130, 8, 0)
        scene.set_groups(group, words)
        exp, exp_cb = _expected(ps, False, 0.0, group, words)
        n_host = C.c_size_t(0)
        tab = np.ascontiguousarray(ps.tf)
        cbh = np.full(4, FILL, dtype=np.uint64)
        fn = pkg.engine.dll().hfcl_scene_self_pairs
        assert fn(scene._h, pkg.abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), None, C.c_size_t(0), pkg.abi.ptr(cbh), C.byref(n_host)) == 0
        assert n_host.value == len(exp) and cbh.tobytes() == exp_cb.tobytes()
        cap = len(exp) // 2
        got, cb, n = _pairs_device(torch_cuda, scene, ps.tf, 0.0, cap)
        assert n == len(exp) and len(got) == cap + 4
        _same(np.ascontiguousarray(got[:cap]), np.ascontiguousarray(exp[:cap]), "pairs below the capacity")
        assert np.all(got[cap:] == FILL32)
        _same(cb, exp_cb, "conf_begin with a short capacity")
    finally:
        scene.close()


# ---- 2. set, replace, refuse, clear ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_objects", [64, 130])
def test_set_clear_and_refusals(pkg, torch_cuda, world, n_objects):
    ps = world["get"](n_objects, 3)
    abi = pkg.abi
    scene = world["lib"].scene(ps.obj_shape, NO_PAIRS)
    try:
        base, base_cb = ps.expected(False, 0.0)
        assert scene.n_groups == 0
        scene.clear_groups()  # (nothing set: fine)
        pairs, cb = scene.self_pairs(ps.tf, 0.0)
        _same(pairs, base, "before any groups")
        group, words = groups_model.between(17, n_objects)
        scene.set_groups(group, groups_model.matrix_of(words))  # (the matrix form)
        exp, exp_cb = groups_model.filter_list(base, base_cb, group, words)
        assert 0 < len(exp) < len(base) and scene.n_groups == 2
        pairs, cb = scene.self_pairs(ps.tf, 0.0)
        _same(pairs, exp, "two managers")
        _same(cb, exp_cb, "two managers: conf_begin")
        # refused calls leave the groups in force
        g8 = np.zeros(n_objects, dtype=np.uint8)
        bad64 = g8.copy()
        bad64[n_objects // 2] = 64
        w64 = np.full(64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        refusals = [
            ("not symmetric", g8, np.array([2, 0], dtype=np.uint64)),
            ("group 64", bad64, w64),
            ("group 2", np.full(n_objects, 2, dtype=np.uint8), np.array([3, 3], dtype=np.uint64)),
            ("bit set at or above", g8, np.array([3, 1 | (1 << 40)], dtype=np.uint64)),
        ]
        for msg, g, w in refusals:
            with pytest.raises(pkg.EngineError) as e:
                scene.set_groups(g, w)
            assert e.value.code == abi.ERR_INVALID_ARGUMENT and msg in str(e.value), (msg, str(e.value))
            assert scene.n_groups == 2
        d = pkg.engine.dll()
        for n_groups in (0, 65):
            assert d.hfcl_scene_set_groups(scene._h, abi.ptr(g8), C.c_size_t(n_groups), abi.ptr(w64)) == abi.ERR_INVALID_ARGUMENT
            assert "groups (1 to 64)" in pkg.engine.last_error()
        assert d.hfcl_scene_set_groups(scene._h, None, C.c_size_t(2), abi.ptr(w64)) == abi.ERR_INVALID_ARGUMENT and "null" in pkg.engine.last_error()
        assert d.hfcl_scene_set_groups(scene._h, abi.ptr(g8), C.c_size_t(2), None) == abi.ERR_INVALID_ARGUMENT and "null" in pkg.engine.last_error()
        pairs, cb = scene.self_pairs(ps.tf, 0.0)
        _same(pairs, exp, "after the refused calls")
        # replaced, then cleared: the unfiltered model's list
        group, words = groups_model.random_matrix(n_objects, 64, 1)
        scene.set_groups(group, words)
        exp, exp_cb = groups_model.filter_list(base, base_cb, group, words)
        pairs, cb = scene.self_pairs(ps.tf, 0.0)
        _same(pairs, exp, "replaced")
        _same(cb, exp_cb, "replaced: conf_begin")
        scene.clear_groups()
        assert scene.n_groups == 0
        pairs, cb = scene.self_pairs(ps.tf, 0.0)
        _same(pairs, base, "cleared")
        _same(cb, base_cb, "cleared: conf_begin")
    finally:
        scene.close()
    # a scene made before hfcl_lib_set_shapes is refused, as in the other scene calls
    L = pairs_model.mixed_library(pkg)
    lib = pkg.Library(L)
    stale = lib.scene(ps.obj_shape, NO_PAIRS)
    try:
        shapes, verts = np.ascontiguousarray(L.shapes_array()), np.ascontiguousarray(L.vertices_array(), dtype=np.float64)
        assert pkg.engine.dll().hfcl_lib_set_shapes(lib._h, abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), C.c_size_t(len(verts))) == abi.OK
        for call in (lambda: stale.set_groups(*groups_model.between(1, n_objects)), stale.clear_groups):
            with pytest.raises(pkg.EngineError) as e:
                call()
            assert e.value.code == abi.ERR_INVALID_ARGUMENT and "hfcl_lib_set_shapes" in str(e.value)
    finally:
        stale.close()
        lib.close()


# ---- 3. records and summaries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obstacles", [122, 40])
def test_records_equal_the_explicit_list(pkg, torch_cuda, n_obstacles):
    """workloads.scene_robot_env: collide_self / distance_self with groups against collide_culled / distance_culled on a second scene
    that holds the allowed pairs as its list.  130 objects: the tiled form; 48: the wave-per-configuration form (option 64)."""
    abi = pkg.abi
    n_conf, n_links = 37, 8
    sc, (group, words), explicit = pkg.workloads.scene_robot_env(n_conf, n_links, n_obstacles)
    lib = pkg.Library(sc.lib, options={"scene_pairs_small_max": 64})
    grouped = lib.scene(sc.obj_shape, NO_PAIRS)
    listed = lib.scene(sc.obj_shape, explicit)
    try:
        grouped.set_groups(group, words)
        for f32 in (False, True):
            table = sc.obj_pose_f32 if f32 else sc.obj_tf
            for kind in ("collide", "distance"):
                what = "%s%s, %d obstacles" % (kind, " f32" if f32 else "", n_obstacles)
                req = abi.default_distance_request() if kind == "distance" else abi.default_collision_request()
                inflate = 0.25 if kind == "distance" else 0.0
                exp_rec, ids, exp_cb, exp_summ = getattr(listed, kind + "_culled")(table, inflate, req)
                p = (ids % np.uint64(len(explicit))).astype(np.int64)
                # neither empty nor the whole explicit list; a configuration with a contact and one without
                assert 0 < len(ids) < n_conf * len(explicit), what
                if kind == "collide":
                    assert (exp_summ["n_contacts"] > 0).any() and (exp_summ["n_contacts"] == 0).any(), what
                rec, pairs, cb, summ = getattr(grouped, kind + "_self")(table, req, inflate)
                _same(pairs, np.ascontiguousarray(explicit[p]), "pairs: " + what)
                _same(cb, exp_cb, "conf_begin: " + what)
                _same(rec, exp_rec, "records: " + what)
                for field in ("min_distance", "n_contacts", "n_skipped"):
                    _same(summ[field], exp_summ[field], field + ": " + what)
                for field in ("min_pair", "first_contact"):  # (a rank in the configuration's list; the culled call names the pair p)
                    rank = summ[field].astype(np.int64)
                    there = summ[field] != NONE
                    assert np.array_equal(there, exp_summ[field] != NONE), field + ": " + what
                    k = cb[:-1].astype(np.int64)[there] + rank[there]
                    assert np.array_equal(p[k], exp_summ[field][there].astype(np.int64)), field + ": " + what
                rec2, pairs2, cb2, summ2 = getattr(grouped, kind + "_self")(table, req, inflate, records=False)
                assert rec2 is None
                _same(summ2, summ, "summaries only: " + what)
    finally:
        grouped.close()
        listed.close()
        lib.close()


# ---- 4. ownership -------------------------------------------------------------------------------------------------------------------------
def test_group_tables_are_given_back(pkg, torch_cuda):
    """The live-handle counts (hfcl_debug_live_handles) are back at their baseline after closing a scene that had groups set, replaced
    and cleared, and one closed with groups still set."""
    def live():
        out = (C.c_int64 * 4)()
        pkg.engine.dll().hfcl_debug_live_handles(out)
        return tuple(int(v) for v in out)

    L = pairs_model.mixed_library(pkg)
    obj_shape = np.arange(70, dtype=np.uint32) % np.uint32(len(L))
    tf = pkg.geometry.make_pose(T=np.random.default_rng(3).uniform(-2, 2, (70, 3))).reshape(1, 70, 12)
    lib = pkg.Library(L)
    try:
        warm = lib.scene(obj_shape, NO_PAIRS)
        warm.self_pairs(tf, 0.0)  # (the library's scene workspace: it stays with the library)
        warm.close()
        base = live()
        for still_set in (False, True):
            scene = lib.scene(obj_shape, NO_PAIRS)
            made = live()
            scene.set_groups(*groups_model.between(17, 70))
            with_groups = live()
            assert sum(with_groups) == sum(made) + 3  # (an object's group, the masks, the tile words)
            scene.self_pairs(tf, 0.0)
            scene.set_groups(*groups_model.random_matrix(70, 64, 0))
            assert live() == with_groups  # (replaced: the old tables are freed)
            scene.self_pairs(tf, 0.0)
            if not still_set:
                scene.clear_groups()
                assert live() == made
            scene.close()
            assert live() == base, ("live handles after close()", live(), "baseline", base)
    finally:
        lib.close()


# ---- 5. front ends ------------------------------------------------------------------------------------------------------------------------
def test_compat_scene_with_groups(pkg, torch_cuda):
    """compat.collide_scene / distance_scene(..., broadphase="self", groups=...): two managers in one scene list what the objects of
    one manager collect against the other (the reference's DynamicAABBTreeCollisionManager::collide(otherManager, callback))."""
    fcl = pkg.compat
    rng = np.random.default_rng(23)
    geoms = [fcl.Box(0.6, 0.8, 1.0), fcl.Sphere(0.5), fcl.Capsule(0.3, 1.2)]
    objs = []
    for k in range(24):
        t = fcl.Transform3f()
        t.setTranslation(rng.uniform(-2.0, 2.0, 3))
        objs.append(fcl.CollisionObject(geoms[k % 3], t))
    n_a = 9
    req = fcl.CollisionRequest()
    got, summ = fcl.collide_scene(objs, None, req, broadphase="self", groups=pkg.engine.groups_between(n_a, 24 - n_a))
    full, _ = fcl.collide_scene(objs, None, req, broadphase="self")
    other = fcl.DynamicAABBTreeCollisionManager()  # (the second manager; every object of the first against it)
    other.registerObjects(objs[n_a:])
    other.setup()
    collect = fcl.CollisionCallBackCollect(10 ** 6)
    for o in objs[:n_a]:
        other.collide(o, collect)
    index = {id(o): k for k, o in enumerate(objs)}
    kept = sorted(tuple(sorted((index[id(x)], index[id(y)]))) for x, y in collect.getCollisionPairs())
    assert 0 < len(kept) < len(full) and [ij for ij, _ in got] == kept
    by_pair = {ij: r for ij, r in full}
    for ij, r in got:
        assert r.numContacts() == by_pair[ij].numContacts() and r.distance_lower_bound == by_pair[ij].distance_lower_bound
    assert summ["n_contacts"][0] == sum(r.isCollision() for _, r in got)
    # an allowed-collision matrix: neighbours in the list of objects excluded
    dist, pairs, dsumm = fcl.distance_scene(objs, None, fcl.DistanceRequest(), broadphase="self", inflate=0.5,
                                            groups=pkg.engine.groups_excluding(24, [(k, k + 1) for k in range(23)]))
    dfull, pfull, _ = fcl.distance_scene(objs, None, fcl.DistanceRequest(), broadphase="self", inflate=0.5)
    keep = pfull[0][:, 1] - pfull[0][:, 0] >= 2
    assert 0 < keep.sum() < len(keep) and np.array_equal(pairs[0], pfull[0][keep]) and np.array_equal(dist[0], dfull[0][keep])
    assert dsumm["min_distance"][0] == dist[0].min()


def test_cpp_shim_groups(tmp_path):
    """include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene::setGroups / clearGroups / numGroups against a list filtered on the host (g++ build)."""
    exe = str(tmp_path / "test_groups_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_groups", "test_groups_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("same") == 3 and "DIFFERENT" not in r.stdout
