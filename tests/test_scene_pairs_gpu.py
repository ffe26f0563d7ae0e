"""The self-collision pairs of a scene per configuration on the GPU (include/hppfcl_amd_pairs.h).  The yardsticks: the numpy model of the list
(tests/pairs_model.py, held against the host broadphase and the g++ build of the header in tests/test_scene_pairs_cpu.py) byte for byte; the
device cull of the all-pairs list; the per-pair calls' records byte for byte; the numpy fold of those records with the rank rule.

The scenes (pairs_model.PairScene): cfg5's shape mix; configuration 0 without a pair, configuration 1 with every pair, the others with 1 % to
30 % of all pairs, asserted on the model's output.  n_conf = 1 is each of the first three configurations of the three-configuration scene on
its own.  The Plane and the BVHModel<OBBRSS> have a scene of their own (test_mesh_and_plane_scene): a Plane that is not aligned with an axis
has an unbounded world box, which touches every box, so no configuration that holds it is without a pair."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cull_model
import pairs_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
FILL = 0x5A5A5A5A5A5A5A5A
FILL32 = 0x5A5A5A5A
OBJECTS = [1, 2, 5, 63, 64, 65, 130, 257, 600]
CONFS = [1, 3, 37]


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _same(a, b, what):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


@pytest.fixture(scope="module")
def world(pkg, torch_cuda):
    """One library (cfg5's mix) and, per (n_objects, n_conf), the model's scene and the device scene -- with an EMPTY pair list of its own,
    which plays no part.  Made once, shared, not modified."""
    L = pairs_model.mixed_library(pkg)
    lib = pkg.Library(L)
    made = {}

    def get(n_objects, n_conf):
        key = (n_objects, max(n_conf, 3))  # (n_conf = 1: the configurations of the three-configuration scene one by one)
        if key not in made:
            ps = pairs_model.PairScene(pkg, L, key[0], key[1])
            ps.check_shares()
            made[key] = (ps, lib.scene(ps.obj_shape, np.zeros((0, 2), dtype=np.uint32)))
        return made[key]

    yield dict(lib=lib, L=L, get=get)
    for _, scene in made.values():
        scene.close()
    lib.close()


def _tables(ps, n_conf, f32):
    """(table, expected pairs, expected conf_begin) of the test's cases: the whole scene, or its first three configurations one by one."""
    table = ps.pose if f32 else ps.tf

    def cases(inflate):
        pairs, cb = ps.expected(f32, inflate)
        if n_conf > 1:
            return [(table, pairs, cb)]
        return [(table[c:c + 1], np.ascontiguousarray(pairs[int(cb[c]):int(cb[c + 1])]), (cb[c:c + 2] - cb[c]).astype(np.uint64)) for c in range(3)]

    return cases


def _pairs_device(torch, scene, table, inflate, capacity, f32=False, count_only=False):
    dev = torch.device("cuda:0")
    n_conf = table.shape[0]
    d_tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    d_pairs = torch.full((2 * (capacity + 4),), FILL32, dtype=torch.int32, device=dev)  # (four guard entries behind the capacity)
    d_cb = torch.full((n_conf + 1,), FILL, dtype=torch.int64, device=dev)
    d_n = torch.full((1,), FILL, dtype=torch.int64, device=dev)
    scene.self_pairs_device(d_tab, n_conf, inflate, None if count_only else d_pairs, capacity, d_cb, d_n, f32=f32, stream=_stream(torch))
    torch.cuda.synchronize()
    pairs = d_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2)
    return pairs, d_cb.cpu().numpy().view(np.uint64), int(d_n.cpu().numpy()[0]), (d_tab, d_pairs, d_cb)


# ---- 1. the list ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_conf", CONFS)
@pytest.mark.parametrize("n_objects", OBJECTS)
def test_list_equals_the_model(pkg, torch_cuda, world, n_objects, n_conf):
    ps, scene = world["get"](n_objects, n_conf)
    for f32 in (False, True):
        cases = _tables(ps, n_conf, f32)
        for inflate in (0.0, 0.25):
            for table, exp, exp_cb in cases(inflate):
                what = "%d objects, %d configurations, f32 %d, inflate %g" % (n_objects, len(table), f32, inflate)
                pairs, cb = scene.self_pairs(table, inflate)
                _same(pairs, exp, "host form pairs: " + what)
                _same(cb, exp_cb, "host form conf_begin: " + what)
                got, cb, n, _ = _pairs_device(torch_cuda, scene, table, inflate, len(exp), f32)
                assert n == len(exp), what
                _same(np.ascontiguousarray(got[:n]), exp, "device form pairs: " + what)
                _same(cb, exp_cb, "device form conf_begin: " + what)
                assert np.all(got[n:] == FILL32), what


@pytest.mark.parametrize("n_objects", [2, 5, 63, 64, 65, 130])
def test_list_equals_the_cull_of_all_pairs(pkg, torch_cuda, world, n_objects):
    """The same list from the route that exists: a scene whose own list is all pairs in triu order, culled on the device, q mapped to (i, j)."""
    ps, scene = world["get"](n_objects, 3)
    i, j = np.triu_indices(n_objects, 1)
    tri = np.stack([i, j], axis=1).astype(np.uint32)
    other = world["lib"].scene(ps.obj_shape, tri)
    try:
        for table in (ps.tf, ps.pose):
            for inflate in (0.0, 0.25):
                ids, cb = other.cull(table, inflate)
                pairs, cb2 = scene.self_pairs(table, inflate)
                _same(pairs, np.ascontiguousarray(tri[(ids % np.uint64(len(tri))).astype(np.int64)]), "pairs")
                _same(cb2, cb, "conf_begin")
    finally:
        other.close()


@pytest.mark.parametrize("n_objects", [65, 130, 257, 600])
def test_list_does_not_depend_on_the_chunks(pkg, torch_cuda, world, n_objects):
    """Chunks of 40 rows are two and a half row blocks of the tiled form: whole blocks, 32 or 48 rows; neither divides these object counts,
    so chunks start in the middle of configurations.  One row block a chunk (option 1), the whole call (0), and 37 configurations."""
    lib = world["lib"]
    try:
        for n_conf in (3, 37) if n_objects == 130 else (3,):
            ps, scene = world["get"](n_objects, n_conf)
            for f32, inflate in ((False, 0.0), (True, 0.25)):
                exp, exp_cb = ps.expected(f32, inflate)
                for chunk in (40, 1, 1000, 0):
                    lib.set_option("scene_cull_chunk", chunk)
                    pairs, cb = scene.self_pairs(ps.pose if f32 else ps.tf, inflate)
                    _same(pairs, exp, "pairs, chunk %d" % chunk)
                    _same(cb, exp_cb, "conf_begin, chunk %d" % chunk)
    finally:
        lib.set_option("scene_cull_chunk", 0)


@pytest.mark.parametrize("n_objects", [2, 5, 63, 64])
def test_both_forms_write_the_same_bytes(pkg, torch_cuda, world, n_objects):
    """Option scene_pairs_small_max: the wave-per-configuration form (the default up to 32 objects, possible up to 64) against the tiled form
    on the same scenes."""
    lib = world["lib"]
    assert lib.set_option("scene_pairs_small_max", 64) is None
    with pytest.raises(pkg.EngineError):
        lib.set_option("scene_pairs_small_max", 65)
    try:
        for n_conf in (3, 37):
            ps, scene = world["get"](n_objects, n_conf)
            exp, exp_cb = ps.expected(False, 0.25)
            for small_max, chunk in ((64, 0), (0, 0), (n_objects, 0), (n_objects - 1, 0), (0, 40), (64, 40)):
                lib.set_option("scene_pairs_small_max", small_max)
                lib.set_option("scene_cull_chunk", chunk)
                pairs, cb = scene.self_pairs(ps.tf, 0.25)
                _same(pairs, exp, "pairs, small_max %d chunk %d" % (small_max, chunk))
                _same(cb, exp_cb, "conf_begin, small_max %d chunk %d" % (small_max, chunk))
    finally:
        lib.set_option("scene_pairs_small_max", 32)
        lib.set_option("scene_cull_chunk", 0)


@pytest.mark.parametrize("n_objects", [5, 64, 257])
def test_count_only_and_short_capacity(pkg, torch_cuda, world, n_objects):
    ps, scene = world["get"](n_objects, 3)
    exp, exp_cb = ps.expected(False, 0.0)
    # count only: no list, the count and conf_begin
    got, cb, n, _ = _pairs_device(torch_cuda, scene, ps.tf, 0.0, 0, count_only=True)
    assert n == len(exp) and np.all(got == FILL32)
    _same(cb, exp_cb, "count-only conf_begin")
    n_host = C.c_size_t(0)
    tab = np.ascontiguousarray(ps.tf)
    fn = pkg.engine.dll().hfcl_scene_self_pairs
    assert fn(scene._h, pkg.abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), None, C.c_size_t(0), None, C.byref(n_host)) == 0 and n_host.value == len(exp)
    # a capacity below the count.  Device form: the count is true, the entries below the capacity are right, the words behind it untouched
    cap = len(exp) // 2
    got, cb, n, _ = _pairs_device(torch_cuda, scene, ps.tf, 0.0, cap)
    assert n == len(exp) and len(got) == cap + 4
    _same(np.ascontiguousarray(got[:cap]), np.ascontiguousarray(exp[:cap]), "pairs below the capacity")
    assert np.all(got[cap:] == FILL32)
    _same(cb, exp_cb, "conf_begin with a short capacity")
    # host form: HFCL_ERR_LIMIT, the count set, the buffers untouched
    pairs = np.full((cap, 2), FILL32, dtype=np.uint32)
    cbh = np.full(4, FILL, dtype=np.uint64)
    rc = fn(scene._h, pkg.abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), pkg.abi.ptr(pairs), C.c_size_t(cap), pkg.abi.ptr(cbh), C.byref(n_host))
    assert rc == pkg.abi.ERR_LIMIT and n_host.value == len(exp) and np.all(pairs == FILL32) and np.all(cbh == FILL)


def test_refusals_and_empty_calls(pkg, torch_cuda, world):
    ps, scene = world["get"](5, 3)
    for bad in (-0.5, np.nan):
        with pytest.raises(pkg.EngineError) as e:
            scene.self_pairs(ps.tf, bad)
        assert e.value.code == pkg.abi.ERR_INVALID_ARGUMENT and "inflate" in str(e.value)
    pairs, cb = scene.self_pairs(ps.tf[:0], 0.0)
    assert len(pairs) == 0 and cb.shape == (1,) and cb[0] == 0
    one, scene1 = world["get"](1, 3)
    pairs, cb = scene1.self_pairs(one.tf, 0.0)
    assert len(pairs) == 0 and cb.shape == (4,) and not cb.any()
    rec, pairs, cb, summ = scene1.collide_self(one.tf)
    assert len(rec) == 0 and len(pairs) == 0 and not cb.any() and np.all(np.isposinf(summ["min_distance"])) and np.all(summ["min_pair"] == NONE)
    # a scene made before hfcl_lib_set_shapes is refused, as in the other scene calls
    L = pairs_model.mixed_library(pkg)
    lib = pkg.Library(L)
    stale = lib.scene(ps.obj_shape, np.zeros((0, 2), dtype=np.uint32))
    try:
        shapes, verts = np.ascontiguousarray(L.shapes_array()), np.ascontiguousarray(L.vertices_array(), dtype=np.float64)
        d, abi = pkg.engine.dll(), pkg.abi
        assert d.hfcl_lib_set_shapes(lib._h, abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), C.c_size_t(len(verts))) == abi.OK
        with pytest.raises(pkg.EngineError) as e:
            stale.self_pairs(ps.tf, 0.0)
        assert e.value.code == pkg.abi.ERR_INVALID_ARGUMENT and "hfcl_lib_set_shapes" in str(e.value)
        with pytest.raises(pkg.EngineError):
            stale.collide_self(ps.tf)
    finally:
        stale.close()
        lib.close()


# ---- 2. records and summaries -------------------------------------------------------------------------------------------------------------
def _on_list_device(torch, pkg, scene, d_tab, n_conf, d_pairs, n, d_cb, kind, req, f32, records=True):
    dev = torch.device("cuda:0")
    d_out = torch.zeros(max(n, 1) * (11 if f32 else 24), dtype=torch.int32, device=dev) if records else None
    d_sum = torch.full((n_conf * 6,), 0x7F7F7F7F, dtype=torch.int32, device=dev)  # (every summary must be written)
    d_g = None
    if f32:
        fn = scene.distance_pairs_device_f32 if kind == "distance" else scene.collide_pairs_device_f32
        fn(d_tab, n_conf, d_pairs, n, d_cb, req, d_out, d_sum, stream=_stream(torch))
    else:
        d_g = torch.zeros(max(n, 1) * 8, dtype=torch.int32, device=dev) if records else None
        fn = scene.distance_pairs_device if kind == "distance" else scene.collide_pairs_device
        fn(d_tab, n_conf, d_pairs, n, d_cb, req, d_out, d_sum, None, d_g, stream=_stream(torch))
    torch.cuda.synchronize()
    rec = d_out.cpu().numpy().view(pkg.abi.RESULT_F32_DTYPE if f32 else pkg.abi.RESULT_DTYPE)[:n] if records else None
    g = d_g.cpu().numpy().view(pkg.abi.GUESS_DTYPE)[:n] if d_g is not None else None
    return rec, d_sum.cpu().numpy().view(pkg.abi.SCENE_SUMMARY_DTYPE), g


def _per_pair(torch, pkg, lib, obj_shape, table, pairs, cb, kind, req, f32):
    """The records of the per-pair arrays expanded on the host: lib.collide / lib.distance (fp64, with the guesses they hand out), the
    device batch entry points of the fp32 path."""
    s1, s2, r1, r2 = pairs_model.expand(obj_shape, table, pairs, cb)
    if not f32:
        return (lib.distance if kind == "distance" else lib.collide)(s1, s2, r1, r2, req, want_guess=True)
    dev = torch.device("cuda:0")
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s1.astype(np.int32), s2.astype(np.int32), r1, r2)]
    d_out = torch.zeros(max(len(s1), 1) * 11, dtype=torch.int32, device=dev)
    (lib.distance_device_f32 if kind == "distance" else lib.collide_device_f32)(d[0], d[1], d[2], d[3], len(s1), req, d_out, stream=_stream(torch))
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(pkg.abi.RESULT_F32_DTYPE)[:len(s1)], None


@pytest.mark.parametrize("kind,f32", [("collide", False), ("distance", False), ("collide", True), ("distance", True)])
@pytest.mark.parametrize("n_objects,n_conf", [(5, 37), (64, 3), (130, 3)])
def test_records_and_summaries(pkg, torch_cuda, world, n_objects, n_conf, kind, f32):
    """Record k of the calls on a list is the per-pair call's record of (shape[i_k], shape[j_k], tf[c][i_k], tf[c][j_k]) byte for byte
    (guesses too in fp64), in one chunk and in chunks that end inside configurations; the summaries are the numpy fold with the rank rule
    (130 objects: the configuration with every pair has 8 385 entries, 33 fold pieces); the host forms equal the device forms, and
    records=False gives the same summaries."""
    abi, lib = pkg.abi, world["lib"]
    ps, scene = world["get"](n_objects, n_conf)
    table = ps.pose if f32 else ps.tf
    req = abi.default_distance_request() if kind == "distance" else abi.default_collision_request()
    margin = None
    if kind == "collide":
        req.security_margin = margin = 0.05
    inflate = 0.25
    exp, exp_cb = ps.expected(f32, inflate)
    exp_rec, exp_g = _per_pair(torch_cuda, pkg, lib, ps.obj_shape, table, exp, exp_cb, kind, req, f32)
    exp_summ = pairs_model.fold_ranked(abi, exp_rec, exp_cb, margin)
    assert np.isposinf(exp_summ["min_distance"][0]) and exp_summ["min_pair"][0] == NONE and exp_summ["min_pair"][1] != NONE
    assert kind == "distance" or exp_summ["n_contacts"][1] > 0
    got, cb, n, (d_tab, d_pairs, d_cb) = _pairs_device(torch_cuda, scene, table, inflate, len(exp), f32)
    assert n == len(exp)
    host = scene.distance_self if kind == "distance" else scene.collide_self
    try:
        for chunk in (0, 50, 7) if n_objects < 100 else (0, 1000, 257):
            lib.set_option("scene_chunk", chunk)
            what = "%s%s chunk %d" % (kind, " f32" if f32 else "", chunk)
            rec, summ, g = _on_list_device(torch_cuda, pkg, scene, d_tab, n_conf, d_pairs, n, d_cb, kind, req, f32)
            _same(rec, exp_rec, "device form records: " + what)
            _same(summ, exp_summ, "device form summaries: " + what)
            if not f32:
                _same(g, exp_g, "device form guesses: " + what)
            _, summ, _ = _on_list_device(torch_cuda, pkg, scene, d_tab, n_conf, d_pairs, n, d_cb, kind, req, f32, records=False)
            _same(summ, exp_summ, "summary-only device form: " + what)
            rec, pairs, cbh, summ = host(table, req, inflate)
            _same(pairs, exp, "host form pairs: " + what)
            _same(cbh, exp_cb, "host form conf_begin: " + what)
            _same(rec, exp_rec, "host form records: " + what)
            _same(summ, exp_summ, "host form summaries: " + what)
            rec, pairs, cbh, summ = host(table, req, inflate, records=False)
            assert rec is None
            _same(pairs, exp, "summary-only host form pairs: " + what)
            _same(summ, exp_summ, "summary-only host form: " + what)
    finally:
        lib.set_option("scene_chunk", 0)
    # the caller reads a summary's pair as pairs[conf_begin[c] + rank]
    c = 1
    k = int(exp_cb[c]) + int(exp_summ["min_pair"][c])
    value = exp_rec["distance"][k] - (exp_rec["distance"].dtype.type(margin) if margin is not None else 0)
    assert float(value) == exp_summ["min_distance"][c]


def test_host_form_capacity(pkg, torch_cuda, world):
    """HFCL_ERR_LIMIT before any narrow-phase work when the outputs are too small; the count is set."""
    ps, scene = world["get"](64, 3)
    exp, _ = ps.expected(False, 0.0)
    abi = pkg.abi
    cap = len(exp) - 1
    out = np.zeros(cap, dtype=abi.RESULT_DTYPE)
    pairs = np.full((cap, 2), FILL32, dtype=np.uint32)
    n = C.c_size_t(0)
    req = abi.default_collision_request()
    tab = np.ascontiguousarray(ps.tf)
    rc = pkg.engine.dll().hfcl_scene_collide_self(scene._h, abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), C.byref(req), abi.ptr(out), C.c_size_t(cap),
                                                  abi.ptr(pairs), None, None, None, None, C.byref(n))
    assert rc == abi.ERR_LIMIT and n.value == len(exp) and np.all(pairs == FILL32) and not out["status"].any()


# ---- 3. a mesh and a Plane -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obj", [40, 70])
def test_mesh_and_plane_scene(pkg, torch_cuda, n_obj):
    """cfg5's mix plus one Plane not aligned with an axis and one BVHModel<OBBRSS>: the list is the model's on the device's own boxes (a
    mesh has no host box function), every pair of the Plane is listed in every configuration, and the records are the device batch's.
    40 objects: the wave-per-configuration form (and the tiled one, by the option) meets the unbounded box; 70: the tiled form alone."""
    wl, abi = pkg.workloads, pkg.abi
    torch = torch_cuda
    mesh = wl.mesh_variants(1, 12, 10)[0]
    L = pairs_model.mixed_library(pkg)
    plane = len(L)
    L.add_plane([1, 2, -1], 0.5)
    bvh = len(L)
    L.add_bvh(0, len(mesh.vertices))
    rng = np.random.default_rng(9)
    n_conf, i_mesh = 3, n_obj - 4
    obj_shape = rng.integers(0, plane, n_obj).astype(np.uint32)
    obj_shape[17], obj_shape[i_mesh] = plane, bvh
    half = 3.5 if n_obj == 70 else 2.9
    tf = pkg.geometry.make_pose(quat=wl.uniform_quaternions(rng, n_conf * n_obj), T=rng.uniform(-half, half, (n_conf * n_obj, 3))).reshape(n_conf, n_obj, 12)
    tf[1, :, :9] = pkg.geometry.make_pose()[:9]  # a configuration of identity rotations
    lib = pkg.Library(L)
    lib.add_bvh(mesh)
    scene = lib.scene(obj_shape, np.zeros((0, 2), dtype=np.uint32))
    try:
        boxes = scene.world_aabbs(tf)
        exp, exp_cb = pairs_model.self_pairs(boxes, 0.0)
        all_pairs = n_obj * (n_obj - 1) // 2
        counts = np.diff(exp_cb.astype(np.int64))
        assert np.all(counts >= n_obj - 1) and np.all(counts <= 0.3 * all_pairs)
        for c in range(n_conf):
            mine = exp[int(exp_cb[c]):int(exp_cb[c + 1])]
            assert ((mine == 17).any(axis=1)).sum() == n_obj - 1, c
        assert (exp == i_mesh).any()
        for small_max, chunk in ((64, 0), (0, 0), (64, 40), (0, 40)):
            lib.set_option("scene_pairs_small_max", small_max)
            lib.set_option("scene_cull_chunk", chunk)
            pairs, cb = scene.self_pairs(tf, 0.0)
            _same(pairs, exp, "pairs, small_max %d chunk %d" % (small_max, chunk))
            _same(cb, exp_cb, "conf_begin, small_max %d chunk %d" % (small_max, chunk))
        lib.set_option("scene_cull_chunk", 0)
        lib.set_option("scene_pairs_small_max", 64)  # (40 objects: the records below come from the list of the wave-per-configuration form)
        req = abi.default_collision_request()
        s1, s2, r1, r2 = pairs_model.expand(obj_shape, tf, exp, exp_cb)
        dev = torch.device("cuda:0")
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s1.astype(np.int32), s2.astype(np.int32), r1, r2)]
        d_out = torch.zeros(len(s1) * 24, dtype=torch.int32, device=dev)
        d_g = torch.zeros(len(s1) * 8, dtype=torch.int32, device=dev)
        lib.collide_device(d[0], d[1], d[2], d[3], len(s1), req, d_out, None, d_g, stream=_stream(torch))
        torch.cuda.synchronize()
        exp_rec, exp_g = d_out.cpu().numpy().view(abi.RESULT_DTYPE), d_g.cpu().numpy().view(abi.GUESS_DTYPE)
        got, cb, n, (d_tab, d_pairs, d_cb) = _pairs_device(torch, scene, tf, 0.0, len(exp))
        for chunk in (0, 11):
            lib.set_option("scene_chunk", chunk)
            rec, summ, g = _on_list_device(torch, pkg, scene, d_tab, n_conf, d_pairs, n, d_cb, "collide", req, False)
            _same(rec, exp_rec, "records, chunk %d" % chunk)
            _same(g, exp_g, "guesses, chunk %d" % chunk)
            _same(summ, pairs_model.fold_ranked(abi, exp_rec, exp_cb, 0.0), "summaries, chunk %d" % chunk)
    finally:
        lib.set_option("scene_chunk", 0)
        lib.set_option("scene_cull_chunk", 0)
        scene.close()
        lib.close()


# ---- 4. front ends ---------------------------------------------------------------------------------------------------------------------
def test_compat_scene_with_self_broadphase(pkg, torch_cuda):
    """compat.collide_scene / distance_scene(..., broadphase="self"): no list; per configuration ((i, j), result) of the pairs whose boxes
    overlap -- the pairs the manager collects, in (i, j) order --, the results those of collide_pairs, the summaries' pairs ranks in that list.
    A Plane among the objects: its box is unbounded, so it meets every object, in front of it and behind it in the list."""
    fcl = pkg.compat
    rng = np.random.default_rng(22)
    geoms = [fcl.Box(0.6, 0.8, 1.0), fcl.Sphere(0.5), fcl.Capsule(0.3, 1.2)]
    objs = []
    for k in range(24):
        t = fcl.Transform3f()
        t.setTranslation(rng.uniform(-2.5, 2.5, 3))
        objs.append(fcl.CollisionObject(geoms[k % 3], t))
    dist, pairs, dsumm = fcl.distance_scene(objs, None, fcl.DistanceRequest(), broadphase="self", inflate=0.5)
    i, j = np.triu_indices(24, 1)
    full, _, _ = fcl.distance_scene(objs, np.stack([i, j], axis=1), fcl.DistanceRequest())
    assert len(dist) == 1 and 0 < len(dist[0]) == len(pairs[0]) < 276 and dsumm["min_distance"][0] == dist[0].min()
    where = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(i, j))}
    assert np.array_equal(dist[0], full[0][[where[tuple(p)] for p in pairs[0].tolist()]])
    objs[5] = fcl.CollisionObject(fcl.Plane(np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0), 0.5), fcl.Transform3f())  # (an unbounded box)
    req = fcl.CollisionRequest()
    got, summ = fcl.collide_scene(objs, None, req, broadphase="self")
    mgr, collect = fcl.DynamicAABBTreeCollisionManager(), fcl.CollisionCallBackCollect(10 ** 6)
    mgr.registerObjects(objs)
    mgr.setup()
    mgr.collide(collect)
    index = {id(o): k for k, o in enumerate(objs)}
    kept = sorted(tuple(sorted((index[id(a)], index[id(b)]))) for a, b in collect.getCollisionPairs())
    assert 23 <= len(kept) < 276 and [ij for ij, _ in got] == kept
    expected = fcl.collide_pairs([(objs[i], objs[j]) for i, j in kept], req)
    n_col, first = 0, None
    for rank, ((ij, g), e) in enumerate(zip(got, expected)):
        assert g.numContacts() == e.numContacts() and g.distance_lower_bound == e.distance_lower_bound
        for c in range(g.numContacts()):
            a, b = g.getContact(c), e.getContact(c)
            assert a.o1 is b.o1 and a.o2 is b.o2 and a.penetration_depth == b.penetration_depth and np.array_equal(a.pos, b.pos)
        if g.isCollision():
            n_col += 1
            first = rank if first is None else first
    assert n_col > 0 and summ["n_contacts"][0] == n_col and summ["first_contact"][0] == first  # (a rank in the configuration's list)
    # several configurations as an array of tables; distance
    table = np.stack([np.concatenate([o.getTransform()._abi().reshape(1, 12) for o in objs])] * 2)
    table[1, :, 9] += np.arange(24) * 50.0  # spread out: only the Plane's pairs are left
    got2, summ2 = fcl.collide_scene(objs, None, req, transforms=table, broadphase="self")
    assert [ij for ij, _ in got2[0]] == kept and sorted(ij for ij, _ in got2[1]) == sorted((min(5, k), max(5, k)) for k in range(24) if k != 5)
    with pytest.raises(ValueError):
        fcl.collide_scene(objs[:4], None, req, broadphase="tree")


def test_cpp_shim_self_pairs(tmp_path):
    """include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene::selfPairs / collideSelf / distanceSelf against the culled all-pairs Scene (g++ build)."""
    exe = str(tmp_path / "test_pairs_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_pairs", "test_pairs_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("same") == 3 and "DIFFERENT" not in r.stdout
