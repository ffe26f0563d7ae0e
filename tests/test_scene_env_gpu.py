"""A static environment kept on the device (include/hppfcl_amd_env.h) on the GPU.  The yardsticks: the numpy model of the env list
(tests/env_model.py, held against the g++ build of the header in tests/test_scene_env_cpu.py) byte for byte; the existing device path --
hfcl_scene_self_pairs* and hfcl_scene_*_pairs_device* on the FULL table, the moving rows of a configuration followed by the environment's
--; the per-pair batch calls' records byte for byte; the numpy fold with the rank rule.

The scenes (env_model.EnvScene): cfg5's shape mix, the environment in slabs along x so that its tiles are compact; configuration 0 lists
nothing, the others between 1 % and 30 % of the allowed pairs, every environment tile is met, cells are skipped by their box -- asserted on
the model's output.  n_conf = 1 is each of the three configurations of the three-configuration scene on its own."""
import ctypes as C

import numpy as np
import pytest

import env_model
import pairs_model
from test_scene_pairs_gpu import FILL, FILL32, NONE, _on_list_device, _per_pair, _same, _stream

pytestmark = pytest.mark.gpu
SIZES, CONFS = env_model.SIZES, env_model.CONFS


@pytest.fixture(scope="module")
def world(pkg, torch_cuda):
    """One library (cfg5's mix) and, per (n_moving, n_env, n_conf), the model's scene and the device scene of all its objects -- with an
    EMPTY pair list of its own, which plays no part.  Made once, shared; the environment is set by the test that needs it."""
    L = pairs_model.mixed_library(pkg)
    lib = pkg.Library(L)
    made = {}

    def get(n_moving, n_env, n_conf):
        key = (n_moving, n_env, max(n_conf, 3))
        if key not in made:
            es = env_model.EnvScene(pkg, L, *key)
            es.check()
            made[key] = (es, lib.scene(es.obj_shape, np.zeros((0, 2), dtype=np.uint32)))
        return made[key]

    yield dict(lib=lib, L=L, get=get)
    for _, scene in made.values():
        scene.close()
    lib.close()


def _set_env(scene, es, f32):
    scene.set_environment(es.n_moving, es.env_pose if f32 else es.env_tf)
    assert scene.n_moving == es.n_moving


def _cases(es, n_conf, f32, inflate, groups=None):
    """[(moving table, full table, expected pairs, expected conf_begin)]: the whole scene, or its three configurations one by one."""
    moving, full = (es.moving_pose, es.pose) if f32 else (es.moving_tf, es.tf)
    pairs, cb = es.expected(f32, inflate, groups)
    if n_conf > 1:
        return [(moving, full, pairs, cb)]
    return [(moving[c:c + 1], full[c:c + 1], np.ascontiguousarray(pairs[int(cb[c]):int(cb[c + 1])]), (cb[c:c + 2] - cb[c]).astype(np.uint64))
            for c in range(3)]


def _env_device(torch, scene, moving, inflate, capacity, f32=False, count_only=False):
    dev = torch.device("cuda:0")
    n_conf = moving.shape[0]
    d_tab = torch.from_numpy(np.ascontiguousarray(moving)).to(dev)
    d_pairs = torch.full((2 * (capacity + 4),), FILL32, dtype=torch.int32, device=dev)  # (four guard entries behind the capacity)
    d_cb = torch.full((n_conf + 1,), FILL, dtype=torch.int64, device=dev)
    d_n = torch.full((1,), FILL, dtype=torch.int64, device=dev)
    scene.env_pairs_device(d_tab, n_conf, inflate, None if count_only else d_pairs, capacity, d_cb, d_n, f32=f32, stream=_stream(torch))
    torch.cuda.synchronize()
    pairs = d_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2)
    return pairs, d_cb.cpu().numpy().view(np.uint64), int(d_n.cpu().numpy()[0]), (d_tab, d_pairs, d_cb)


# ---- 1. the list ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_conf", CONFS)
@pytest.mark.parametrize("n_moving,n_env", SIZES)
def test_list_equals_the_model_and_the_filtered_self_pairs(pkg, torch_cuda, world, n_moving, n_env, n_conf):
    es, scene = world["get"](n_moving, n_env, n_conf)
    for f32 in (False, True):
        _set_env(scene, es, f32)
        for inflate in (0.0, 0.25):
            for moving, full, exp, exp_cb in _cases(es, n_conf, f32, inflate):
                what = "%d + %d objects, %d configurations, f32 %d, inflate %g" % (n_moving, n_env, len(moving), f32, inflate)
                pairs, cb = scene.env_pairs(moving, inflate)
                _same(pairs, exp, "host form pairs: " + what)
                _same(cb, exp_cb, "host form conf_begin: " + what)
                # the existing GPU path as a second yardstick: the list of the full table, less the entries with i >= n_moving
                theirs, their_cb = env_model.filter_moving(*scene.self_pairs(full, inflate), n_moving)
                _same(pairs, theirs, "self_pairs filtered: " + what)
                _same(cb, their_cb, "self_pairs filtered conf_begin: " + what)
                got, cb, n, _ = _env_device(torch_cuda, scene, moving, inflate, len(exp), f32)
                assert n == len(exp), what
                _same(np.ascontiguousarray(got[:n]), exp, "device form pairs: " + what)
                _same(cb, exp_cb, "device form conf_begin: " + what)
                assert np.all(got[n:] == FILL32), what


@pytest.mark.parametrize("n_moving,n_env", [(5, 255), (17, 257), (64, 600)])
def test_count_only_and_short_capacity(pkg, torch_cuda, world, n_moving, n_env):
    es, scene = world["get"](n_moving, n_env, 3)
    _set_env(scene, es, False)
    exp, exp_cb = es.expected(False, 0.0)
    got, cb, n, _ = _env_device(torch_cuda, scene, es.moving_tf, 0.0, 0, count_only=True)
    assert n == len(exp) and np.all(got == FILL32)
    _same(cb, exp_cb, "count-only conf_begin")
    n_host = C.c_size_t(0)
    tab = np.ascontiguousarray(es.moving_tf)
    fn = pkg.engine.dll().hfcl_scene_env_pairs
    assert fn(scene._h, pkg.abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), None, C.c_size_t(0), None, C.byref(n_host)) == 0 and n_host.value == len(exp)
    # a capacity one short.  Device form: the true count, the entries below the capacity, nothing at or past it
    cap = len(exp) - 1
    got, cb, n, _ = _env_device(torch_cuda, scene, es.moving_tf, 0.0, cap)
    assert n == len(exp) and len(got) == cap + 4
    _same(np.ascontiguousarray(got[:cap]), np.ascontiguousarray(exp[:cap]), "pairs below the capacity")
    assert np.all(got[cap:] == FILL32)
    _same(cb, exp_cb, "conf_begin with a short capacity")
    # host form: HFCL_ERR_LIMIT, the count set, the buffers untouched
    pairs = np.full((cap, 2), FILL32, dtype=np.uint32)
    cbh = np.full(4, FILL, dtype=np.uint64)
    rc = fn(scene._h, pkg.abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), pkg.abi.ptr(pairs), C.c_size_t(cap), pkg.abi.ptr(cbh), C.byref(n_host))
    assert rc == pkg.abi.ERR_LIMIT and n_host.value == len(exp) and np.all(pairs == FILL32) and np.all(cbh == FILL)
    # the host forms of the narrow phase refuse the same before any narrow-phase work
    abi = pkg.abi
    out = np.zeros(cap, dtype=abi.RESULT_DTYPE)
    req = abi.default_collision_request()
    rc = pkg.engine.dll().hfcl_scene_collide_env(scene._h, abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), C.byref(req), abi.ptr(out), C.c_size_t(cap),
                                                 abi.ptr(pairs), None, None, None, None, C.byref(n_host))
    assert rc == abi.ERR_LIMIT and n_host.value == len(exp) and np.all(pairs == FILL32) and not out["status"].any()


# ---- 2. cutting the call ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_moving,n_env", [(17, 257), (65, 600), (130, 513)])
def test_list_does_not_depend_on_chunks_and_spans(pkg, torch_cuda, world, n_moving, n_env):
    """scene_cull_chunk 7 is one row block a chunk (whole blocks: 16 rows), 64 four -- neither divides 17, 65 or 130 rows, so chunks start
    inside configurations --, 0 the whole call; scene_env_span 1 and 2 tiles a cell, 0 the automatic length."""
    lib = world["lib"]
    try:
        for n_conf in (3, 37) if n_moving == 130 else (3,):
            es, scene = world["get"](n_moving, n_env, n_conf)
            for f32, inflate in ((False, 0.0), (True, 0.25)):
                _set_env(scene, es, f32)
                exp, exp_cb = es.expected(f32, inflate)
                for chunk in (7, 64, 0):
                    for span in (1, 2, 0):
                        lib.set_option("scene_cull_chunk", chunk)
                        lib.set_option("scene_env_span", span)
                        pairs, cb = scene.env_pairs(es.moving_pose if f32 else es.moving_tf, inflate)
                        _same(pairs, exp, "pairs, chunk %d span %d" % (chunk, span))
                        _same(cb, exp_cb, "conf_begin, chunk %d span %d" % (chunk, span))
    finally:
        lib.set_option("scene_cull_chunk", 0)
        lib.set_option("scene_env_span", 0)


# ---- 3. groups --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_moving,n_env", [(5, 255), (17, 257), (63, 600)])
def test_groups(pkg, torch_cuda, world, n_moving, n_env):
    """scene_robot_env's groups (neighbours excluded, the obstacles one group): the filtered groups_model list; a matrix of all ones equals no
    groups.  The groups set before the environment and after it."""
    lib = world["lib"]
    es, scene = world["get"](n_moving, n_env, 3)
    robot = ("robot",) + env_model.robot_groups(n_moving, es.n)
    ones = ("ones", np.random.default_rng(1).integers(0, 8, es.n).astype(np.uint8), np.full(8, 0xFF, dtype=np.uint64))
    try:
        for order in ("groups first", "environment first"):
            for groups in (robot, ones):
                scene.clear_environment()
                scene.clear_groups()
                if order == "groups first":
                    scene.set_groups(groups[1], groups[2])
                _set_env(scene, es, False)
                if order != "groups first":
                    scene.set_groups(groups[1], groups[2])
                for inflate in (0.0, 0.25):
                    exp, exp_cb = es.expected(False, inflate, groups)
                    if groups is ones:
                        _same(exp, es.expected(False, inflate)[0], "a matrix of all ones is no groups")
                    for span in (1, 0):
                        lib.set_option("scene_env_span", span)
                        pairs, cb = scene.env_pairs(es.moving_tf, inflate)
                        _same(pairs, exp, "%s, %s, inflate %g, span %d" % (groups[0], order, inflate, span))
                        _same(cb, exp_cb, "conf_begin")
                    theirs, their_cb = env_model.filter_moving(*scene.self_pairs(es.tf, inflate), n_moving)
                    _same(theirs, exp, "self_pairs with groups, filtered")
        scene.clear_groups()  # the tables of the groups are gone: the list without them
        _same(scene.env_pairs(es.moving_tf, 0.0)[0], es.expected(False, 0.0)[0], "after clear_groups")
    finally:
        lib.set_option("scene_env_span", 0)
        scene.clear_groups()


# ---- 4. the tile rule on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_moving,n_env", [(1, 1), (5, 255), (16, 256), (17, 257), (65, 600), (130, 513)])
def test_environment_boxes_and_tile_boxes(pkg, torch_cuda, world, n_moving, n_env):
    es, scene = world["get"](n_moving, n_env, 3)
    for f32 in (False, True):
        _set_env(scene, es, f32)
        boxes, tiles = scene.environment_aabbs()
        theirs = scene.world_aabbs(es.pose if f32 else es.tf)
        _same(boxes, np.ascontiguousarray(theirs[0, n_moving:]), "environment boxes = world_aabbs of the full table's environment rows")
        _same(boxes, np.ascontiguousarray((es.boxes32 if f32 else es.boxes)[0, n_moving:]), "... = the host's")
        _same(tiles, env_model.tile_boxes(boxes), "tile boxes")
        assert tiles.shape == ((n_env + 255) // 256, 6)


def test_nan_poses(pkg, torch_cuda, world):
    """A NaN environment pose and a NaN moving pose: the tile that holds the NaN box gets an infinite coordinate where the NaN is -- that
    coordinate no longer skips it --, and the lists equal the model on the device's own boxes (the rule's comparisons are false on a NaN:
    configuration 0, far below everything in z, now lists the pairs of the object whose z is NaN)."""
    es, scene = world["get"](17, 257, 3)
    try:
        for f32 in (False, True):
            env = (es.env_pose if f32 else es.env_tf).copy()
            moving = (es.moving_pose if f32 else es.moving_tf).copy()
            env[100, -1] = np.nan      # z of the translation
            env[256, -3] = np.nan      # the tile of one member: x
            moving[1, 16, -2] = np.nan
            moving[0, 3, -1] = np.nan  # (the configuration that lists nothing else)
            scene.set_environment(17, env)
            full = env_model.full_table(moving, env)
            boxes = scene.world_aabbs(full)
            assert np.isnan(boxes[0, 17 + 100]).any() and np.isnan(boxes[1, 16]).any()
            got_boxes, tiles = scene.environment_aabbs()
            _same(got_boxes, np.ascontiguousarray(boxes[0, 17:]), "environment boxes")
            _same(tiles, env_model.tile_boxes(got_boxes), "tile boxes")
            assert np.isinf(tiles[0]).any() and np.isinf(tiles[1]).any() and not np.isnan(tiles).any()
            for inflate in (0.0, 0.25):
                exp, exp_cb = env_model.env_pairs(boxes, 17, inflate)
                first = exp[:int(exp_cb[1])]
                assert len(first) > 0 and np.all((first == 3).any(axis=1) | (first[:, 1] == 17 + 100))  # (only the NaN boxes' pairs)
                pairs, cb = scene.env_pairs(moving, inflate)
                _same(pairs, exp, "pairs, f32 %d inflate %g" % (f32, inflate))
                _same(cb, exp_cb, "conf_begin")
    finally:
        _set_env(scene, es, False)


# ---- 5. the narrow phase -------------------------------------------------------------------------------------------------------------------
def _on_env_list_device(torch, pkg, scene, d_tab, n_conf, d_pairs, n, d_cb, kind, req, f32, records=True, d_gin=None):
    dev = torch.device("cuda:0")
    d_out = torch.zeros(max(n, 1) * (11 if f32 else 24), dtype=torch.int32, device=dev) if records else None
    d_sum = torch.full((n_conf * 6,), 0x7F7F7F7F, dtype=torch.int32, device=dev)  # (every summary must be written)
    d_g = None
    if f32:
        fn = scene.distance_env_pairs_device_f32 if kind == "distance" else scene.collide_env_pairs_device_f32
        fn(d_tab, n_conf, d_pairs, n, d_cb, req, d_out, d_sum, stream=_stream(torch))
    else:
        d_g = torch.zeros(max(n, 1) * 8, dtype=torch.int32, device=dev) if records else None
        fn = scene.distance_env_pairs_device if kind == "distance" else scene.collide_env_pairs_device
        fn(d_tab, n_conf, d_pairs, n, d_cb, req, d_out, d_sum, d_gin, d_g, stream=_stream(torch))
    torch.cuda.synchronize()
    rec = d_out.cpu().numpy().view(pkg.abi.RESULT_F32_DTYPE if f32 else pkg.abi.RESULT_DTYPE)[:n] if records else None
    g = d_g.cpu().numpy().view(pkg.abi.GUESS_DTYPE)[:n] if d_g is not None else None
    return rec, d_sum.cpu().numpy().view(pkg.abi.SCENE_SUMMARY_DTYPE), g


@pytest.mark.parametrize("kind,f32", [("collide", False), ("distance", False), ("collide", True), ("distance", True)])
@pytest.mark.parametrize("n_moving,n_env,n_conf", [(5, 255, 37), (64, 600, 3), (130, 513, 3)])
def test_records_and_summaries(pkg, torch_cuda, world, n_moving, n_env, n_conf, kind, f32):
    """Records, guesses in and out and summaries of the calls on an env list are byte for byte those of hfcl_scene_*_pairs_device* on the
    full table with the same list, and the per-pair batch calls'; the summaries are the numpy fold with the rank rule; the host forms
    (records, pairs, conf_begin, summaries; summaries only) equal the device route.  In one chunk and in chunks that end inside
    configurations."""
    torch, abi, lib = torch_cuda, pkg.abi, world["lib"]
    es, scene = world["get"](n_moving, n_env, n_conf)
    _set_env(scene, es, f32)
    moving, full = (es.moving_pose, es.pose) if f32 else (es.moving_tf, es.tf)
    req = abi.default_distance_request() if kind == "distance" else abi.default_collision_request()
    margin = None
    if kind == "collide":
        req.security_margin = margin = 0.05
    inflate = 0.25
    exp, exp_cb = es.expected(f32, inflate)
    exp_rec, exp_g = _per_pair(torch, pkg, lib, es.obj_shape, full, exp, exp_cb, kind, req, f32)
    exp_summ = pairs_model.fold_ranked(abi, exp_rec, exp_cb, margin)
    assert np.isposinf(exp_summ["min_distance"][0]) and exp_summ["min_pair"][0] == NONE and exp_summ["min_pair"][1] != NONE
    got, cb, n, (d_tab, d_pairs, d_cb) = _env_device(torch, scene, moving, inflate, len(exp), f32)
    assert n == len(exp)
    _same(np.ascontiguousarray(got[:n]), exp, "the list")
    d_full = torch.from_numpy(np.ascontiguousarray(full)).to(torch.device("cuda:0"))
    host = scene.distance_env if kind == "distance" else scene.collide_env
    try:
        for chunk in (0, 50, 7) if n_moving < 100 else (0, 1000, 257):
            lib.set_option("scene_chunk", chunk)
            what = "%s%s chunk %d" % (kind, " f32" if f32 else "", chunk)
            rec, summ, g = _on_env_list_device(torch, pkg, scene, d_tab, n_conf, d_pairs, n, d_cb, kind, req, f32)
            theirs, their_summ, their_g = _on_list_device(torch, pkg, scene, d_full, n_conf, d_pairs, n, d_cb, kind, req, f32)
            _same(rec, theirs, "records = the pairs call's on the full table: " + what)
            _same(summ, their_summ, "summaries = the pairs call's: " + what)
            _same(rec, exp_rec, "records = the per-pair calls': " + what)
            _same(summ, exp_summ, "summaries = the fold: " + what)
            if not f32:
                _same(g, their_g, "guesses out = the pairs call's: " + what)
                _same(g, exp_g, "guesses out = the per-pair calls': " + what)
            _, summ, _ = _on_env_list_device(torch, pkg, scene, d_tab, n_conf, d_pairs, n, d_cb, kind, req, f32, records=False)
            _same(summ, exp_summ, "summary-only device form: " + what)
            rec, pairs, cbh, summ = host(moving, req, inflate)
            _same(pairs, exp, "host form pairs: " + what)
            _same(cbh, exp_cb, "host form conf_begin: " + what)
            _same(rec, exp_rec, "host form records: " + what)
            _same(summ, exp_summ, "host form summaries: " + what)
            rec, pairs, cbh, summ = host(moving, req, inflate, records=False)
            assert rec is None
            _same(pairs, exp, "summary-only host form pairs: " + what)
            _same(summ, exp_summ, "summary-only host form: " + what)
        if not f32:  # guesses in: the ones the first call handed out, into both routes
            lib.set_option("scene_chunk", 50)
            d_gin = torch.from_numpy(np.ascontiguousarray(exp_g).view(np.int32).reshape(-1)).to(torch.device("cuda:0"))
            rec, summ, g = _on_env_list_device(torch, pkg, scene, d_tab, n_conf, d_pairs, n, d_cb, kind, req, f32, d_gin=d_gin)
            d_out = torch.zeros(max(n, 1) * 24, dtype=torch.int32, device=torch.device("cuda:0"))
            d_g = torch.zeros(max(n, 1) * 8, dtype=torch.int32, device=torch.device("cuda:0"))
            d_sum = torch.zeros(n_conf * 6, dtype=torch.int32, device=torch.device("cuda:0"))
            (scene.distance_pairs_device if kind == "distance" else scene.collide_pairs_device)(d_full, n_conf, d_pairs, n, d_cb, req, d_out, d_sum, d_gin,
                                                                                                 d_g, stream=_stream(torch))
            torch.cuda.synchronize()
            _same(rec, d_out.cpu().numpy().view(abi.RESULT_DTYPE)[:n], "records with guesses in")
            _same(g, d_g.cpu().numpy().view(abi.GUESS_DTYPE)[:n], "guesses out with guesses in")
            _same(summ, d_sum.cpu().numpy().view(abi.SCENE_SUMMARY_DTYPE), "summaries with guesses in")
    finally:
        lib.set_option("scene_chunk", 0)


def test_mesh_and_plane_in_the_environment(pkg, torch_cuda):
    """cfg5's mix moving among an environment that holds a BVHModel<OBBRSS> and a Plane not aligned with an axis (an unbounded world box:
    every moving object pairs with it, and no tile that holds it is ever skipped).  The list is the model's on the device's own boxes (a
    mesh has no host box function); the records are those of the pairs call on the full table and of the device batch."""
    wl, abi, torch = pkg.workloads, pkg.abi, torch_cuda
    mesh = wl.mesh_variants(1, 12, 10)[0]
    L = pairs_model.mixed_library(pkg)
    plane = len(L)
    L.add_plane([1, 2, -1], 0.5)
    bvh = len(L)
    L.add_bvh(0, len(mesh.vertices))
    rng = np.random.default_rng(9)
    n_conf, nm, ne = 3, 20, 300
    n = nm + ne
    obj_shape = rng.integers(0, plane, n).astype(np.uint32)
    i_plane, i_mesh = nm + 270, nm + 5  # (the Plane in the second tile, the mesh in the first)
    obj_shape[i_plane], obj_shape[i_mesh] = plane, bvh
    T_env = rng.uniform(-4.0, 4.0, (ne, 3))
    T_env[256:, 0] += 40.0  # the second tile far away: only the Plane keeps it from being skipped
    env_tf = pkg.geometry.make_pose(quat=wl.uniform_quaternions(rng, ne), T=T_env).reshape(ne, 12)
    moving = pkg.geometry.make_pose(quat=wl.uniform_quaternions(rng, n_conf * nm), T=rng.uniform(-4.0, 4.0, (n_conf * nm, 3))).reshape(n_conf, nm, 12)
    moving[1, :, :9] = pkg.geometry.make_pose()[:9]  # a configuration of identity rotations
    moving[2, :, 9:] = T_env[5] + rng.uniform(-0.5, 0.5, (nm, 3))  # ... and one around the mesh
    full = env_model.full_table(moving, env_tf)
    lib = pkg.Library(L)
    lib.add_bvh(mesh)
    scene = lib.scene(obj_shape, np.zeros((0, 2), dtype=np.uint32))
    try:
        scene.set_environment(nm, env_tf)
        boxes = scene.world_aabbs(full)
        got_boxes, tiles = scene.environment_aabbs()
        _same(got_boxes, np.ascontiguousarray(boxes[0, nm:]), "environment boxes")
        _same(tiles, env_model.tile_boxes(got_boxes), "tile boxes")
        exp, exp_cb = env_model.env_pairs(boxes, nm, 0.0)
        for c in range(n_conf):
            mine = exp[int(exp_cb[c]):int(exp_cb[c + 1])]
            assert (mine[:, 1] == i_plane).sum() == nm, c
        assert (exp[:, 1] == i_mesh).any()
        for span, chunk in ((0, 0), (1, 0), (1, 7)):
            lib.set_option("scene_env_span", span)
            lib.set_option("scene_cull_chunk", chunk)
            pairs, cb = scene.env_pairs(moving, 0.0)
            _same(pairs, exp, "pairs, span %d chunk %d" % (span, chunk))
            _same(cb, exp_cb, "conf_begin, span %d chunk %d" % (span, chunk))
        lib.set_option("scene_env_span", 0)
        lib.set_option("scene_cull_chunk", 0)
        req = abi.default_collision_request()
        s1, s2, r1, r2 = pairs_model.expand(obj_shape, full, exp, exp_cb)
        dev = torch.device("cuda:0")
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s1.astype(np.int32), s2.astype(np.int32), r1, r2)]
        d_out = torch.zeros(len(s1) * 24, dtype=torch.int32, device=dev)
        d_g = torch.zeros(len(s1) * 8, dtype=torch.int32, device=dev)
        lib.collide_device(d[0], d[1], d[2], d[3], len(s1), req, d_out, None, d_g, stream=_stream(torch))
        torch.cuda.synchronize()
        exp_rec, exp_g = d_out.cpu().numpy().view(abi.RESULT_DTYPE), d_g.cpu().numpy().view(abi.GUESS_DTYPE)
        got, cb, k, (d_tab, d_pairs, d_cb) = _env_device(torch, scene, moving, 0.0, len(exp))
        d_full = torch.from_numpy(full).to(dev)
        for chunk in (0, 11):
            lib.set_option("scene_chunk", chunk)
            rec, summ, g = _on_env_list_device(torch, pkg, scene, d_tab, n_conf, d_pairs, k, d_cb, "collide", req, False)
            theirs, their_summ, their_g = _on_list_device(torch, pkg, scene, d_full, n_conf, d_pairs, k, d_cb, "collide", req, False)
            _same(rec, exp_rec, "records, chunk %d" % chunk)
            _same(rec, theirs, "records = the pairs call's, chunk %d" % chunk)
            _same(g, exp_g, "guesses, chunk %d" % chunk)
            _same(summ, their_summ, "summaries = the pairs call's, chunk %d" % chunk)
            _same(summ, pairs_model.fold_ranked(abi, exp_rec, exp_cb, 0.0), "summaries, chunk %d" % chunk)
        rec, pairs, cbh, summ = scene.collide_env(moving, req, 0.0)
        _same(rec, exp_rec, "host form records")
        _same(pairs, exp, "host form pairs")
    finally:
        lib.set_option("scene_chunk", 0)
        lib.set_option("scene_cull_chunk", 0)
        lib.set_option("scene_env_span", 0)
        scene.close()
        lib.close()


# ---- 6. existing calls ---------------------------------------------------------------------------------------------------------------------
def test_existing_calls_do_not_see_the_environment(pkg, torch_cuda, world):
    """self_pairs, collide_self and nearest_self on a full table return the same bytes before set_environment, after it, and after
    clear_environment."""
    es, scene = world["get"](17, 257, 3)
    scene.clear_environment()
    assert scene.n_moving == scene.n_objects == es.n

    def everything():
        out = list(scene.self_pairs(es.tf, 0.25)) + list(scene.self_pairs(es.pose, 0.0))
        out += list(scene.collide_self(es.tf, inflate=0.25, want_guess=True))
        clear, rec, n_eval = scene.nearest_self(es.tf, upper_bound=2.0)
        return out + [clear, rec, np.array(n_eval)]

    before = everything()
    _set_env(scene, es, False)
    during = everything()
    _set_env(scene, es, True)
    during32 = everything()
    scene.clear_environment()
    assert scene.n_moving == es.n
    after = everything()
    for k, a in enumerate(before):
        for name, other in (("after set_environment", during), ("after set_environment_f32", during32), ("after clear_environment", after)):
            _same(other[k], a, "output %d %s" % (k, name))
    with pytest.raises(pkg.EngineError) as e:
        scene.env_pairs(es.tf, 0.0)  # (without an environment every object counts as moving: the wrapper wants a full table, the call refuses)
    assert e.value.code == pkg.abi.ERR_INVALID_ARGUMENT and "no environment" in str(e.value)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, torch_cuda, world):
    """The code, and that nothing was written: a stale scene, n_moving > n_objects, no environment set, a precision mismatch, a negative
    or NaN inflate, a null count, a null table with n_conf > 0."""
    torch, abi, d = torch_cuda, pkg.abi, pkg.engine.dll()
    es, scene = world["get"](5, 255, 3)
    dev = torch.device("cuda:0")
    tab, tab32 = np.ascontiguousarray(es.moving_tf), np.ascontiguousarray(es.moving_pose)
    env, env32 = np.ascontiguousarray(es.env_tf), np.ascontiguousarray(es.env_pose)
    creq = abi.default_collision_request()
    three, cap = C.c_size_t(3), C.c_size_t(64)

    def refused(fn_name, handle, table, inflate=0.0, code=abi.ERR_INVALID_ARGUMENT, word="", count=True):
        """The host list form, the device list form and the host narrow-phase form of one precision."""
        f32 = fn_name.endswith("_f32")
        sfx = "_f32" if f32 else ""
        pairs = np.full((64, 2), FILL32, dtype=np.uint32)
        cb = np.full(4, FILL, dtype=np.uint64)
        summ = np.full(3 * 24, 0x5A, dtype=np.uint8)
        n = C.c_size_t(77)
        rc = getattr(d, "hfcl_scene_env_pairs" + sfx)(handle, abi.ptr(table) if table is not None else None, three, C.c_double(inflate), abi.ptr(pairs),
                                                      cap, abi.ptr(cb), C.byref(n) if count else None)
        assert rc == code and word in pkg.engine.last_error(), (fn_name, pkg.engine.last_error())
        args = [handle, abi.ptr(table) if table is not None else None, three, C.c_double(inflate), C.byref(creq), None, cap, abi.ptr(pairs), abi.ptr(cb),
                abi.ptr(summ)] + ([] if f32 else [None, None]) + [C.byref(n) if count else None]
        rc = getattr(d, "hfcl_scene_collide_env" + sfx)(*args)
        assert rc == code and word in pkg.engine.last_error(), (fn_name, pkg.engine.last_error())
        assert np.all(pairs == FILL32) and np.all(cb == FILL) and np.all(summ == 0x5A) and n.value == 77
        d_tab = torch.from_numpy(table).to(dev) if table is not None else None
        d_pairs = torch.full((128,), FILL32, dtype=torch.int32, device=dev)
        d_cb = torch.full((4,), FILL, dtype=torch.int64, device=dev)
        d_n = torch.full((1,), FILL, dtype=torch.int64, device=dev)
        rc = getattr(d, "hfcl_scene_env_pairs_device" + sfx)(handle, C.c_void_p(d_tab.data_ptr()) if d_tab is not None else None, three,
                                                             C.c_double(inflate), C.c_void_p(d_pairs.data_ptr()), cap, C.c_void_p(d_cb.data_ptr()),
                                                             C.c_void_p(d_n.data_ptr()) if count else None, C.c_void_p(_stream(torch)))
        assert rc == code and word in pkg.engine.last_error(), (fn_name, pkg.engine.last_error())
        d_sum = torch.full((18,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        args = [handle, C.c_void_p(d_tab.data_ptr()) if d_tab is not None else None, three, C.c_void_p(d_pairs.data_ptr()), C.c_size_t(4),
                C.c_void_p(d_cb.data_ptr()), C.byref(creq), None, C.c_void_p(d_sum.data_ptr())] + ([] if f32 else [None, None]) + [C.c_void_p(_stream(torch))]
        if count:  # (the narrow phase on a list has no count and no inflate: the refusals of the scene and the table)
            rc = getattr(d, "hfcl_scene_collide_env_pairs_device" + sfx)(*args)
            assert rc == code and word in pkg.engine.last_error(), (fn_name, pkg.engine.last_error())
        torch.cuda.synchronize()
        assert bool((d_pairs == FILL32).all()) and bool((d_cb == FILL).all()) and bool((d_n == FILL).all()) and bool((d_sum == 0x5A5A5A5A).all())

    # no environment set
    scene.clear_environment()
    refused("env", scene._h, tab, word="no environment")
    refused("env_f32", scene._h, tab32, word="no environment")
    boxes = np.full(6, 7.5)
    assert d.hfcl_scene_environment_aabbs(scene._h, abi.ptr(boxes), None) == abi.ERR_INVALID_ARGUMENT and np.all(boxes == 7.5)
    # n_moving > n_objects: refused, the scene as it was
    assert d.hfcl_scene_set_environment(scene._h, C.c_size_t(es.n + 1), abi.ptr(env)) == abi.ERR_INVALID_ARGUMENT
    assert "moving objects" in pkg.engine.last_error() and d.hfcl_scene_n_moving(scene._h) == es.n
    assert d.hfcl_scene_set_environment(scene._h, C.c_size_t(5), None) == abi.ERR_INVALID_ARGUMENT and "null environment" in pkg.engine.last_error()
    refused("env", scene._h, tab, word="no environment")
    # a precision mismatch, both ways
    _set_env(scene, es, False)
    refused("env_f32", scene._h, tab32, word="not converted")
    _set_env(scene, es, True)
    refused("env", scene._h, tab, word="not converted")
    # inflate, a null count, a null table
    _set_env(scene, es, False)
    for bad in (-0.5, np.nan):
        pairs = np.full((64, 2), FILL32, dtype=np.uint32)
        n = C.c_size_t(77)
        assert d.hfcl_scene_env_pairs(scene._h, abi.ptr(tab), three, C.c_double(bad), abi.ptr(pairs), cap, None, C.byref(n)) == abi.ERR_INVALID_ARGUMENT
        assert "inflate" in pkg.engine.last_error() and np.all(pairs == FILL32) and n.value == 77
        d_n = torch.full((1,), FILL, dtype=torch.int64, device=dev)
        d_tab = torch.from_numpy(tab).to(dev)
        rc = d.hfcl_scene_env_pairs_device(scene._h, C.c_void_p(d_tab.data_ptr()), three, C.c_double(bad), None, C.c_size_t(0), None,
                                           C.c_void_p(d_n.data_ptr()), C.c_void_p(_stream(torch)))
        torch.cuda.synchronize()
        assert rc == abi.ERR_INVALID_ARGUMENT and "inflate" in pkg.engine.last_error() and bool((d_n == FILL).all())
        with pytest.raises(pkg.EngineError):
            scene.collide_env(es.moving_tf, inflate=bad)
    refused("env", scene._h, tab, word="null count", count=False)
    refused("env", scene._h, None, word="null pose table")
    # n_conf == 0 and n_moving == 0: HFCL_OK, an empty list
    pairs, cb = scene.env_pairs(es.moving_tf[:0], 0.0)
    assert len(pairs) == 0 and cb.shape == (1,) and cb[0] == 0
    scene.set_environment(0, es.tf[0])
    pairs, cb = scene.env_pairs(np.zeros((3, 0, 12)), 0.0)
    assert len(pairs) == 0 and cb.shape == (4,) and not cb.any() and scene.n_moving == 0
    rec, pairs, cb, summ = scene.collide_env(np.zeros((3, 0, 12)))
    assert len(rec) == 0 and not cb.any() and np.all(np.isposinf(summ["min_distance"])) and np.all(summ["min_pair"] == NONE)
    _set_env(scene, es, False)
    # a scene made before hfcl_lib_set_shapes is refused, as in the other scene calls: the setter and the calls
    L = pairs_model.mixed_library(pkg)
    lib = pkg.Library(L)
    stale = lib.scene(es.obj_shape, np.zeros((0, 2), dtype=np.uint32))
    try:
        stale.set_environment(5, es.env_tf)
        shapes, verts = np.ascontiguousarray(L.shapes_array()), np.ascontiguousarray(L.vertices_array(), dtype=np.float64)
        assert d.hfcl_lib_set_shapes(lib._h, abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), C.c_size_t(len(verts))) == abi.OK
        refused("env", stale._h, tab, word="hfcl_lib_set_shapes")
        assert d.hfcl_scene_set_environment(stale._h, C.c_size_t(5), abi.ptr(env)) == abi.ERR_INVALID_ARGUMENT
        assert "hfcl_lib_set_shapes" in pkg.engine.last_error()
        assert d.hfcl_scene_set_environment_f32(stale._h, C.c_size_t(5), abi.ptr(env32)) == abi.ERR_INVALID_ARGUMENT
        assert d.hfcl_scene_clear_environment(stale._h) == abi.ERR_INVALID_ARGUMENT
    finally:
        stale.close()
        lib.close()


# ---- 8. Python and compat --------------------------------------------------------------------------------------------------------------------
def test_compat_scene_with_env_broadphase(pkg, torch_cuda):
    """compat.collide_scene / distance_scene(..., broadphase="env", n_moving=K): the results of broadphase="self" with the equivalent groups
    on the full transforms -- moving against moving and against the environment, no pair of two environment objects."""
    fcl = pkg.compat
    rng = np.random.default_rng(23)
    geoms = [fcl.Box(0.6, 0.8, 1.0), fcl.Sphere(0.5), fcl.Capsule(0.3, 1.2)]
    K, n, n_conf = 6, 40, 3
    objs = []
    for k in range(n):
        t = fcl.Transform3f()
        t.setTranslation(rng.uniform(-2.0, 2.0, 3))
        objs.append(fcl.CollisionObject(geoms[k % 3], t))
    own = np.concatenate([o.getTransform()._abi().reshape(1, 12) for o in objs])
    moving = np.stack([own[:K]] * n_conf)
    moving[1:, :, 9:] += rng.uniform(-1.0, 1.0, (n_conf - 1, K, 3))
    full = np.concatenate([moving, np.broadcast_to(own[K:], (n_conf, n - K, 12))], axis=1)
    group = (np.arange(n) >= K).astype(np.uint8)
    collides = np.array([[True, True], [True, False]])
    req = fcl.CollisionRequest()
    got, summ = fcl.collide_scene(objs, None, req, transforms=moving, broadphase="env", n_moving=K, inflate=0.1)
    want, want_summ = fcl.collide_scene(objs, None, req, transforms=full, broadphase="self", inflate=0.1, groups=(group, collides))
    everything, _ = fcl.collide_scene(objs, None, req, transforms=full, broadphase="self", inflate=0.1)
    assert len(got) == n_conf and summ.tobytes() == want_summ.tobytes()
    n_col = 0
    for c in range(n_conf):
        assert [ij for ij, _ in got[c]] == [ij for ij, _ in want[c]] == [ij for ij, _ in everything[c] if ij[0] < K]
        assert len(got[c]) < len(everything[c])  # (pairs of two environment objects exist and are not listed)
        for (_, g), (_, e) in zip(got[c], want[c]):
            assert g.numContacts() == e.numContacts() and g.distance_lower_bound == e.distance_lower_bound
            for k in range(g.numContacts()):
                a, b = g.getContact(k), e.getContact(k)
                assert a.o1 is b.o1 and a.o2 is b.o2 and a.penetration_depth == b.penetration_depth and np.array_equal(a.pos, b.pos)
            n_col += g.isCollision()
    assert n_col > 0
    listed = [ij for c in range(n_conf) for ij, _ in got[c]]
    assert any(j < K for _, j in listed) and any(j >= K for _, j in listed)  # (both kinds of pair)
    # one configuration, the objects' own transforms; distance; groups on top
    got1, _ = fcl.collide_scene(objs, None, req, broadphase="env", n_moving=K, inflate=0.1)
    assert [ij for ij, _ in got1] == [ij for ij, _ in got[0]]
    dist, pairs, dsumm = fcl.distance_scene(objs, None, fcl.DistanceRequest(), transforms=moving, broadphase="env", n_moving=K, inflate=0.5)
    wdist, wpairs, wsumm = fcl.distance_scene(objs, None, fcl.DistanceRequest(), transforms=full, broadphase="self", inflate=0.5, groups=(group, collides))
    assert dsumm.tobytes() == wsumm.tobytes()
    for c in range(n_conf):
        assert np.array_equal(pairs[c], wpairs[c]) and np.array_equal(dist[c], wdist[c]) and len(dist[c]) > 0
    chain = env_model.robot_groups(K, n)  # (links without their neighbours, the obstacles one group)
    got2, _ = fcl.collide_scene(objs, None, req, transforms=moving, broadphase="env", n_moving=K, inflate=0.1, groups=chain)
    want2, _ = fcl.collide_scene(objs, None, req, transforms=full, broadphase="self", inflate=0.1, groups=chain)
    for c in range(n_conf):
        assert [ij for ij, _ in got2[c]] == [ij for ij, _ in want2[c]] and not any(j == i + 1 and j < K for (i, j), _ in got2[c])
    with pytest.raises(ValueError):
        fcl.collide_scene(objs, None, req, broadphase="env")
    with pytest.raises(ValueError):
        fcl.collide_scene(objs, None, req, broadphase="self", n_moving=K)


def test_workload_and_spatial_order(pkg, torch_cuda):
    """workloads.scene_robot_env's two forms through the calls, the obstacles in generated order and in spatial_order: the env list with
    the workload's groups is the groups sweep's list on the full table (every entry of which has a link in front)."""
    wl = pkg.workloads
    for spatial in (False, True):
        sc, groups, P, (moving_tf, env_tf), (moving_pose, env_pose) = wl.scene_robot_env(6, 12, 1500, seed=3, split=True, spatial=spatial)
        lib = pkg.Library(sc.lib)
        scene = lib.scene(sc.obj_shape, np.zeros((0, 2), dtype=np.uint32))
        try:
            scene.set_groups(*groups)
            for moving, env, full in ((moving_tf, env_tf, sc.obj_tf), (moving_pose, env_pose, sc.obj_pose_f32)):
                scene.set_environment(12, env)
                want, want_cb = scene.self_pairs(full, 0.1)
                assert len(want) > 0 and want[:, 0].max() < 12
                pairs, cb = scene.env_pairs(moving, 0.1)
                _same(pairs, want, "the groups sweep's list, spatial %d" % spatial)
                _same(cb, want_cb, "conf_begin")
                rec, pairs2, cb2, summ = scene.collide_env(moving, inflate=0.1)
                wrec, _, _, wsumm = scene.collide_self(full, inflate=0.1)
                _same(rec, wrec, "records = collide_self's")
                _same(summ, wsumm, "summaries = collide_self's")
        finally:
            scene.close()
            lib.close()
