"""The clearance of the moving objects among an environment kept on the device (include/hppfcl_amd_nearest_env.h) on the GPU.  The
yardsticks, none of which runs the code under test: on a second scene that holds P_env as its explicit list, scene.distance (the
minimum's bits, the pair, the record's bytes) and scene.nearest (both pass counts, n_evaluated and n_skipped per configuration) on the
FULL table; and scene.nearest_self on the full table of another scene whose groups forbid exactly the environment x environment pairs
(tests/nearest_env_model.py: env_groups).  Outputs are pre-filled with a poison pattern: every element must be written.  Scenes and
references are made once and shared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import env_model
import nearest_env_model as model
import pairs_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
NO_PAIRS = np.zeros((0, 2), dtype=np.uint32)
SIZES = model.SIZES + [(64, 600), (130, 513)]
CONFS = {3: [1, 3, 4], 1: [3]}  # n_conf -> configurations of the five: (among, hover, graze); hover alone
BOUNDS = [np.inf, 0.5, 0.0]
GUARD = 3


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _poison(n, dtype):
    return np.full(max(n, 1) * dtype.itemsize, 0x5A, dtype=np.uint8).view(dtype)[:n]


class Case:
    """Some configurations of a NearestEnvScene, the groups (or None), and the references."""

    def __init__(self, pkg, lib, sc, confs, groups=None):
        self.pkg, self.lib, self.sc, self.groups = pkg, lib, sc, groups
        self.n_moving, self.n, self.n_conf = sc.n_moving, sc.n, len(confs)
        self.obj_shape = np.ascontiguousarray(sc.obj_shape, dtype=np.uint32)
        self.moving = {False: np.ascontiguousarray(sc.moving_tf[confs]), True: np.ascontiguousarray(sc.moving_pose[confs])}
        self.env = {False: sc.env_tf, True: sc.env_pose}
        self.full = {False: np.ascontiguousarray(sc.tf[confs]), True: np.ascontiguousarray(sc.pose[confs])}
        self.P = model.explicit_list(self.n_moving, self.n, groups)
        self._ref = {}

    def scene(self, f32):
        s = self.lib.scene(self.obj_shape, NO_PAIRS)
        if self.groups is not None:
            s.set_groups(*self.groups)
        s.set_environment(self.n_moving, self.env[f32])
        return s

    def ref(self, f32, D):
        """((records, summaries) of distance on P_env, (summaries, n_evaluated) of nearest on P_env with the bound D), full tables."""
        if ("full", f32) not in self._ref or (D, f32) not in self._ref:
            s = self.lib.scene(self.obj_shape, self.P)
            try:
                if ("full", f32) not in self._ref:
                    self._ref[("full", f32)] = (s.distance_f32 if f32 else s.distance)(self.full[f32]) if len(self.P) else None
                if (D, f32) not in self._ref:
                    summ, _, n = (s.nearest_f32 if f32 else s.nearest)(self.full[f32], upper_bound=D, records=False)
                    self._ref[(D, f32)] = (summ, n)
            finally:
                s.close()
        return self._ref[("full", f32)], self._ref[(D, f32)]

    def ref_self(self, f32, D):
        """nearest_self on the full table with the environment group."""
        if ("self", D, f32) not in self._ref:
            s = self.lib.scene(self.obj_shape, NO_PAIRS)
            try:
                s.set_groups(*model.env_groups(self.n_moving, self.n, self.groups))
                self._ref[("self", D, f32)] = s.nearest_self(self.full[f32], upper_bound=D)
            finally:
                s.close()
        return self._ref[("self", D, f32)]


def _call(torch, case, scene, f32, device, D=np.inf, records=True):
    """One call in the host or the device form into poisoned outputs with guard entries behind them: (clearance, min_records, n_evaluated)."""
    abi, d = case.pkg.abi, case.pkg.engine.dll()
    rdt = abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE
    cdt = abi.SCENE_CLEARANCE_DTYPE
    table = case.moving[f32]
    req = abi.default_distance_request()
    n = (C.c_size_t * 2)(77, 77)
    nc = case.n_conf
    if not device:
        out, rec = _poison(nc + GUARD, cdt), (_poison(nc + GUARD, rdt) if records else None)
        fn = d.hfcl_scene_nearest_env_f32 if f32 else d.hfcl_scene_nearest_env
        rc = fn(scene._h, abi.ptr(table) if table.size else None, C.c_size_t(nc), C.byref(req), C.c_double(D), abi.ptr(out), abi.ptr(rec), n)
        assert rc == 0, case.pkg.engine.last_error()
    else:
        dev = torch.device("cuda:0")
        d_tab = torch.from_numpy(table).to(dev) if table.size else None
        d_out = torch.full(((nc + GUARD) * cdt.itemsize,), 0x5A, dtype=torch.uint8, device=dev)
        d_rec = torch.full(((nc + GUARD) * rdt.itemsize,), 0x5A, dtype=torch.uint8, device=dev) if records else None
        fn = scene.nearest_env_device_f32 if f32 else scene.nearest_env_device
        n = fn(d_tab, nc, req, d_out, d_rec, upper_bound=D, stream=_stream(torch))
        torch.cuda.synchronize()
        out, rec = d_out.cpu().numpy().view(cdt), (d_rec.cpu().numpy().view(rdt) if records else None)
    assert out[nc:].tobytes() == _poison(GUARD, cdt).tobytes()  # nothing is written behind the outputs
    if records:
        assert rec[nc:].tobytes() == _poison(GUARD, rdt).tobytes()
    return out[:nc], (rec[:nc] if records else None), (int(n[0]), int(n[1]))


def _check(case, got, f32, D=np.inf, against_self=True):
    """The promises of the header against distance and nearest on P_env, and the cross-check against nearest_self.  Returns the
    configurations beyond the bound."""
    clear, rec, n_eval = got
    beyond = 0
    if len(case.P):
        (full_rec, full), (near, near_n) = case.ref(f32, D)
        n_pairs = len(case.P)
        within = full["min_distance"] <= D
        assert clear["min_distance"][within].tobytes() == full["min_distance"][within].tobytes()
        mp = full["min_pair"][within].astype(np.int64)
        assert np.array_equal(clear["min_i"][within], case.P[mp, 0]) and np.array_equal(clear["min_j"][within], case.P[mp, 1])
        if rec is not None:
            want = full_rec.reshape(case.n_conf, n_pairs)[np.flatnonzero(within), mp]
            assert rec[within].tobytes() == want.tobytes()
        assert np.all(clear["min_distance"][~within] > D)
        # the identity with nearest on P_env
        assert n_eval == near_n
        assert clear["min_distance"].tobytes() == near["min_distance"].tobytes()
        assert np.array_equal(clear["n_skipped"], near["n_skipped"])
        has = near["min_pair"] != NONE
        assert np.array_equal(clear["min_i"][has], case.P[near["min_pair"][has].astype(np.int64), 0])
        assert np.array_equal(clear["min_j"][has], case.P[near["min_pair"][has].astype(np.int64), 1])
        assert np.all(clear["min_i"][~has] == NONE) and np.all(clear["min_j"][~has] == NONE)
        assert int(clear["n_evaluated"].sum()) == sum(n_eval)
        if rec is not None:
            assert np.all(rec["status"][~has] == 0x80000000) and np.all(np.isposinf(rec["distance"][~has]))
        beyond = int((~within).sum())
    if against_self:
        s_clear, s_rec, s_n = case.ref_self(f32, D)
        assert clear.tobytes() == s_clear.tobytes() and n_eval == s_n
        if rec is not None:
            assert rec.tobytes() == s_rec.tobytes()
    return beyond


@pytest.fixture(scope="module")
def world(pkg, torch_cuda, oracle):
    """One library (cfg5's mix); the scenes are made once (seed 0) and not modified."""
    L = pairs_model.mixed_library(pkg)
    lib = pkg.Library(L)
    made = {}

    def scene(n_moving, n_env):
        if (n_moving, n_env) not in made:
            made[(n_moving, n_env)] = model.NearestEnvScene(pkg, oracle, L, n_moving, n_env, 0)
        return made[(n_moving, n_env)]

    def case(n_moving, n_env, n_conf, with_groups=False):
        key = (n_moving, n_env, n_conf, with_groups)
        if key not in made:
            groups = env_model.robot_groups(n_moving, n_moving + n_env) if with_groups else None
            made[key] = Case(pkg, lib, scene(n_moving, n_env), CONFS[n_conf], groups)
        return made[key]

    yield dict(lib=lib, L=L, case=case)
    lib.close()


# ---- forms and sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("n_moving,n_env", SIZES)
def test_forms_and_sizes(pkg, torch_cuda, world, n_moving, n_env, f32):
    """Host and device forms, one and three configurations, three upper bounds: identical to the yardsticks wherever promised,
    min_distance > upper_bound elsewhere."""
    evaluated = {}
    for n_conf in (1, 3):
        case = world["case"](n_moving, n_env, n_conf)
        scene = case.scene(f32)
        try:
            for D in BOUNDS:
                host = _call(torch_cuda, case, scene, f32, False, D)
                beyond = _check(case, host, f32, D)
                dev = _call(torch_cuda, case, scene, f32, True, D)
                assert host[0].tobytes() == dev[0].tobytes() and host[1].tobytes() == dev[1].tobytes() and host[2] == dev[2], (n_conf, D)
                evaluated[(n_conf, D)] = (host[2], beyond)
            bare = _call(torch_cuda, case, scene, f32, True, records=False)  # clearances alone
            assert bare[0].tobytes() == _call(torch_cuda, case, scene, f32, False)[0].tobytes()
        finally:
            scene.close()
    print("(%d, %d) f32 %d: %d candidates a configuration; (n_conf, D) -> (n_evaluated, configurations beyond D): %s"
          % (n_moving, n_env, f32, len(case.P), evaluated))
    if len(case.P) >= env_model.SHARE_MIN_ALLOWED:
        assert sum(evaluated[(1, np.inf)][0]) <= model.HOVER_SHARE * len(case.P)  # hover alone
        assert evaluated[(1, 0.0)][1] == 1                                          # ... is clear: beyond a bound of 0


def test_thirty_seven_configurations_against_nearest_self(pkg, torch_cuda, world):
    """(130, 513) x 37 configurations of the EnvScene, against nearest_self on the full table alone."""
    es = env_model.EnvScene(pkg, world["L"], 130, 513, 37)
    sc = type("S", (), dict(n_moving=130, n=es.n, obj_shape=es.obj_shape, moving_tf=es.moving_tf, moving_pose=es.moving_pose, env_tf=es.env_tf,
                            env_pose=es.env_pose, tf=es.tf, pose=es.pose))
    case = Case(pkg, world["lib"], sc, list(range(37)))
    for f32 in (False, True):
        scene = case.scene(f32)
        try:
            for device in (False, True):
                got = _call(torch_cuda, case, scene, f32, device)
                s_clear, s_rec, s_n = case.ref_self(f32, np.inf)
                assert got[0].tobytes() == s_clear.tobytes() and got[1].tobytes() == s_rec.tobytes() and got[2] == s_n
                assert (got[0]["min_distance"][1:] < 0).any() and got[0]["min_distance"][0] > 0
        finally:
            scene.close()


# ---- cuts and pruning ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_moving,n_env", [(17, 257), (65, 600)])
def test_spans_chunks_and_pruning_give_the_same_bytes(pkg, torch_cuda, world, n_moving, n_env):
    lib = world["lib"]
    case = world["case"](n_moving, n_env, 3)
    scene = case.scene(False)
    try:
        base = _call(torch_cuda, case, scene, False, False)
        _check(case, base, False)
        for span in (1, 2, 0):
            for chunk in (16, 0):
                for prune in (0, 1):
                    lib.set_option("scene_env_span", span)
                    lib.set_option("scene_cull_chunk", chunk)
                    lib.set_option("scene_nearest_env_prune", prune)
                    for device in ((False, True) if span == 1 else (chunk == 16,)):
                        got = _call(torch_cuda, case, scene, False, device)
                        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[2] == base[2], (span, chunk, prune)
    finally:
        lib.set_option("scene_env_span", 0)  # (the defaults)
        lib.set_option("scene_cull_chunk", 0)
        lib.set_option("scene_nearest_env_prune", 1)
        scene.close()


# ---- groups ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_moving,n_env", [(5, 255), (17, 257)])
def test_groups(pkg, torch_cuda, world, n_moving, n_env):
    """env_model.robot_groups: the chain's neighbours may not pair, the environment is one group."""
    case = world["case"](n_moving, n_env, 3, True)
    plain = world["case"](n_moving, n_env, 3)
    assert 0 < len(case.P) < len(plain.P)
    for f32 in (False, True):
        scene = case.scene(f32)
        try:
            for D in (np.inf, 0.5):
                host = _call(torch_cuda, case, scene, f32, False, D)
                _check(case, host, f32, D)
                dev = _call(torch_cuda, case, scene, f32, True, D)
                assert host[0].tobytes() == dev[0].tobytes() and host[1].tobytes() == dev[1].tobytes() and host[2] == dev[2]
            scene.clear_groups()  # the call follows the scene's groups
            _check(plain, _call(torch_cuda, plain, scene, f32, False), f32)
        finally:
            scene.close()


# ---- the environment's tables ------------------------------------------------------------------------------------------------------------------
def test_a_second_environment_replaces_the_terms(pkg, torch_cuda, world):
    """Set, call, set another environment (the same objects elsewhere, and another n_moving), call: what a fresh scene gives."""
    lib = world["lib"]
    a = world["case"](17, 257, 3)
    # both on the objects of `a`: environment B is A's moved and turned round, with the first 19 objects moving
    sc = a.sc
    shifted = np.ascontiguousarray(sc.tf[CONFS[3]])
    shifted[:, 19:, 9:] = shifted[:, 19:, 9:][:, ::-1] + np.array([0.5, -0.25, 0.125])
    other = type("S", (), dict(n_moving=19, n=sc.n, obj_shape=sc.obj_shape, moving_tf=shifted[:, :19], moving_pose=sc.moving_pose[:, :19],
                               env_tf=np.ascontiguousarray(shifted[0, 19:]), env_pose=sc.env_pose[2:], tf=shifted, pose=sc.pose))
    case_b = Case(pkg, lib, other, [0, 1, 2])
    scene = a.scene(False)
    try:
        first = _call(torch_cuda, a, scene, False, False)
        _check(a, first, False)
        scene.set_environment(19, case_b.env[False])
        second = _call(torch_cuda, case_b, scene, False, False)
        _check(case_b, second, False)
        fresh = case_b.scene(False)
        try:
            want = _call(torch_cuda, case_b, fresh, False, False)
        finally:
            fresh.close()
        assert second[0].tobytes() == want[0].tobytes() and second[1].tobytes() == want[1].tobytes() and second[2] == want[2]
        scene.set_environment(a.n_moving, a.env[False])  # ... and back
        third = _call(torch_cuda, a, scene, False, True)
        assert third[0].tobytes() == first[0].tobytes() and third[1].tobytes() == first[1].tobytes() and third[2] == first[2]
    finally:
        scene.close()


def test_the_env_lists_are_unchanged_by_the_new_tables(pkg, torch_cuda, world):
    """hfcl_scene_environment_aabbs and the env list of a scene are what they were: the model's."""
    case = world["case"](17, 257, 3)
    scene = case.scene(False)
    try:
        boxes, tiles = scene.environment_aabbs()
        assert boxes.tobytes() == np.ascontiguousarray(case.sc.boxes[0, case.n_moving:]).tobytes()
        assert tiles.tobytes() == env_model.tile_boxes(boxes).tobytes()
        pairs, cb = scene.env_pairs(case.moving[False], 0.25)
        want, want_cb = env_model.env_pairs(case.sc.boxes[CONFS[3]], case.n_moving, 0.25)
        assert pairs.tobytes() == want.tobytes() and cb.tobytes() == want_cb.tobytes()
    finally:
        scene.close()


# ---- refusals and edge cases -------------------------------------------------------------------------------------------------------------------
def test_refusals_and_edge_cases(pkg, torch_cuda, world):
    abi, d = pkg.abi, pkg.engine.dll()
    case = world["case"](5, 255, 3)
    req = abi.default_distance_request()
    cdt = abi.SCENE_CLEARANCE_DTYPE
    out = _poison(3, cdt)
    n = (C.c_size_t * 2)(7, 7)
    tab, pose = case.moving[False], case.moving[True]
    inf = C.c_double(np.inf)
    scene = world["lib"].scene(case.obj_shape, NO_PAIRS)
    try:
        # no environment set
        assert d.hfcl_scene_nearest_env(scene._h, abi.ptr(tab), C.c_size_t(3), C.byref(req), inf, abi.ptr(out), None, n) == abi.ERR_INVALID_ARGUMENT
        assert "no environment" in pkg.engine.last_error()
        scene.set_environment(case.n_moving, case.env[False])
        # the setter of the other precision: the env calls' message
        assert d.hfcl_scene_nearest_env_f32(scene._h, abi.ptr(pose), C.c_size_t(3), C.byref(req), inf, abi.ptr(out), None, n) == abi.ERR_INVALID_ARGUMENT
        assert "other precision" in pkg.engine.last_error() and "hfcl_scene_set_environment" in pkg.engine.last_error()
        assert d.hfcl_scene_nearest_env_device_f32(scene._h, None, C.c_size_t(3), C.byref(req), inf, abi.ptr(out), None, n, None) == abi.ERR_INVALID_ARGUMENT
        assert "other precision" in pkg.engine.last_error()
        for args, word in (((abi.ptr(tab), C.c_size_t(3), C.byref(req), inf, None, None, n), "null output"),
                           ((abi.ptr(tab), C.c_size_t(3), None, inf, abi.ptr(out), None, n), "null request"),
                           ((abi.ptr(tab), C.c_size_t(3), C.byref(req), C.c_double(np.nan), abi.ptr(out), None, n), "upper_bound"),
                           ((None, C.c_size_t(3), C.byref(req), inf, abi.ptr(out), None, n), "null pose table")):
            assert d.hfcl_scene_nearest_env(scene._h, *args) == abi.ERR_INVALID_ARGUMENT
            assert word in pkg.engine.last_error(), pkg.engine.last_error()
        assert tuple(n) == (7, 7) and out.tobytes() == _poison(3, cdt).tobytes()
        # n_conf == 0: nothing to do, nothing written but the counts
        assert d.hfcl_scene_nearest_env(scene._h, None, C.c_size_t(0), C.byref(req), inf, abi.ptr(out), None, n) == 0
        assert tuple(n) == (0, 0) and out.tobytes() == _poison(3, cdt).tobytes()
        # n_moving == 0: the "no record" answers, both forms
        scene.set_environment(0, np.ascontiguousarray(case.full[False][0]))
        empty = Case(pkg, world["lib"], type("S", (), dict(n_moving=0, n=case.n, obj_shape=case.obj_shape, moving_tf=np.zeros((5, 0, 12)),
                                                         moving_pose=np.zeros((5, 0, 7), dtype=np.float32), env_tf=None, env_pose=None,
                                                         tf=case.sc.tf, pose=case.sc.pose)), [0, 1, 2])
        for device in (False, True):
            clear, rec, cnt = _call(torch_cuda, empty, scene, False, device)
            assert cnt == (0, 0) and np.all(np.isposinf(clear["min_distance"])) and np.all(clear["min_i"] == NONE) and np.all(clear["min_j"] == NONE)
            assert not clear["n_evaluated"].any() and not clear["n_skipped"].any()
            assert np.all(rec["status"] == 0x80000000) and np.all(np.isposinf(rec["distance"]))
    finally:
        scene.close()
    # groups that allow no pair: no candidate
    none = Case(pkg, world["lib"], case.sc, CONFS[3], (np.zeros(case.n, dtype=np.uint8), np.array([0], dtype=np.uint64)))
    scene = none.scene(False)
    try:
        for device in (False, True):
            clear, rec, cnt = _call(torch_cuda, none, scene, False, device)
            assert cnt == (0, 0) and np.all(np.isposinf(clear["min_distance"])) and np.all(clear["min_i"] == NONE)
            assert np.all(rec["status"] == 0x80000000)
    finally:
        scene.close()


def test_workspace_is_shared_with_the_other_scene_calls(pkg, torch_cuda, world):
    """A nearest_self and an env list in between leave the answer as it was, and are themselves what a scene that never ran
    nearest_env gives."""
    case = world["case"](17, 257, 3)
    scene = case.scene(False)
    other = case.scene(False)
    try:
        first = _call(torch_cuda, case, scene, False, False)
        between = scene.nearest_self(case.full[False])
        listed = scene.distance_env(case.moving[False], inflate=0.25)
        third = _call(torch_cuda, case, scene, False, False)
        assert first[0].tobytes() == third[0].tobytes() and first[1].tobytes() == third[1].tobytes() and first[2] == third[2]
        want = other.nearest_self(case.full[False])
        assert between[0].tobytes() == want[0].tobytes() and between[1].tobytes() == want[1].tobytes() and between[2] == want[2]
        for a, b in zip(listed, other.distance_env(case.moving[False], inflate=0.25)):
            assert a.tobytes() == b.tobytes()
    finally:
        scene.close()
        other.close()


# ---- the front ends ----------------------------------------------------------------------------------------------------------------------------
def test_bindings(pkg, torch_cuda, world):
    case = world["case"](17, 257, 3)
    scene = case.scene(False)
    try:
        want = _call(torch_cuda, case, scene, False, False, 0.5)
        got = scene.nearest_env(case.moving[False], upper_bound=0.5)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
        bare = scene.nearest_env(case.moving[False], upper_bound=0.5, records=False)
        assert bare[1] is None and bare[0].tobytes() == want[0].tobytes()
    finally:
        scene.close()


def test_compat_distance_scene(pkg, torch_cuda):
    """compat.distance_scene(..., broadphase="env", nearest=True, n_moving=K): the DistanceResult of the closest pair that has a moving
    object in it, what nearest=True with broadphase="self" and the two managers' groups gives on the full tables."""
    fcl = pkg.compat
    rng = np.random.default_rng(3)
    geoms = [fcl.Box(0.5, 0.4, 0.3), fcl.Sphere(0.3), fcl.Capsule(0.2, 0.6)]
    K, n = 4, 30
    objs = []
    for i in range(n):
        t = fcl.Transform3f()
        t.setTranslation(rng.uniform(-4, 4, 3))
        objs.append(fcl.CollisionObject(geoms[i % 3], t))
    req = fcl.DistanceRequest()
    moving = np.stack([np.concatenate([o.getTransform()._abi().reshape(1, 12) for o in objs[:K]]) for _ in range(2)])
    moving[1, :, 9:] += 0.25
    full = np.stack([np.concatenate([moving[c]] + [o.getTransform()._abi().reshape(1, 12) for o in objs[K:]]) for c in range(2)])
    got = fcl.distance_scene(objs, None, req, moving, broadphase="env", nearest=True, n_moving=K)
    group = (np.arange(n) >= K).astype(np.uint8)
    want = fcl.distance_scene(objs, None, req, full, broadphase="self", nearest=True, groups=(group, np.array([3, 1], dtype=np.uint64)))
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert a.min_distance == b.min_distance and a.o1 is b.o1 and a.o2 is b.o2 and np.array_equal(a.normal, b.normal)
        assert np.array_equal(a.nearest_points[0], b.nearest_points[0]) and np.array_equal(a.nearest_points[1], b.nearest_points[1])
        assert any(a.o1 is o.collisionGeometry() for o in objs[:K])


def test_cpp_shim(pkg, torch_cuda, tmp_path):
    exe = str(tmp_path / "test_nearest_env_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_nearest_env", "test_nearest_env_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("same") == 4 and "DIFFERENT" not in r.stdout
