"""The clearance per configuration on device-made pairs (include/hppfcl_amd_nearest_self.h) on the GPU.  The yardsticks, on a second
scene that holds every allowed pair as the explicit lexicographic list P: scene.distance (the minimum's bits, the pair, the record's
bytes) and scene.nearest (both pass counts, n_evaluated and n_skipped per configuration: the same bounds, predicates and tie rule, so
an identity); where the lists themselves are looked at, the numpy model of tests/nearest_self_model.py (held against the g++ build of
the kernels' arithmetic in tests/test_scene_nearest_self_cpu.py) fed with the device's records.  Outputs are pre-filled with a poison
pattern: every element must be written.  References are computed once per scene and shared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nearest_model
import nearest_self_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
NO_PAIRS = np.zeros((0, 2), dtype=np.uint32)
ROBOTS = [(8, 6, 40, 3.0), (8, 6, 100, 3.0), (4, 6, 300, 3.0), (8, 12, 300, 1.0)]


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _poison(n, dtype):
    return np.full(max(n, 1) * dtype.itemsize, 0x5A, dtype=np.uint8).view(dtype)[:n]


class Case:
    """Objects of one library, their pose tables, the groups (or None) and the references on the explicit list P."""

    def __init__(self, pkg, lib, obj_shape, tf, pose, groups):
        self.pkg, self.lib, self.obj_shape, self.tf, self.pose, self.groups = pkg, lib, np.ascontiguousarray(obj_shape, dtype=np.uint32), tf, pose, groups
        self.n_conf, self.n = tf.shape[:2]
        self.P = model.explicit_list(self.n, groups)
        self._ref = {}

    def table(self, f32):
        return self.pose if f32 else self.tf

    def scene(self):
        s = self.lib.scene(self.obj_shape, NO_PAIRS)
        if self.groups is not None:
            s.set_groups(*self.groups)
        return s

    def ref(self, f32, D=np.inf):
        """(records, summaries) of distance on P, (summaries, n_evaluated) of nearest on P with the bound D."""
        if ("full", f32) not in self._ref or (D, f32) not in self._ref:
            s = self.lib.scene(self.obj_shape, self.P)
            try:
                if ("full", f32) not in self._ref:
                    self._ref[("full", f32)] = (s.distance_f32 if f32 else s.distance)(self.table(f32)) if len(self.P) else None
                if (D, f32) not in self._ref:
                    summ, _, n = (s.nearest_f32 if f32 else s.nearest)(self.table(f32), upper_bound=D, records=False)
                    self._ref[(D, f32)] = (summ, n)
            finally:
                s.close()
        return self._ref[("full", f32)], self._ref[(D, f32)]


def _call(torch, case, scene, f32, device, D=np.inf, records=True):
    """One call in the host or the device form into poisoned outputs: (clearance, min_records, n_evaluated)."""
    abi, d = case.pkg.abi, case.pkg.engine.dll()
    rdt = abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE
    table = np.ascontiguousarray(case.table(f32))
    req = abi.default_distance_request()
    n = (C.c_size_t * 2)(77, 77)
    if not device:
        out, rec = _poison(case.n_conf, abi.SCENE_CLEARANCE_DTYPE), (_poison(case.n_conf, rdt) if records else None)
        fn = d.hfcl_scene_nearest_self_f32 if f32 else d.hfcl_scene_nearest_self
        rc = fn(scene._h, abi.ptr(table), C.c_size_t(case.n_conf), C.byref(req), C.c_double(D), abi.ptr(out), abi.ptr(rec), n)
        assert rc == 0, case.pkg.engine.last_error()
        return out, rec, (int(n[0]), int(n[1]))
    dev = torch.device("cuda:0")
    d_tab = torch.from_numpy(table).to(dev)
    d_out = torch.full((case.n_conf * 24,), 0x5A, dtype=torch.uint8, device=dev)
    d_rec = torch.full((case.n_conf * rdt.itemsize,), 0x5A, dtype=torch.uint8, device=dev) if records else None
    fn = scene.nearest_self_device_f32 if f32 else scene.nearest_self_device
    got = fn(d_tab, case.n_conf, req, d_out, d_rec, upper_bound=D, stream=_stream(torch))
    torch.cuda.synchronize()
    return (d_out.cpu().numpy().view(abi.SCENE_CLEARANCE_DTYPE), d_rec.cpu().numpy().view(rdt) if records else None, got)


def _check(case, got, f32, D=np.inf):
    """The promises of the header against distance and nearest on P.  Returns the configurations beyond the bound."""
    clear, rec, n_eval = got
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
    # the identity with nearest on P
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
    return int((~within).sum())


def _per_conf_evaluated(case, f32, D=np.inf):
    """n_evaluated per configuration as the model lists it from the device's own boxes and records."""
    (full_rec, _), _ = case.ref(f32, D)
    s = case.lib.scene(case.obj_shape, NO_PAIRS)
    try:
        boxes = s.world_aabbs(case.table(f32))
    finally:
        s.close()
    return model.select(case.pkg.abi, boxes, case.groups, full_rec, D, nearest_model.R32 if f32 else nearest_model.R64)


@pytest.fixture(scope="module")
def world(pkg, torch_cuda):
    """The robot scenes share one shape library (scene_robot_env draws it from the seed alone); every case is made once and not modified."""
    made = {}
    libs = []

    def robot(key):
        if key not in made:
            ps, groups, P = pkg.workloads.scene_robot_env(key[0], key[1], key[2], seed=1, spread=key[3])
            if not libs:
                libs.append(pkg.Library(ps.lib))
            case = Case(pkg, libs[0], ps.obj_shape, ps.obj_tf, ps.obj_pose_f32, groups)
            assert np.array_equal(case.P, P)
            made[key] = case
        return made[key]

    def free(n, n_conf=3):
        """Without groups: n objects of the same library, scattered."""
        key = ("free", n, n_conf)
        if key not in made:
            robot(ROBOTS[0])
            rng = np.random.default_rng([7, n])
            shape = rng.integers(0, 64 * 5, n).astype(np.uint32)
            quat = pkg.workloads.uniform_quaternions(rng, n_conf * n)
            T = rng.uniform(-4, 4, (n_conf * n, 3))
            tf = pkg.geometry.make_pose(quat=quat, T=T).reshape(n_conf, n, 12)
            pose = pkg.geometry.pose_f32_from_quat(quat, T).reshape(n_conf, n, 7)
            made[key] = Case(pkg, libs[0], shape, tf, pose, None)
        return made[key]

    yield dict(robot=robot, free=free, lib=lambda: (robot(ROBOTS[0]), libs[0])[1])
    for lib in libs:
        lib.close()


# ---- the four scenes of the issue's table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("key", ROBOTS)
def test_robot_scenes(pkg, torch_cuda, world, key, f32):
    case = world["robot"](key)
    scene = case.scene()
    try:
        host = _call(torch_cuda, case, scene, f32, False)
        assert _check(case, host, f32) == 0
        dev = _call(torch_cuda, case, scene, f32, True)
        for a, b in zip(host[:2], dev[:2]):
            assert a.tobytes() == b.tobytes()
        assert host[2] == dev[2]
        share = 100.0 * sum(host[2]) / (case.n_conf * len(case.P))
        print("scene_robot_env%r f32 %d: %d + %d of %d candidates evaluated (%.2f %%)" % (key, f32, host[2][0], host[2][1], case.n_conf * len(case.P), share))
        if key[3] == 3.0:
            assert share <= 5.0
        else:
            assert host[2][1] == 0  # dense: pass 2 is empty
        # summaries alone
        bare = _call(torch_cuda, case, scene, f32, True, records=False)
        assert bare[0].tobytes() == host[0].tobytes() and bare[2] == host[2]
    finally:
        scene.close()


def test_lists_are_the_models(pkg, torch_cuda, world):
    """n_evaluated per configuration: the model's two lists from the device's own boxes."""
    for key, f32 in ((ROBOTS[0], False), (ROBOTS[2], True)):
        case = world["robot"](key)
        scene = case.scene()
        try:
            clear, rec, n_eval = _call(torch_cuda, case, scene, f32, False)
        finally:
            scene.close()
        exp = _per_conf_evaluated(case, f32)
        assert n_eval == (len(exp["pairs1"]), len(exp["pairs2"]))
        assert clear.tobytes() == exp["clearance"].tobytes() and rec.tobytes() == exp["min_records"].tobytes()


# ---- without groups, both kernel forms, the options ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [20, 70])
def test_all_pairs_without_groups(pkg, torch_cuda, world, n):
    case = world["free"](n)
    assert len(case.P) == n * (n - 1) // 2
    scene = case.scene()
    try:
        for f32 in (False, True):
            host = _call(torch_cuda, case, scene, f32, False)
            assert _check(case, host, f32) == 0
            dev = _call(torch_cuda, case, scene, f32, True)
            assert host[0].tobytes() == dev[0].tobytes() and host[1].tobytes() == dev[1].tobytes() and host[2] == dev[2]
            assert sum(host[2]) < case.n_conf * len(case.P) / 2
    finally:
        scene.close()


def test_small_and_tiled_forms_and_chunks_give_the_same_bytes(pkg, torch_cuda, world):
    lib = world["lib"]()
    try:
        for case in (world["robot"](ROBOTS[0]), world["free"](20), world["robot"](ROBOTS[2])):
            scene = case.scene()
            try:
                base = _call(torch_cuda, case, scene, False, False)
                _check(case, base, False)
                for small_max, chunk in ((0, 0), (64, 16), (0, 16), (64, 1)):
                    lib.set_option("scene_pairs_small_max", small_max)
                    lib.set_option("scene_cull_chunk", chunk)
                    for device in (False, True):
                        got = _call(torch_cuda, case, scene, False, device)
                        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[2] == base[2], (small_max, chunk)
                    lib.set_option("scene_pairs_small_max", 32)
                    lib.set_option("scene_cull_chunk", 0)
            finally:
                scene.close()
    finally:
        lib.set_option("scene_pairs_small_max", 32)  # (the defaults)
        lib.set_option("scene_cull_chunk", 0)


@pytest.mark.parametrize("D", [0.5, 0.05])
def test_upper_bound(pkg, torch_cuda, world, D):
    case = world["robot"](ROBOTS[0])
    scene = case.scene()
    try:
        unbounded = _call(torch_cuda, case, scene, False, False)
        for device in (False, True):
            got = _call(torch_cuda, case, scene, False, device, D)
            beyond = _check(case, got, False, D)
            assert 0 < beyond < case.n_conf
            assert sum(got[2]) < sum(unbounded[2])
    finally:
        scene.close()


# ---- ties -------------------------------------------------------------------------------------------------------------------------------
def test_ties_report_the_lowest_pair(pkg, torch_cuda):
    """A 4 x 4 x 4 grid of identical spheres at equal spacing, one group, a matrix of all ones: many pairs attain the minimum, many
    boxes the smallest bound."""
    L = pkg.ShapeLibrary()
    L.add_sphere(0.25)
    lib = pkg.Library(L)
    try:
        k = np.arange(64)
        T = np.stack([k // 16, (k // 4) % 4, k % 4], axis=1).astype(np.float64)  # (integers and a radius of 1/4: every sum is exact)
        quat = np.tile([1.0, 0, 0, 0], (64, 1))
        tf = pkg.geometry.make_pose(quat=quat, T=T).reshape(1, 64, 12)
        pose = pkg.geometry.pose_f32_from_quat(quat, T).reshape(1, 64, 7)
        groups = (np.zeros(64, dtype=np.uint8), np.array([1], dtype=np.uint64))
        case = Case(pkg, lib, np.zeros(64, dtype=np.uint32), tf, pose, groups)
        assert len(case.P) == 64 * 63 // 2
        scene = case.scene()
        try:
            for small_max in (64, 0):
                lib.set_option("scene_pairs_small_max", small_max)
                for f32 in (False, True):
                    got = _call(torch_cuda, case, scene, f32, False)
                    assert _check(case, got, f32) == 0
                    (full_rec, full), _ = case.ref(f32)
                    ties = int((full_rec["distance"] == full_rec["distance"][0]).sum())
                    print("f32 %d: %d pairs attain the minimum %r" % (f32, ties, float(full["min_distance"][0])))
                    assert ties > 1 and full["min_pair"][0] == 0 and (got[0]["min_i"][0], got[0]["min_j"][0]) == (0, 1)
                    exp = _per_conf_evaluated(case, f32)
                    assert got[2] == (len(exp["pairs1"]), len(exp["pairs2"])) and got[2][0] == 1 and got[2][1] == 143  # (3 * 16 * 3 neighbours, less the seed)
                    assert got[0].tobytes() == exp["clearance"].tobytes()
        finally:
            scene.close()
    finally:
        lib.close()


# ---- degenerate cases -------------------------------------------------------------------------------------------------------------------
def test_scenes_without_a_pair(pkg, torch_cuda, world):
    """One object; groups that allow no pair; no configuration."""
    abi = pkg.abi
    free = world["free"](20)
    one = Case(pkg, free.lib, free.obj_shape[:1], free.tf[:, :1], free.pose[:, :1], None)
    nothing = Case(pkg, free.lib, free.obj_shape, free.tf, free.pose, (np.zeros(20, dtype=np.uint8), np.array([0], dtype=np.uint64)))
    for case in (one, nothing):
        scene = case.scene()
        try:
            for f32 in (False, True):
                for device in (False, True):
                    clear, rec, n = _call(torch_cuda, case, scene, f32, device)
                    assert n == (0, 0) and np.all(np.isposinf(clear["min_distance"]))
                    assert np.all(clear["min_i"] == NONE) and np.all(clear["min_j"] == NONE)
                    assert not clear["n_evaluated"].any() and not clear["n_skipped"].any()
                    assert rec.tobytes() == np.repeat(model.no_record(abi, f32), case.n_conf).tobytes()
            d = pkg.engine.dll()
            req = abi.default_distance_request()
            n = (C.c_size_t * 2)(7, 7)
            assert d.hfcl_scene_nearest_self(scene._h, None, C.c_size_t(0), C.byref(req), C.c_double(np.inf), None, None, n) == abi.ERR_INVALID_ARGUMENT
            out = _poison(1, abi.SCENE_CLEARANCE_DTYPE)
            assert d.hfcl_scene_nearest_self(scene._h, None, C.c_size_t(0), C.byref(req), C.c_double(np.inf), abi.ptr(out), None, n) == 0
            assert tuple(n) == (0, 0) and out.tobytes() == _poison(1, abi.SCENE_CLEARANCE_DTYPE).tobytes()
            # refusals with a scene: nothing is written
            n = (C.c_size_t * 2)(7, 7)
            tab = np.ascontiguousarray(case.tf)
            for args, word in (((abi.ptr(tab), C.c_size_t(1), C.byref(req), C.c_double(np.inf), None, None, n), "null output"),
                               ((abi.ptr(tab), C.c_size_t(1), None, C.c_double(np.inf), abi.ptr(out), None, n), "null request"),
                               ((abi.ptr(tab), C.c_size_t(1), C.byref(req), C.c_double(np.nan), abi.ptr(out), None, n), "upper_bound")):
                assert d.hfcl_scene_nearest_self(scene._h, *args) == abi.ERR_INVALID_ARGUMENT
                assert word in pkg.engine.last_error()
            assert tuple(n) == (7, 7) and out.tobytes() == _poison(1, abi.SCENE_CLEARANCE_DTYPE).tobytes()
        finally:
            scene.close()


def test_nan_pose_and_plane(pkg, torch_cuda):
    """A NaN pose in one object of one configuration: its pairs have no bound, land in pass 1 and do not count in the fold.  A Plane
    among the objects: its unbounded box puts its pairs in pass 1."""
    L = pkg.ShapeLibrary()
    L.add_sphere(0.3)
    L.add_box(0.5, 0.4, 0.3)
    L.add_plane([0.0, 0.0, 1.0], -5.0)
    lib = pkg.Library(L)
    try:
        rng = np.random.default_rng(5)
        n, n_conf = 70, 3
        shape = rng.integers(0, 2, n).astype(np.uint32)
        shape[33] = 2
        quat = pkg.workloads.uniform_quaternions(rng, n_conf * n)
        quat.reshape(n_conf, n, 4)[:, 33] = [1.0, 0, 0, 0]
        T = rng.uniform(-4, 4, (n_conf * n, 3))
        T.reshape(n_conf, n, 3)[:, 33] = 0.0
        T.reshape(n_conf, n, 3)[1, 50] = np.nan
        tf = pkg.geometry.make_pose(quat=quat, T=T).reshape(n_conf, n, 12)
        pose = pkg.geometry.pose_f32_from_quat(quat, T).reshape(n_conf, n, 7)
        case = Case(pkg, lib, shape, tf, pose, None)
        scene = case.scene()
        try:
            for f32 in (False, True):
                for device in (False, True):
                    got = _call(torch_cuda, case, scene, f32, device)
                    assert _check(case, got, f32) == 0
                    exp = _per_conf_evaluated(case, f32)
                    assert got[2] == (len(exp["pairs1"]), len(exp["pairs2"]))
                    p1 = exp["pairs1"][int(exp["conf_begin1"][1]):int(exp["conf_begin1"][2])]
                    assert ((p1 == 50).any(axis=1)).sum() == n - 1 and ((p1 == 33).any(axis=1)).sum() == n - 1
                    assert got[0]["n_evaluated"][1] >= 2 * (n - 1) - 1 and np.all(np.isfinite(got[0]["min_distance"]))
                    assert got[0].tobytes() == exp["clearance"].tobytes()
        finally:
            scene.close()
    finally:
        lib.close()


def test_a_list_that_outgrows_its_first_buffer(pkg, torch_cuda):
    """300 boxes on one spot in one configuration: 44 850 pairs in pass 1 against a first buffer of 4 800 entries."""
    L = pkg.ShapeLibrary()
    L.add_sphere(0.3)
    lib = pkg.Library(L)
    try:
        n = 300
        tf = np.tile(pkg.geometry.make_pose(), (n, 1)).reshape(1, n, 12)
        pose = pkg.geometry.pose_f32_from_quat(np.tile([1.0, 0, 0, 0], (n, 1)), np.zeros((n, 3))).reshape(1, n, 7)
        case = Case(pkg, lib, np.zeros(n, dtype=np.uint32), tf, pose, None)
        scene = case.scene()
        try:
            for device in (False, True):
                got = _call(torch_cuda, case, scene, False, device)
                assert _check(case, got, False) == 0
                assert got[2] == (44850, 0) and (got[0]["min_i"][0], got[0]["min_j"][0]) == (0, 1) and got[0]["n_evaluated"][0] == 44850
        finally:
            scene.close()
    finally:
        lib.close()


# ---- the workspace and the scene's state -----------------------------------------------------------------------------------------------------
def test_workspace_is_shared_with_the_other_scene_calls(pkg, torch_cuda, world):
    case = world["robot"](ROBOTS[0])
    scene = case.scene()
    fresh_lib = pkg.Library(pkg.workloads.scene_robot_env(*ROBOTS[0][:3], seed=1, spread=ROBOTS[0][3])[0].lib)
    try:
        first = _call(torch_cuda, case, scene, False, False)
        between = scene.collide_self(case.tf)
        third = _call(torch_cuda, case, scene, False, False)
        assert first[0].tobytes() == third[0].tobytes() and first[1].tobytes() == third[1].tobytes() and first[2] == third[2]
        other = fresh_lib.scene(case.obj_shape, NO_PAIRS)
        try:
            other.set_groups(*case.groups)
            want = other.collide_self(case.tf)
        finally:
            other.close()
        for a, b in zip(between, want):
            assert a.tobytes() == b.tobytes()
    finally:
        scene.close()
        fresh_lib.close()


def test_call_follows_the_scenes_groups(pkg, torch_cuda, world):
    robot = world["robot"](ROBOTS[0])
    everything = Case(pkg, robot.lib, robot.obj_shape, robot.tf, robot.pose, None)
    scene = robot.lib.scene(robot.obj_shape, NO_PAIRS)
    try:
        assert _check(everything, _call(torch_cuda, everything, scene, False, False), False) == 0
        scene.set_groups(*robot.groups)
        with_groups = _call(torch_cuda, robot, scene, False, False)
        assert _check(robot, with_groups, False) == 0
        scene.clear_groups()
        without = _call(torch_cuda, everything, scene, False, False)
        assert _check(everything, without, False) == 0
        assert sum(without[2]) != sum(with_groups[2])
        got = scene.nearest_self(robot.tf)  # the binding
        assert got[0].tobytes() == without[0].tobytes() and got[1].tobytes() == without[1].tobytes() and got[2] == without[2]
    finally:
        scene.close()


def test_cpp_shim(pkg, torch_cuda, tmp_path):
    exe = str(tmp_path / "test_nearest_self_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_nearest_self", "test_nearest_self_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("same") == 4 and "DIFFERENT" not in r.stdout
