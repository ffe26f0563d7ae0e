"""A static environment kept on the device (include/hppfcl_amd_env.h) without a GPU: the exports and the refusals without a device; the
numpy model's scenes (tests/env_model.py: EnvScene) holding what they promise; the header (hpp-fcl_amd/csrc/hfcl_env.hpp) built with g++
(tests/env_harness) -- the tile-box rule against numpy bit for bit, the cells' count / scan / emit with the box and group skipping against
the model byte for byte however the call is cut, never a listed pair in a skipped cell -- and the harness's own program (a random property
check and the order check) run stand-alone; spatial_order; the workload's two forms."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import env_model
import pairs_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL32, FILL64 = 0xABABABAB, 0xABABABABABABABAB
SRC = os.path.join(ROOT, "tests", "env_harness", "env_harness.cpp")
CXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("env_harness") / "libenv_harness.so")
    subprocess.check_call(CXX + ["-fPIC", "-shared", "-o", out, SRC])
    d = C.CDLL(out)
    d.eh_env_pairs.restype = C.c_uint64
    d.eh_tile_boxes.restype = C.c_uint32
    return d


_SCENES = {}


def _scene(pkg, n_moving, n_env, n_conf):
    """Built once, shared, not modified."""
    key = (n_moving, n_env, n_conf)
    if key not in _SCENES:
        if "lib" not in _SCENES:
            _SCENES["lib"] = pairs_model.mixed_library(pkg)
        _SCENES[key] = env_model.EnvScene(pkg, _SCENES["lib"], n_moving, n_env, n_conf)
    return _SCENES[key]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings(pkg):
    pkg.engine.build_native()
    lib = pkg.engine.dll()
    e = pkg.engine
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_env.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted(e.ENV_SYMBOLS) and len(syms) == 17
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    assert not set(syms) & set(e.EXPORTED_SYMBOLS + e.CULL_SYMBOLS + e.NEAREST_SYMBOLS + e.PAIRS_SYMBOLS + e.GROUPS_SYMBOLS + e.NEAREST_SELF_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert len(re.findall(r'#include "[./]*hppfcl_amd_env\.h"', main)) == 1
    assert main.index("hppfcl_amd_nearest_self.h") < main.index("hppfcl_amd_env.h") < main.index("hppfcl_amd_pairs.h")  # (the pairs header stays last)
    assert lib.hfcl_abi_version() == 5
    for m in ("set_environment", "clear_environment", "n_moving", "environment_aabbs", "env_pairs", "env_pairs_device", "collide_env",
              "distance_env", "collide_env_pairs_device", "distance_env_pairs_device", "collide_env_pairs_device_f32",
              "distance_env_pairs_device_f32"):
        assert hasattr(e.Scene, m), m
    assert "scene_env_span" in e.option_keys()
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd.h")])


def test_entry_points_without_a_device(pkg):
    """No CPU fallback: without a device the setter and every compute entry point say so; with one, a null scene is an invalid argument.
    Nothing is written."""
    d, abi = pkg.engine.dll(), pkg.abi
    creq, dreq = abi.default_collision_request(), abi.default_distance_request()
    tf, pose = np.zeros((2, 12)), np.zeros((2, 7), dtype=np.float32)
    out = np.full(6, 7.5)
    pairs = np.full(8, FILL32, dtype=np.uint32)
    cb = np.full(2, FILL64, dtype=np.uint64)
    n = C.c_size_t(7)
    one, cap, inf = C.c_size_t(1), C.c_size_t(4), C.c_double(0.0)
    calls = [
        (d.hfcl_scene_set_environment, (None, one, abi.ptr(tf))),
        (d.hfcl_scene_set_environment_f32, (None, one, abi.ptr(pose))),
        (d.hfcl_scene_clear_environment, (None,)),
        (d.hfcl_scene_environment_aabbs, (None, abi.ptr(out), None)),
        (d.hfcl_scene_env_pairs, (None, abi.ptr(tf), one, inf, abi.ptr(pairs), cap, abi.ptr(cb), C.byref(n))),
        (d.hfcl_scene_env_pairs_f32, (None, abi.ptr(pose), one, inf, abi.ptr(pairs), cap, abi.ptr(cb), C.byref(n))),
        (d.hfcl_scene_env_pairs_device, (None, None, one, inf, None, cap, None, None, None)),
        (d.hfcl_scene_env_pairs_device_f32, (None, None, one, inf, None, cap, None, None, None)),
        (d.hfcl_scene_collide_env_pairs_device, (None, None, one, None, cap, None, C.byref(creq), None, None, None, None, None)),
        (d.hfcl_scene_distance_env_pairs_device, (None, None, one, None, cap, None, C.byref(dreq), None, None, None, None, None)),
        (d.hfcl_scene_collide_env_pairs_device_f32, (None, None, one, None, cap, None, C.byref(creq), None, None, None)),
        (d.hfcl_scene_distance_env_pairs_device_f32, (None, None, one, None, cap, None, C.byref(dreq), None, None, None)),
        (d.hfcl_scene_collide_env, (None, abi.ptr(tf), one, inf, C.byref(creq), None, cap, abi.ptr(pairs), abi.ptr(cb), None, None, None, C.byref(n))),
        (d.hfcl_scene_distance_env, (None, abi.ptr(tf), one, inf, C.byref(dreq), None, cap, abi.ptr(pairs), abi.ptr(cb), None, None, None, C.byref(n))),
        (d.hfcl_scene_collide_env_f32, (None, abi.ptr(pose), one, inf, C.byref(creq), None, cap, abi.ptr(pairs), abi.ptr(cb), None, C.byref(n))),
        (d.hfcl_scene_distance_env_f32, (None, abi.ptr(pose), one, inf, C.byref(dreq), None, cap, abi.ptr(pairs), abi.ptr(cb), None, C.byref(n))),
    ]
    assert sorted([fn.__name__ for fn, _ in calls] + ["hfcl_scene_n_moving"]) == sorted(pkg.engine.ENV_SYMBOLS)
    no_device = pkg.engine.device_count() == 0
    for fn, args in calls:
        assert fn(*args) == (abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT), fn.__name__
        assert ("no CPU fallback" if no_device else "null scene") in pkg.engine.last_error(), fn.__name__
    assert d.hfcl_scene_n_moving(None) == 0
    assert np.all(out == 7.5) and np.all(pairs == FILL32) and np.all(cb == FILL64) and n.value == 7


def test_shim_methods_compile(tmp_path):
    src = tmp_path / "shim.cpp"
    src.write_text('#include "hppfcl_amd_compat.hpp"\n'
                   "size_t use(hpp::fcl::amd::Scene& s, const std::vector<hpp::fcl::Transform3f>& env, const hpp::fcl::Transform3f* moving,\n"
                   "           const hpp::fcl::CollisionRequest& creq, const hpp::fcl::DistanceRequest& dreq) {\n"
                   "  s.setEnvironment(2, env);\n"
                   "  std::vector<uint32_t> pairs;\n"
                   "  std::vector<uint64_t> conf_begin;\n"
                   "  std::vector<hfcl_scene_summary> summaries;\n"
                   "  std::vector<hpp::fcl::CollisionResult> cres;\n"
                   "  std::vector<hpp::fcl::DistanceResult> dres;\n"
                   "  s.envPairs(moving, 3, 0.0, pairs, conf_begin);\n"
                   "  s.collideEnv(moving, 3, 0.0, creq, &cres, pairs, conf_begin, &summaries);\n"
                   "  s.distanceEnv(moving, 3, 0.0, dreq, &dres, pairs, conf_begin, nullptr);\n"
                   "  s.clearEnvironment();\n"
                   "  return pairs.size() + s.numMoving();\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src)])


# ---- the model's scenes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_conf", [3, 37])
@pytest.mark.parametrize("n_moving,n_env", env_model.SIZES)
def test_scenes_hold_what_they_promise(pkg, n_moving, n_env, n_conf):
    """Asserted on the model's output, not assumed: configuration 0 lists nothing, some configuration lists both kinds of pair, every
    environment tile has a listed pair in some configuration, some cell is skipped by box, the other configurations list between 1 % and
    30 % of the allowed pairs.  (n_conf = 1 in the GPU tests: the configurations of the three-configuration scene one by one.)"""
    es = _scene(pkg, n_moving, n_env, n_conf)
    es.check()
    # the list is the full scene's with i >= n_moving removed: nothing but the rule of the header, restated
    full, cb = pairs_model.self_pairs(es.boxes, 0.25)
    keep = full[:, 0] < n_moving
    got, got_cb = es.expected(False, 0.25)
    assert np.array_equal(got, full[keep]) and got_cb[-1] == keep.sum()
    assert np.array_equal(np.diff(got_cb.astype(np.int64)), np.bincount(pairs_model.conf_of(cb)[keep], minlength=n_conf))


# ---- the header's host build ------------------------------------------------------------------------------------------------------------
def _tile_boxes(harness, pkg, boxes):
    b = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
    out = np.full(((len(b) + 255) // 256, 6), 123.0)
    assert harness.eh_tile_boxes(pkg.abi.ptr(b) if len(b) else None, C.c_uint32(len(b)), pkg.abi.ptr(out) if len(out) else None) == len(out)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_tile_box_rule_bit_for_bit(pkg, harness):
    rng = np.random.default_rng(5)
    big = np.finfo(np.float64).max
    for n_env in (1, 255, 256, 257, 511, 513, 600):  # (a last tile of 1 object: 257, 513; of 255 objects: 255, 511)
        mid = rng.uniform(-20, 20, (n_env, 3))
        half = rng.uniform(0.0, 2.0, (n_env, 3))
        boxes = np.concatenate([mid - half, mid + half], axis=1)
        cases = {"plain": boxes}
        nan = boxes.copy()
        for k in range(6):  # a NaN in every coordinate, in different members, the first and the last one among them
            nan[(k * 97) % n_env, k] = np.nan
        nan[0, 0] = nan[n_env - 1, 5] = np.nan
        cases["nan"] = nan
        inf = boxes.copy()  # a Plane that is not aligned with an axis: +-inf and +-DBL_MAX sides, and a side that overflowed into a NaN
        inf[n_env // 2] = [-np.inf, -np.inf, -big, np.inf, big, np.inf]
        inf[n_env - 1] = [-np.inf, np.nan, -big, np.inf, np.nan, big]
        cases["inf"] = inf
        zeros = boxes.copy()  # signed zeros: the fold keeps the first of two equal values
        zeros[:, 0], zeros[:, 3] = np.where(np.arange(n_env) % 2, 0.0, -0.0), np.where(np.arange(n_env) % 2, -0.0, 0.0)
        cases["zeros"] = zeros
        for name, b in cases.items():
            got, want = _tile_boxes(harness, pkg, b), env_model.tile_boxes(b)
            assert _bits(got) == _bits(want), (n_env, name)
            for t in range(len(want)):  # ... and tile by tile, the fold written as a loop over the members
                assert _bits(want[t]) == _bits(env_model.fold_boxes(b[t * 256:(t + 1) * 256])), (n_env, name, t)
        tiles = env_model.tile_boxes(nan)
        assert tiles[0, 0] == -np.inf and tiles[-1, 5] == np.inf
        with np.errstate(invalid="ignore"):  # numpy's own min / max where no NaN is about
            want = np.stack([np.concatenate([boxes[t:t + 256, :3].min(axis=0), boxes[t:t + 256, 3:].max(axis=0)]) for t in range(0, n_env, 256)])
        assert np.array_equal(env_model.tile_boxes(boxes), want)


def _harness_list(harness, pkg, es, f32, inflate, chunk, span, n_cus, groups=None, capacity=None):
    boxes = es.boxes32 if f32 else es.boxes
    nm, ne, n_conf = es.n_moving, es.n_env, es.n_conf
    moving = np.ascontiguousarray(boxes[:, :nm])
    env = np.ascontiguousarray(boxes[0, nm:])
    assert _bits(np.broadcast_to(env, (n_conf,) + env.shape)) == _bits(boxes[:, nm:])  # (the environment stands still)
    exp, exp_cb = es.expected(f32, inflate, groups)
    capacity = len(exp) if capacity is None else capacity
    pairs = np.full((capacity + 4, 2), FILL32, dtype=np.uint32)
    cb = np.full(n_conf + 1, FILL64, dtype=np.uint64)
    stats = np.zeros(4, dtype=np.uint64)
    geometry = np.zeros(2, dtype=np.uint32)
    group, words = (groups[1], groups[2]) if groups else (None, None)
    n = harness.eh_env_pairs(pkg.abi.ptr(moving) if moving.size else None, C.c_uint32(nm), pkg.abi.ptr(env) if env.size else None, C.c_uint32(ne),
                             C.c_uint64(n_conf), C.c_double(inflate), C.c_uint64(chunk), C.c_uint32(span), C.c_uint32(n_cus),
                             pkg.abi.ptr(group) if groups else None, C.c_uint32(len(words) if groups else 0), pkg.abi.ptr(words) if groups else None,
                             pkg.abi.ptr(pairs), C.c_uint64(capacity), pkg.abi.ptr(cb), pkg.abi.ptr(stats), pkg.abi.ptr(geometry))
    return n, pairs, cb, stats, geometry, exp, exp_cb


@pytest.mark.parametrize("n_moving,n_env", env_model.SIZES)
def test_cells_equal_the_model(pkg, harness, n_moving, n_env):
    """The cells' count / scan / emit, whole and in chunks, span lengths 1, 2, all and automatic (256 compute units), both precisions' boxes
    and both inflates, equal the model byte for byte; nothing is written behind the capacity; and -- exhaustively, on every cell these
    scenes skip by its box -- no skipped cell holds a listed pair, while the model's own count of skipped cells is the harness's."""
    for n_conf in (3, 37) if (n_moving, n_env) in ((17, 257), (130, 513)) else (3,):
        es = _scene(pkg, n_moving, n_env, n_conf)
        for f32, inflate in ((False, 0.0), (True, 0.25), (False, 0.25)):
            model_skipped, _, _ = env_model.skipped_by_box(es.boxes32 if f32 else es.boxes, n_moving, inflate)
            for chunk in (7, 64, 0):
                for span, n_cus in ((1, 0), (2, 0), (0, 0), (0, 256)):
                    n, pairs, cb, stats, geometry, exp, exp_cb = _harness_list(harness, pkg, es, f32, inflate, chunk, span, n_cus)
                    what = (n_moving, n_env, n_conf, f32, inflate, chunk, span, n_cus)
                    assert n == len(exp), what
                    assert pairs[:n].tobytes() == exp.tobytes() and cb.tobytes() == exp_cb.tobytes(), what
                    assert np.all(pairs[n:] == FILL32), what
                    assert stats[3] == 0, what  # never skips a listed pair
                    assert stats[0] == model_skipped.sum() and stats[1] == n_conf * ((n_moving + 15) // 16) * ((n_env + 255) // 256), what
                    if span:
                        assert geometry[0] == min(span, max((n_moving + 255) // 256 + (n_env + 255) // 256, 1)), what
        # a capacity one short: the true count, nothing at or past the capacity
        n, pairs, cb, _, _, exp, exp_cb = _harness_list(harness, pkg, es, False, 0.0, 0, 1, 0, capacity=max(len(es.expected()[0]) - 1, 0))
        assert n == len(exp) and cb.tobytes() == exp_cb.tobytes()
        assert pairs[:max(n - 1, 0)].tobytes() == exp[:max(n - 1, 0)].tobytes() and np.all(pairs[max(n - 1, 0):] == FILL32)


@pytest.mark.parametrize("n_moving,n_env", [(5, 255), (17, 257), (63, 600)])
def test_cells_with_groups_equal_the_model(pkg, harness, n_moving, n_env):
    """scene_robot_env's groups (neighbours excluded, the obstacles one group), and a matrix of all ones, which is no groups."""
    es = _scene(pkg, n_moving, n_env, 3)
    robot = ("robot",) + env_model.robot_groups(n_moving, es.n)
    ones = ("ones", np.random.default_rng(1).integers(0, 8, es.n).astype(np.uint8), np.full(8, 0xFF, dtype=np.uint64))
    assert es.expected(False, 0.0, ones)[0].tobytes() == es.expected(False, 0.0)[0].tobytes()
    exp = es.expected(False, 0.0, robot)[0]
    assert 0 < len(exp) <= len(es.expected()[0]) and not np.any((exp[:, 1] == exp[:, 0] + 1) & (exp[:, 1] < n_moving))
    if n_moving == 63:  # (enough links for neighbours that touch: the groups take something away)
        assert len(exp) < len(es.expected()[0])
    for groups in (robot, ones):
        for chunk, span in ((7, 1), (0, 2), (0, 0)):
            n, pairs, cb, stats, _, exp, exp_cb = _harness_list(harness, pkg, es, False, 0.25, chunk, span, 0, groups)
            assert n == len(exp) and pairs[:n].tobytes() == exp.tobytes() and cb.tobytes() == exp_cb.tobytes(), (groups[0], chunk, span)
            assert stats[3] == 0


def test_harness_program_stand_alone(tmp_path):
    """The harness's own main: never-skips-a-listed-pair on 10^4 random boxes (NaN, +-inf and unbounded sides among them, inflate 0 and
    0.25), and cell geometry plus the row-major scan against the rule written as three loops, span lengths 1, 2 and all."""
    exe = str(tmp_path / "env_harness")
    subprocess.check_call(CXX + ["-o", exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "env_harness: ok" in run.stdout, run.stdout + run.stderr
    assert re.search(r"property check: 1\d{4} boxes, [1-9]\d* cells skipped", run.stdout), run.stdout


# ---- the upper layers -----------------------------------------------------------------------------------------------------------------
def test_spatial_order(pkg):
    rng = np.random.default_rng(2)
    pts = rng.uniform(-5, 5, (4096, 3))
    order = pkg.engine.spatial_order(pts)
    assert sorted(order.tolist()) == list(range(4096))
    assert np.array_equal(order, pkg.engine.spatial_order(pts))

    def tile_volume(p):
        t = p.reshape(-1, 256, 3)
        return np.prod(t.max(axis=1) - t.min(axis=1), axis=1).mean()
    assert tile_volume(pts[order]) < 0.2 * tile_volume(pts)  # (16 tiles of neighbours against 16 tiles that each span the whole box)
    assert pkg.engine.spatial_order(np.zeros((0, 3))).shape == (0,)
    assert pkg.engine.spatial_order(np.ones((5, 3))).tolist() == [0, 1, 2, 3, 4]  # (ties by index)


def test_workload_returns_both_forms(pkg):
    wl = pkg.workloads
    ps, groups, P = wl.scene_robot_env(4, 6, 300, seed=2)
    for order in (False, True):
        sc, groups2, P2, (moving_tf, env_tf), (moving_pose, env_pose) = wl.scene_robot_env(4, 6, 300, seed=2, split=True, spatial=order)
        assert moving_tf.shape == (4, 6, 12) and env_tf.shape == (300, 12) and moving_pose.shape == (4, 6, 7) and env_pose.shape == (300, 7)
        assert moving_tf.dtype == np.float64 and env_pose.dtype == np.float32
        assert env_model.full_table(moving_tf, env_tf).tobytes() == np.ascontiguousarray(sc.obj_tf).tobytes()
        assert env_model.full_table(moving_pose, env_pose).tobytes() == np.ascontiguousarray(sc.obj_pose_f32).tobytes()
        assert np.array_equal(groups2[0], groups[0]) and np.array_equal(groups2[1], groups[1]) and np.array_equal(P2, P)
        if not order:
            assert sc.obj_tf.tobytes() == ps.obj_tf.tobytes() and np.array_equal(sc.obj_shape, ps.obj_shape)
        else:  # the same obstacles, permuted: by Morton code of their centres
            perm = pkg.engine.spatial_order(ps.T[0, 6:])
            assert np.array_equal(sc.obj_shape[6:], ps.obj_shape[6:][perm]) and np.array_equal(sc.T[:, 6:], ps.T[:, 6:][:, perm])
            assert np.array_equal(sc.obj_shape[:6], ps.obj_shape[:6])
