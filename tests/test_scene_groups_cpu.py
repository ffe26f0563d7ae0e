"""Object groups and a group matrix on the device-made pair lists (include/hppfcl_amd_groups.h) without a GPU: the exports and the
refusals without a device; the numpy model (tests/groups_model.py) of two managers against the host broadphase
(hfcl_broadphase_pairs_between) entry for entry; the header (hpp-fcl_amd/csrc/hfcl_pairs.hpp) built with g++ (tests/groups_harness) -- both
group kernels' count / scan / emit with the tile and block skipping, however the call is cut -- against the model byte for byte for every
layout; the argument helpers; and workloads.scene_robot_env."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import groups_model
import pairs_model
from test_scene_pairs_cpu import SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL32, FILL64 = 0xABABABAB, 0xABABABABABABABAB
CHUNKINGS = ((0, 64), (40, 64), (1, 64), (0, 0), (40, 0))  # (option scene_cull_chunk, option scene_pairs_small_max)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("groups_harness") / "libgroups_harness.so")
    src = os.path.join(ROOT, "tests", "groups_harness", "groups_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-o", out, src])
    d = C.CDLL(out)
    d.gh_self_pairs.restype = C.c_uint64
    d.gh_tile_words.restype = C.c_uint32
    return d


_SCENES = {}


def _scene(pkg, n_objects, n_conf):
    """Built once, shared, not modified."""
    key = (n_objects, n_conf)
    if key not in _SCENES:
        if "lib" not in _SCENES:
            _SCENES["lib"] = pairs_model.mixed_library(pkg)
        _SCENES[key] = pairs_model.PairScene(pkg, _SCENES["lib"], n_objects, n_conf)
    return _SCENES[key]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings(pkg):
    pkg.engine.build_native()
    lib = pkg.engine.dll()
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_groups.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted(pkg.engine.GROUPS_SYMBOLS) == ["hfcl_scene_clear_groups", "hfcl_scene_num_groups", "hfcl_scene_set_groups"]
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    e = pkg.engine
    assert not set(syms) & set(e.EXPORTED_SYMBOLS + e.CULL_SYMBOLS + e.NEAREST_SYMBOLS + e.PAIRS_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    includes = re.findall(r'#include "(hppfcl_amd_[a-z]+\.h)"', main)
    assert includes == ["hppfcl_amd_cull.h", "hppfcl_amd_nearest.h", "hppfcl_amd_groups.h", "hppfcl_amd_pairs.h"]
    assert lib.hfcl_abi_version() == 5
    for m in ("set_groups", "clear_groups", "n_groups"):
        assert hasattr(pkg.engine.Scene, m), m
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd.h")])


def test_entry_points_without_a_device(pkg):
    """No CPU fallback: without a device every entry point says so; with one, a null scene is an invalid argument.  Nothing is written."""
    d, abi = pkg.engine.dll(), pkg.abi
    group = np.full(4, 0xAB, dtype=np.uint8)
    words = np.full(2, FILL64, dtype=np.uint64)
    calls = [
        (d.hfcl_scene_set_groups, (None, abi.ptr(group), C.c_size_t(2), abi.ptr(words))),
        (d.hfcl_scene_clear_groups, (None,)),
    ]
    assert sorted([fn.__name__ for fn, _ in calls] + ["hfcl_scene_num_groups"]) == sorted(pkg.engine.GROUPS_SYMBOLS)
    no_device = pkg.engine.device_count() == 0
    for fn, args in calls:
        assert fn(*args) == (abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT), fn.__name__
        assert ("no CPU fallback" if no_device else "null scene") in pkg.engine.last_error(), fn.__name__
    assert d.hfcl_scene_num_groups(None) == 0
    assert np.all(group == 0xAB) and np.all(words == FILL64)


def test_shim_methods_compile(tmp_path):
    src = tmp_path / "shim.cpp"
    src.write_text('#include "hppfcl_amd_compat.hpp"\n'
                   "size_t use(hpp::fcl::amd::Scene& s, const std::vector<uint8_t>& g, const std::vector<uint64_t>& w) { s.setGroups(g, w); "
                   "s.clearGroups(); return s.numGroups(); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_argument_helpers(pkg):
    e = pkg.engine
    g, w = e.groups_between(3, 4)
    mg, mw = groups_model.between(3, 7)
    assert g.dtype == np.uint8 and w.dtype == np.uint64 and g.tobytes() == mg.tobytes() and w.tobytes() == mw.tobytes()
    g, w = e.groups_excluding(9, [(k, k + 1) for k in range(8)])
    mg, mw = groups_model.chain(9)
    assert g.tobytes() == mg.tobytes() and w.tobytes() == mw.tobytes()
    g, w = e.groups_excluding(64, np.zeros((0, 2), dtype=np.int64))
    assert w[63] == np.uint64(0x7FFFFFFFFFFFFFFF) and w[0] == np.uint64(0xFFFFFFFFFFFFFFFE)
    m = np.random.default_rng(1).random((64, 64)) < 0.5
    assert e.group_words(m).tobytes() == groups_model.words_of(m).tobytes()
    assert np.array_equal(groups_model.matrix_of(e.group_words(m)), m)
    assert e.group_words(np.array([2, 1], dtype=np.uint64)).tobytes() == np.array([2, 1], dtype=np.uint64).tobytes()
    for bad in (np.ones((65, 65), dtype=bool), np.ones((2, 3), dtype=bool), np.ones((2, 2, 2), dtype=bool)):
        with pytest.raises(ValueError):
            e.group_words(bad)
    with pytest.raises(ValueError):
        e.groups_excluding(65, [])
    fcl = pkg.compat
    objs = [fcl.CollisionObject(fcl.Sphere(0.5), fcl.Transform3f()) for _ in range(3)]
    for kw in (dict(broadphase=True), dict(broadphase=False)):
        with pytest.raises(ValueError) as err:
            fcl.collide_scene(objs, [(0, 1)], fcl.CollisionRequest(), groups=e.groups_between(1, 2), **kw)
        assert 'broadphase="self"' in str(err.value)
        with pytest.raises(ValueError) as err:
            fcl.distance_scene(objs, [(0, 1)], fcl.DistanceRequest(), groups=e.groups_between(1, 2), **kw)
        assert 'broadphase="self"' in str(err.value)
    with pytest.raises(ValueError) as err:
        fcl.distance_scene(objs, [(0, 1)], fcl.DistanceRequest(), nearest=True, groups=e.groups_between(1, 2))
    assert 'broadphase="self"' in str(err.value)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_objects", sorted({n for n, _ in SIZES[2:]}))
def test_layouts_keep_their_promises(n_objects):
    names = []
    for seed in (0, 1, 2):
        for name, group, words in groups_model.layouts(n_objects, seed):
            groups_model.check_layout(name, group, words)
            names.append(name)
            assert group.dtype == np.uint8 and words.dtype == np.uint64 and len(group) == n_objects
    assert {"a:1", "a:%d" % (n_objects - 1), "c:8", "c:64", "d", "e"} <= set(names)
    assert ("b" in names) == (n_objects <= 64) and ("f" in names) == ("g" in names) == (n_objects == 600)
    if n_objects > 17:
        assert {"a:16", "a:17"} <= set(names)


@pytest.mark.parametrize("n_objects,n_conf", [(5, 37), (64, 3), (65, 3), (130, 3), (600, 3)])
def test_two_managers_equal_the_host_broadphase(pkg, n_objects, n_conf):
    """Layout (a) on the model's boxes is hfcl_broadphase_pairs_between(boxes[:n_a], boxes[n_a:]) with n_a added to every j, entry for
    entry; the configuration with every pair touching has n_a * (n - n_a) entries."""
    sc = _scene(pkg, n_objects, n_conf)
    sc.check_shares()
    pairs, cb = sc.expected()
    tested = 0
    for name, group, words in groups_model.layouts(n_objects):
        if not name.startswith("a:"):
            continue
        n_a = int(name[2:])
        mine, mcb = groups_model.filter_list(pairs, cb, group, words)
        assert mcb[2] - mcb[1] == n_a * (n_objects - n_a) == groups_model.n_allowed(group, words) and mcb[1] == 0
        for c in range(n_conf):
            host = pkg.engine.broadphase_pairs_between(sc.boxes[c, :n_a], sc.boxes[c, n_a:]).astype(np.uint32)
            host[:, 1] += n_a
            assert mine[int(mcb[c]):int(mcb[c + 1])].tobytes() == host.tobytes(), (name, c)
        tested += 1
    assert tested == (2 if n_objects == 5 else 4)


# ---- the header -------------------------------------------------------------------------------------------------------------------------
def _header_pairs(harness, pkg, boxes, inflate, group, words, chunk_rows=0, small_max=64, capacity=None, count_only=False):
    n_conf, n = boxes.shape[:2]
    cap = max(n_conf * n * (n - 1) // 2, 1) if capacity is None else capacity
    pairs = np.full((max(cap, 1) + 3, 2), FILL32, dtype=np.uint32)  # (three guard entries)
    cb = np.full(n_conf + 1, FILL64, dtype=np.uint64)
    stats = np.zeros(4, dtype=np.uint64)
    b = np.ascontiguousarray(boxes)
    got = harness.gh_self_pairs(pkg.abi.ptr(b), C.c_uint32(n), C.c_uint64(n_conf), C.c_double(inflate), C.c_uint64(chunk_rows), C.c_uint32(small_max),
                                pkg.abi.ptr(group), C.c_uint32(len(words)), pkg.abi.ptr(words), None if count_only else pkg.abi.ptr(pairs),
                                C.c_uint64(cap), pkg.abi.ptr(cb), pkg.abi.ptr(stats))
    return pairs, cb, int(got), [int(x) for x in stats]


@pytest.mark.parametrize("n_objects,n_conf", SIZES[2:])
def test_header_list_equals_the_model(pkg, harness, n_objects, n_conf):
    sc = _scene(pkg, n_objects, n_conf)
    all_pairs = n_objects * (n_objects - 1) // 2
    for name, group, words in groups_model.layouts(n_objects):
        groups_model.check_layout(name, group, words)
        allowed = groups_model.n_allowed(group, words)
        assert allowed == {"d": all_pairs, "e": 0}.get(name, allowed)
        model_skips = groups_model.skipped(group, words)
        for f32, inflate in ((False, 0.0), (False, 0.25), (True, 0.0), (True, 0.25)):
            base, base_cb = sc.expected(f32, inflate)
            exp, exp_cb = groups_model.filter_list(base, base_cb, group, words)
            assert exp_cb[1] == 0 and exp_cb[2] - exp_cb[1] == allowed, name  # (no pair touches, every pair touches)
            if name == "d":
                assert exp.tobytes() == base.tobytes() and exp_cb.tobytes() == base_cb.tobytes()
            if name == "e":
                assert len(exp) == 0 and not exp_cb.any()
            boxes = sc.boxes32 if f32 else sc.boxes
            for chunk_rows, small_max in CHUNKINGS:
                what = (name, f32, inflate, chunk_rows, small_max)
                pairs, cb, n, stats = _header_pairs(harness, pkg, boxes, inflate, group, words, chunk_rows, small_max)
                assert n == len(exp), what
                assert pairs[:n].tobytes() == exp.tobytes() and cb.tobytes() == exp_cb.tobytes(), what
                assert np.all(pairs[n:] == FILL32), what
                if n_objects > small_max:  # the tiled form: what it skipped is what the tables say, in every configuration
                    assert stats == [n_conf * x for x in model_skips], what
                    if name == "f":
                        assert stats[0] > 0 and 0 < stats[2] < stats[3], what
                    if name == "g":
                        assert stats[0] == 0 and stats[2] == 0, what
                    if name == "e":
                        assert stats[0] == stats[1] and stats[2] == stats[3], what
                    if name == "d":
                        assert stats[0] == 0 and stats[2] == 0, what
        # count only; a capacity of half the count: the count is true, the entries below the capacity right, nothing written past it
        exp, exp_cb = groups_model.filter_list(*sc.expected(False, 0.25), group, words)
        for chunk_rows, small_max in ((40, 64), (40, 0)):
            pairs, cb, n, _ = _header_pairs(harness, pkg, sc.boxes, 0.25, group, words, chunk_rows, small_max, count_only=True)
            assert n == len(exp) and cb.tobytes() == exp_cb.tobytes() and np.all(pairs == FILL32), name
            cap = len(exp) // 2
            pairs, cb, n, _ = _header_pairs(harness, pkg, sc.boxes, 0.25, group, words, chunk_rows, small_max, capacity=cap)
            assert n == len(exp) and pairs[:cap].tobytes() == exp[:cap].tobytes() and np.all(pairs[cap:] == FILL32), name
            assert cb.tobytes() == exp_cb.tobytes(), name


def test_sorted_and_shuffled_groups_skip_differently(pkg, harness):
    """(f) and (g) share the matrix; sorted, the middle tile is skipped by every row block of group 0 and every row block of group 1
    leaves at once; shuffled, nothing can be skipped.  Either way the list is the model's."""
    sc = _scene(pkg, 600, 3)
    (gf, wf), (gg, wg) = groups_model.sorted_600(), groups_model.shuffled_600()
    assert wf.tobytes() == wg.tobytes() and sorted(gf) == sorted(gg)
    skips, tiles, early, blocks = groups_model.skipped(gf, wf)
    # rows 0..255: 16 blocks look at tiles 0 1 2 and skip tile 1; rows 256..511: 16 blocks leave (tiles 1 2 unseen); rows 512..599: 6
    # blocks look at tile 2
    assert (skips, tiles, early, blocks) == (16 + 2 * 16, 3 * 16 + 2 * 16 + 6, 16, 38)
    assert groups_model.skipped(gg, wg) == (0, tiles, 0, 38)
    words = np.zeros(3, dtype=np.uint64)
    assert harness.gh_tile_words(pkg.abi.ptr(gf), C.c_uint32(600), pkg.abi.ptr(words)) == 3
    assert list(words) == [1, 2, 1] and words.tobytes() == groups_model.tile_words(gf).tobytes()
    assert harness.gh_tile_words(pkg.abi.ptr(gg), C.c_uint32(600), pkg.abi.ptr(words)) == 3 and list(words) == [3, 3, 3]
    base, base_cb = sc.expected(False, 0.0)
    for group, w in ((gf, wf), (gg, wg)):
        exp, exp_cb = groups_model.filter_list(base, base_cb, group, w)
        pairs, cb, n, stats = _header_pairs(harness, pkg, sc.boxes, 0.0, group, w)
        assert n == len(exp) > 0 and pairs[:n].tobytes() == exp.tobytes() and cb.tobytes() == exp_cb.tobytes()
        assert stats == [3 * x for x in groups_model.skipped(group, w)]


# ---- the workload -----------------------------------------------------------------------------------------------------------------------
def test_scene_robot_env(pkg):
    n_conf, n_links, n_obstacles = 37, 8, 40
    sc, (group, words), pairs = pkg.workloads.scene_robot_env(n_conf, n_links, n_obstacles)
    n = n_links + n_obstacles
    assert sc.obj_tf.shape == (n_conf, n, 12) and sc.obj_pose_f32.shape == (n_conf, n, 7) and len(sc.obj_shape) == n
    assert group.dtype == np.uint8 and list(group[:n_links]) == list(range(n_links)) and np.all(group[n_links:] == n_links)
    assert words.dtype == np.uint64 and len(words) == n_links + 1
    m = groups_model.matrix_of(words)
    assert np.array_equal(m, m.T) and not m[n_links, n_links] and m[:n_links, n_links].all()
    assert all(m[a, b] == (abs(a - b) >= 2) for a in range(n_links) for b in range(n_links))
    # the explicit list: the allowed pairs in (i, j) lexicographic order
    i, j = np.triu_indices(n, 1)
    keep = groups_model.allowed(group, words, i, j)
    exp = np.stack([i[keep], j[keep]], axis=1).astype(np.uint32)
    assert pairs.dtype == np.uint32 and pairs.tobytes() == exp.tobytes() and sc.pairs is pairs
    assert len(pairs) == (n_links - 1) * (n_links - 2) // 2 + n_links * n_obstacles
    # the obstacles do not move, the links do
    assert np.all(sc.T[:, n_links:] == sc.T[:1, n_links:]) and np.all(sc.quat[:, n_links:] == sc.quat[:1, n_links:])
    assert not np.all(sc.T[:, 1:n_links] == sc.T[:1, 1:n_links])
    # some configuration has a link-obstacle pair whose boxes touch, some configuration has none
    boxes = np.stack([pkg.engine.world_aabbs(sc.lib, sc.obj_shape, sc.obj_tf[c]) for c in range(n_conf)])
    listed, cb = groups_model.self_pairs(boxes, 0.0, group, words)
    conf = pairs_model.conf_of(cb)
    with_obstacle = np.bincount(conf[listed[:, 1] >= n_links], minlength=n_conf)
    assert with_obstacle.max() > 0 and with_obstacle.min() == 0, with_obstacle
    assert 0 < len(listed) < n_conf * len(pairs)
    with pytest.raises(ValueError):
        pkg.workloads.scene_robot_env(2, 64, 4)
