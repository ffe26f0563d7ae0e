"""The per-configuration minimum distance with box-bound pruning on the GPU (include/hppfcl_amd_nearest.h).  The yardsticks: the unculled
scene call (min_distance / min_pair of its summaries and its records, byte for byte) and the numpy model of tests/nearest_model.py (held
against the definition and the g++ build of the header in tests/test_scene_nearest_cpu.py) fed with the GPU's own boxes and unculled
records: the whole summary and the two counts of evaluated queries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nearest_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _same(a, b, what):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def _raw_distance(pkg, scene, table, req, f32=False):
    """The unculled host call: (rc, records, summaries) -- the return code is kept (HFCL_ERR_UNSUPPORTED_PAIR leaves everything complete)."""
    abi = pkg.abi
    tab = np.ascontiguousarray(table)
    n_conf = len(tab)
    out = np.zeros(n_conf * scene.n_pairs, dtype=abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE)
    summ = np.zeros(n_conf, dtype=abi.SCENE_SUMMARY_DTYPE)
    d = pkg.engine.dll()
    if f32:
        rc = d.hfcl_scene_distance_f32(scene._h, abi.ptr(tab), C.c_size_t(n_conf), C.byref(req), abi.ptr(out), abi.ptr(summ))
    else:
        rc = d.hfcl_scene_distance(scene._h, abi.ptr(tab), C.c_size_t(n_conf), C.byref(req), abi.ptr(out), abi.ptr(summ), None, None)
    return rc, out, summ


def _raw_nearest(pkg, scene, table, req, D=np.inf, f32=False, records=True):
    abi = pkg.abi
    tab = np.ascontiguousarray(table)
    n_conf = len(tab)
    summ = np.full(n_conf, 0x5A, dtype=np.uint8).repeat(24).view(abi.SCENE_SUMMARY_DTYPE)  # (every summary must be written)
    dt = abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE
    rec = np.full(n_conf, 0x5A, dtype=np.uint8).repeat(dt.itemsize).view(dt) if records else None
    n = (C.c_size_t * 2)(99, 99)
    fn = pkg.engine.dll().hfcl_scene_nearest_f32 if f32 else pkg.engine.dll().hfcl_scene_nearest
    rc = fn(scene._h, abi.ptr(tab), C.c_size_t(n_conf), C.byref(req), C.c_double(D), abi.ptr(summ), abi.ptr(rec), n)
    return rc, summ, rec, (int(n[0]), int(n[1]))


def _device_nearest(torch, pkg, scene, table, req, D=np.inf, f32=False):
    abi = pkg.abi
    dev = torch.device("cuda:0")
    n_conf = len(table)
    d_tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    d_sum = torch.full((n_conf * 6,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    d_rec = torch.full((n_conf * (11 if f32 else 24),), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    fn = scene.nearest_device_f32 if f32 else scene.nearest_device
    n = fn(d_tab, n_conf, req, d_sum, d_rec, upper_bound=D, stream=_stream(torch))
    torch.cuda.synchronize()
    return d_sum.cpu().numpy().view(abi.SCENE_SUMMARY_DTYPE), d_rec.cpu().numpy().view(abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE), n


def _expected_min_records(pkg, full_rec, summ, n_pairs):
    """Record c * n_pairs + min_pair of the unculled records; the "no record" record where there is no min_pair."""
    out = np.zeros(len(summ), dtype=full_rec.dtype)
    for c, mp in enumerate(summ["min_pair"]):
        if mp != NONE:
            out[c] = full_rec[c * n_pairs + int(mp)]
        else:
            out[c]["distance"] = np.inf
            out[c]["status"] = 0x80000000
            if "b1" in full_rec.dtype.names:
                out[c]["b1"] = out[c]["b2"] = -1
                for k in ("normal", "p1", "p2"):
                    out[c][k] = np.nan
    return out


def _check(pkg, scene, table, req, full, D=np.inf, f32=False, got=None):
    """One nearest call against the unculled call `full` = (rc, records, summaries) and the model.  Returns (rc, summaries, min records, counts)."""
    abi = pkg.abi
    n_pairs = scene.n_pairs
    _, full_rec, full_summ = full
    rc, summ, rec, n = got if got is not None else _raw_nearest(pkg, scene, table, req, D, f32)
    boxes = scene.world_aabbs(table)
    L = nearest_model.query_bounds(boxes, scene_pairs(scene), nearest_model.R32 if f32 else nearest_model.R64)
    sel = nearest_model.select(abi, L, full_rec, D)
    _same(summ, sel["summary"], "the summaries are the model's fold over the evaluated records")
    nearest_model.check_against_full(summ, full_summ, D)
    assert n == (len(sel["ids1"]), len(sel["ids2"])), (n, len(sel["ids1"]), len(sel["ids2"]))
    if rec is not None:
        _same(rec, _expected_min_records(pkg, full_rec, summ, n_pairs), "min records")
    return rc, summ, rec, n


def _fp32_excess(scene, pose, full_rec, what):
    """What the fp32 rounding term r of the bound has to cover: the largest (lb - d_f32) / M over the queries with separated boxes, against
    the records of the unculled fp32 call.  The constant (hfcl_nearest.hpp: NEAREST_R32) is 16 x the largest value seen, rounded up to a
    power of two."""
    boxes = scene.world_aabbs(pose)
    pairs = scene_pairs(scene)
    lb, _, M = nearest_model.raw_bound(boxes[:, pairs[:, 0]], boxes[:, pairs[:, 1]])
    ok = (np.isfinite(lb) & (lb > 0)).reshape(-1) & ((full_rec["status"] >> 31) == 0)
    excess = ((lb.reshape(-1) - full_rec["distance"].astype(np.float64)) / M.reshape(-1))[ok]
    print("fp32, %s: largest (lb - d_f32) / M = %.3g = 2^%.2f over %d queries with separated boxes" % (
        what, excess.max(), np.log2(max(excess.max(), 1e-300)), ok.sum()))
    return float(excess.max())


_PAIRS = {}


def scene_pairs(scene):
    return _PAIRS[id(scene)]


def _make(pkg, L, obj_shape, pairs, meshes=()):
    lib = pkg.Library(L)
    for m in meshes:
        lib.add_bvh(m)
    scene = lib.scene(obj_shape, pairs)
    _PAIRS[id(scene)] = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    return lib, scene


@pytest.fixture(scope="module")
def planner(pkg, torch_cuda):
    """scene_planner(64, 16): 6 720 queries.  Its library and scene and the unculled distance call in both precisions, computed once."""
    ps = pkg.workloads.scene_planner(64, 16, seed=1)
    lib, scene = _make(pkg, ps.lib, ps.obj_shape, ps.pairs)
    req = pkg.abi.default_distance_request()
    d = dict(ps=ps, lib=lib, scene=scene, tf=ps.obj_tf, pose=ps.obj_pose_f32, req=req)
    d["full"] = {False: _raw_distance(pkg, scene, d["tf"], req), True: _raw_distance(pkg, scene, d["pose"], req, f32=True)}
    assert d["full"][False][0] == 0 and d["full"][True][0] == 0
    yield d
    scene.close()
    lib.close()


# ---- a. the fp64 host form ---------------------------------------------------------------------------------------------------------
def test_host_form_equals_the_unculled_call(pkg, torch_cuda, planner):
    sc, tf, req = planner["scene"], planner["tf"], planner["req"]
    _, full_rec, _ = planner["full"][False]
    only = sc.distance(tf, req, records=False)  # (the call nearest replaces: summaries only)
    rc, summ, rec, n = _check(pkg, sc, tf, req, planner["full"][False])
    assert rc == 0
    _same(summ["min_distance"], only["min_distance"], "min_distance")
    _same(summ["min_pair"], only["min_pair"], "min_pair")
    for c in range(64):
        assert rec[c].tobytes() == full_rec[c * 105 + int(summ["min_pair"][c])].tobytes(), c
    total = 64 * 105
    print("scene_planner(64, 16): %d + %d of %d queries evaluated (%.2f %%)" % (n[0], n[1], total, 100.0 * sum(n) / total))
    assert sum(n) < 0.25 * total
    # the Python front end, with and without min records
    s2, r2, n2 = sc.nearest(tf, req)
    _same(s2, summ, "Scene.nearest summaries")
    _same(r2, rec, "Scene.nearest min records")
    s3, r3, n3 = sc.nearest(tf, records=False)
    assert r3 is None and n2 == n3 == n
    _same(s3, summ, "Scene.nearest without min records")


# ---- b. chunking and determinism ---------------------------------------------------------------------------------------------------
def test_chunks_do_not_change_a_byte(pkg, torch_cuda, planner):
    sc, lib, tf, req = planner["scene"], planner["lib"], planner["tf"], planner["req"]
    base = _raw_nearest(pkg, sc, tf, req)
    try:
        for scene_chunk, cull_chunk in ((512, 256), (50, 1000), (7, 63)):
            lib.set_option("scene_chunk", scene_chunk)
            lib.set_option("scene_cull_chunk", cull_chunk)
            for again in range(2):
                rc, summ, rec, n = _raw_nearest(pkg, sc, tf, req)
                what = "scene_chunk %d, scene_cull_chunk %d, call %d" % (scene_chunk, cull_chunk, again)
                assert rc == 0 and n == base[3], what
                _same(summ, base[1], "summaries: " + what)
                _same(rec, base[2], "min records: " + what)
        _check(pkg, sc, tf, req, planner["full"][False])  # (still in chunks of 7 and 63)
    finally:
        lib.set_option("scene_chunk", 0)
        lib.set_option("scene_cull_chunk", 0)


# ---- c. the device form --------------------------------------------------------------------------------------------------------------
def test_device_form_equals_the_host_form(pkg, torch_cuda, planner):
    sc, tf, req = planner["scene"], planner["tf"], planner["req"]
    rc, summ, rec, n = _raw_nearest(pkg, sc, tf, req)
    d_summ, d_rec, d_n = _device_nearest(torch_cuda, pkg, sc, tf, req)
    assert d_n == n
    _same(d_summ, summ, "device form summaries")
    _same(d_rec, rec, "device form min records")
    # without min records, on a table that is not 16-byte aligned
    torch = torch_cuda
    d_tab = torch.zeros(64 * 16 * 12 + 1, dtype=torch.float64, device="cuda:0")
    d_tab[1:] = torch.from_numpy(tf.reshape(-1)).to("cuda:0")
    d_sum = torch.full((64 * 6,), 0x7F7F7F7F, dtype=torch.int32, device="cuda:0")
    assert sc.nearest_device(d_tab[1:], 64, req, d_sum, None, stream=_stream(torch)) == n
    torch.cuda.synchronize()
    _same(d_sum.cpu().numpy().view(pkg.abi.SCENE_SUMMARY_DTYPE), summ, "device form, summaries only")


# ---- d. the fp32 forms ---------------------------------------------------------------------------------------------------------------
def test_fp32_forms_equal_the_unculled_fp32_call(pkg, torch_cuda, planner):
    sc, pose, req = planner["scene"], planner["pose"], planner["req"]
    full = planner["full"][True]
    rc, summ, rec, n = _check(pkg, sc, pose, req, full, f32=True)
    assert rc == 0
    _same(summ["min_distance"], full[2]["min_distance"], "fp32 min_distance")
    _same(summ["min_pair"], full[2]["min_pair"], "fp32 min_pair")
    d_summ, d_rec, d_n = _device_nearest(torch_cuda, pkg, sc, pose, req, f32=True)
    assert d_n == n
    _same(d_summ, summ, "fp32 device form summaries")
    _same(d_rec, rec, "fp32 device form min records")
    # (random rotations: no distance comes near its box distance here; the aligned scenes below are where the rounding term is measured)
    _fp32_excess(sc, pose, full[1], "scene_planner(64, 16)")


# ---- e. an upper bound -----------------------------------------------------------------------------------------------------------------
def test_upper_bound(pkg, torch_cuda, planner):
    sc, tf, req = planner["scene"], planner["tf"], planner["req"]
    full = planner["full"][False]
    unbounded = _raw_nearest(pkg, sc, tf, req)
    for D in (0.5, 0.05):
        rc, summ, rec, n = _check(pkg, sc, tf, req, full, D=D)
        near = full[2]["min_distance"] <= D
        assert rc == 0 and 0 < near.sum() < 64
        _same(summ["min_distance"][near], full[2]["min_distance"][near], "exact where the minimum is within the bound")
        _same(summ["min_pair"][near], full[2]["min_pair"][near], "min_pair where the minimum is within the bound")
        assert np.all(summ["min_distance"][~near] > D)
        assert sum(n) < sum(unbounded[3])
        d_summ, d_rec, d_n = _device_nearest(torch_cuda, pkg, sc, tf, req, D=D)
        assert d_n == n
        _same(d_summ, summ, "device form with an upper bound")
        _same(d_rec, rec, "device form min records with an upper bound")
    # below every distance: nothing within the bound; -inf: only the queries without a bound are evaluated
    rc, summ, rec, n = _check(pkg, sc, tf, req, full, D=-10.0)
    assert np.all(summ["min_distance"] > -10.0)
    rc, summ, rec, n = _check(pkg, sc, tf, req, full, D=-np.inf)
    assert n[1] == 0 and np.all(summ["min_distance"] > -np.inf)


# ---- f. ties and edges -----------------------------------------------------------------------------------------------------------------
def test_ties_on_a_grid(pkg, torch_cuda):
    """Spheres and unit boxes on an axis-aligned grid, identity rotations: several pairs share the minimal distance bit for bit, the
    bound is as tight as it gets, and min_pair must be the lowest index."""
    abi = pkg.abi
    L = pkg.ShapeLibrary()
    L.add_sphere(0.25)
    L.add_box(1.0, 1.0, 1.0)
    obj_shape = np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=np.uint32)
    grid = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2], [6, 0, 0], [9, 0, 0], [6, 3, 0], [6, 0, 3]], dtype=np.float64)
    T = np.stack([grid, grid * 2.0 + 1.0, grid + [100.0, -50.0, 25.0]])
    tf = pkg.geometry.make_pose(T=T.reshape(-1, 3)).reshape(3, 8, 12)
    i, j = np.triu_indices(8, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    lib, scene = _make(pkg, L, obj_shape, pairs)
    try:
        req = abi.default_distance_request()
        full = _raw_distance(pkg, scene, tf, req)
        assert full[0] == 0
        d = full[1]["distance"].reshape(3, -1)
        ties = (d == d.min(axis=1, keepdims=True)).sum(axis=1)
        print("pairs at the minimal distance, by configuration:", ties)
        assert (ties >= 2).all()
        rc, summ, rec, n = _check(pkg, scene, tf, req, full)
        assert rc == 0
        _same(summ["min_pair"], full[2]["min_pair"], "the lowest index among the ties")
        assert list(summ["min_pair"]) == [int(np.flatnonzero(d[c] == d[c].min())[0]) for c in range(3)]
        got = _device_nearest(torch_cuda, pkg, scene, tf, req)
        _same(got[0], summ, "device form")
        # the fp32 forms on the same grid: the bound is tight, the rounding term has to cover the fp32 narrow phase
        pose = pkg.geometry.pose_f32_from_quat(np.tile([1.0, 0, 0, 0], (24, 1)), T.reshape(-1, 3)).reshape(3, 8, 7)
        full32 = _raw_distance(pkg, scene, pose, req, f32=True)
        r = _fp32_excess(scene, pose, full32[1], "the grid")
        assert r * 16 <= nearest_model.R32
        rc, summ32, rec32, n32 = _check(pkg, scene, pose, req, full32, f32=True)
        assert rc == 0
        _same(summ32["min_distance"], full32[2]["min_distance"], "fp32 min_distance on the grid")
        _same(summ32["min_pair"], full32[2]["min_pair"], "fp32 min_pair on the grid")
        got = _device_nearest(torch_cuda, pkg, scene, pose, req, f32=True)
        _same(got[0], summ32, "fp32 device form on the grid")
        _same(got[1], rec32, "fp32 device form min records on the grid")
    finally:
        scene.close()
        lib.close()


def test_fp32_forms_on_aligned_face_to_face_shapes(pkg, torch_cuda):
    """Where the fp32 bound could fail: every solid kind (Cone and Cylinder included) with identity rotations, the boxes of a pair face to
    face along one axis at separations 0.01, 3 and 100, around coordinate offsets 0, 30, 1000 and 4000.  The fp32 forms against the
    unculled fp32 call; the largest (lb - d_f32) / M is printed and must be covered 16 times by the constant."""
    abi = pkg.abi
    wl = pkg.workloads.all_primitives(n=1, seed=3, nper=3)
    lib_shapes = wl.lib
    n_shapes = len(lib_shapes)
    local = pkg.engine.world_aabbs(lib_shapes, np.arange(n_shapes, dtype=np.uint32), np.tile(pkg.geometry.make_pose()[None], (n_shapes, 1)))
    rng = np.random.default_rng(43)
    n_pair_obj, combos = 21, [(o, s) for o in (0.0, 30.0, 1000.0, 4000.0) for s in (0.01, 3.0, 100.0)]
    n_obj, n_conf = 2 * n_pair_obj, 2 * len(combos)
    obj_shape = np.concatenate([np.arange(n_shapes), rng.integers(0, n_shapes, n_obj - n_shapes)]).astype(np.uint32)
    rng.shuffle(obj_shape)
    pairs = np.stack([np.arange(0, n_obj, 2), np.arange(1, n_obj, 2)], axis=1).astype(np.uint32)
    T = np.zeros((n_conf, n_obj, 3))
    k = np.arange(n_pair_obj)
    for c in range(n_conf):
        offset, sep = combos[c % len(combos)]
        axis = rng.integers(0, 3, n_pair_obj)
        T1 = np.full((n_pair_obj, 3), offset) + rng.uniform(-1, 1, (n_pair_obj, 3))
        T2 = T1 + rng.uniform(-0.05, 0.05, (n_pair_obj, 3))
        s1, s2 = obj_shape[pairs[:, 0]], obj_shape[pairs[:, 1]]
        T2[k, axis] = T1[k, axis] + local[s1, 3 + axis] - local[s2, axis] + sep  # box 2's low face `sep` beyond box 1's high face
        T[c, pairs[:, 0]], T[c, pairs[:, 1]] = T1, T2
    pose = pkg.geometry.pose_f32_from_quat(np.tile([1.0, 0, 0, 0], (n_conf * n_obj, 1)), T.reshape(-1, 3)).reshape(n_conf, n_obj, 7)
    lib, scene = _make(pkg, lib_shapes, obj_shape, pairs)
    try:
        req = abi.default_distance_request()
        full = _raw_distance(pkg, scene, pose, req, f32=True)
        assert full[0] == 0
        r = _fp32_excess(scene, pose, full[1], "aligned face-to-face shapes")
        assert r * 16 <= nearest_model.R32
        rc, summ, rec, n = _check(pkg, scene, pose, req, full, f32=True)
        assert rc == 0
        _same(summ["min_distance"], full[2]["min_distance"], "fp32 min_distance of aligned shapes")
        _same(summ["min_pair"], full[2]["min_pair"], "fp32 min_pair of aligned shapes")
        got = _device_nearest(torch_cuda, pkg, scene, pose, req, f32=True)
        _same(got[0], summ, "fp32 device form")
        _same(got[1], rec, "fp32 device form min records")
        # the fp64 forms on the same table, widened
        tf = pkg.geometry.make_pose(T=pose.reshape(-1, 7)[:, 4:].astype(np.float64)).reshape(n_conf, n_obj, 12)
        full64 = _raw_distance(pkg, scene, tf, req)
        rc, summ, rec, n = _check(pkg, scene, tf, req, full64)
        _same(summ["min_pair"], full64[2]["min_pair"], "fp64 min_pair of aligned shapes")
    finally:
        scene.close()
        lib.close()


def test_plane_self_pair_unsupported_pair_and_nan_pose(pkg, torch_cuda):
    """A Plane (an unbounded box: no bound, always evaluated), a pair with i == j, a TriangleP pair (distance() has no evaluator), and a
    configuration with a NaN pose.  The return code and n_skipped are those of the culled host call: over the evaluated records."""
    abi, d = pkg.abi, pkg.engine.dll()
    L = pkg.ShapeLibrary()
    L.add_sphere(0.5)
    L.add_box(0.4, 0.5, 0.6)
    L.add_capsule(0.2, 0.6)
    L.add_plane([1, 2, -1], 3.0)
    L.add_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0])
    obj_shape = np.array([0, 1, 2, 3, 4, 0, 1, 2], dtype=np.uint32)
    rng = np.random.default_rng(19)
    T = rng.uniform(-2.0, 2.0, (3, 8, 3))
    T[:, 4] = T[:, 0] + 0.1  # the triangle beside body 0: their boxes touch, the pair is evaluated
    tf = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, 24), T=T.reshape(-1, 3)).reshape(3, 8, 12)
    tf[2, 5, 10] = np.nan  # configuration 2: a NaN pose
    i, j = np.triu_indices(8, 1)
    keep = ~((i == 3) & (j == 4))  # (not Plane x TriangleP: it would always be evaluated, and reported)
    pairs = np.concatenate([np.stack([i[keep], j[keep]], axis=1), [[1, 1]]]).astype(np.uint32)
    lib, scene = _make(pkg, L, obj_shape, pairs)
    try:
        req = abi.default_distance_request()
        full = _raw_distance(pkg, scene, tf, req)
        assert full[0] == abi.ERR_UNSUPPORTED_PAIR
        rc, summ, rec, n = _check(pkg, scene, tf, req, full)
        tri = np.flatnonzero((obj_shape[pairs] == 4).any(axis=1))
        assert rc == abi.ERR_UNSUPPORTED_PAIR and "not yet supported" in pkg.engine.last_error()
        assert (summ["n_skipped"] >= 1).all() and (summ["n_skipped"] <= len(tri)).all()
        # the culled host call (boxes that touch): the same code
        out = np.zeros(3 * len(pairs), dtype=abi.RESULT_DTYPE)
        csumm = np.zeros(3, dtype=abi.SCENE_SUMMARY_DTYPE)
        k = C.c_size_t(0)
        tab = np.ascontiguousarray(tf)
        crc = d.hfcl_scene_distance_culled(scene._h, abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), C.byref(req), abi.ptr(out), C.c_size_t(len(out)),
                                           None, None, abi.ptr(csumm), None, None, C.byref(k))
        assert crc == rc and (summ["n_skipped"] >= csumm["n_skipped"]).all()  # (every touching pair is in pass 1)
        # every pair of the Plane and the self pair are evaluated: their records count
        plane = np.flatnonzero((obj_shape[pairs] == 3).any(axis=1))
        assert n[0] >= 3 * (len(plane) + 1)
        _same(summ["min_distance"], full[2]["min_distance"], "min_distance beside a NaN pose")
        _same(summ["min_pair"], full[2]["min_pair"], "min_pair beside a NaN pose")
        # the triangle far from everything (and no NaN box beside it): its pairs are not evaluated, nothing is reported
        away = tf[:2].copy()
        away[:, 4, 9] += 500.0
        full = _raw_distance(pkg, scene, away, req)
        rc, summ, rec, n = _check(pkg, scene, away, req, full)
        assert full[0] == abi.ERR_UNSUPPORTED_PAIR and rc == abi.OK, pkg.engine.last_error()
        assert not summ["n_skipped"].any()
        # the device form reads nothing back: no code, the same summaries
        got = _device_nearest(torch_cuda, pkg, scene, tf, req)
        rc, summ, rec, n = _raw_nearest(pkg, scene, tf, req)
        _same(got[0], summ, "device form beside unsupported pairs")
        _same(got[1], rec, "device form min records beside unsupported pairs")
    finally:
        scene.close()
        lib.close()


def test_one_pair_far_apart_and_no_records(pkg, torch_cuda):
    abi = pkg.abi
    L = pkg.ShapeLibrary()
    L.add_sphere(0.5)
    L.add_box(0.4, 0.5, 0.6)
    L.add_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0])
    rng = np.random.default_rng(29)
    req = abi.default_distance_request()
    # a one-pair scene
    tf = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, 10), T=rng.uniform(-3, 3, (10, 3))).reshape(5, 2, 12)
    lib, scene = _make(pkg, L, np.array([0, 1], dtype=np.uint32), [[0, 1]])
    try:
        full = _raw_distance(pkg, scene, tf, req)
        rc, summ, rec, n = _check(pkg, scene, tf, req, full)
        assert rc == 0 and sum(n) == 5 and np.array_equal(summ["min_pair"], np.zeros(5))
        _same(rec, full[1], "one pair: the min records are the records")
        # an upper bound below the boxes' distance in two configurations: those have no record at all
        tf[3:, 1, 9] += 50.0
        full = _raw_distance(pkg, scene, tf, req)
        D = 10.0
        rc, summ, rec, n = _check(pkg, scene, tf, req, full, D=D)
        far = summ["min_pair"] == NONE
        assert list(far) == [False] * 3 + [True] * 2 and sum(n) == 3 and np.all(np.isposinf(summ["min_distance"][far])) and np.all(rec["status"][far] == 0x80000000)
        assert np.all(np.isposinf(rec["distance"][far]))
        got = _device_nearest(torch_cuda, pkg, scene, tf, req, D=D)
        _same(got[0], summ, "device form, configurations without records")
        _same(got[1], rec, "device form, min records of configurations without records")
        # no pair: configurations without records
        scene.set_pairs(np.zeros((0, 2), dtype=np.uint32))
        _PAIRS[id(scene)] = np.zeros((0, 2), dtype=np.uint32)
        rc, summ, rec, n = _raw_nearest(pkg, scene, tf, req)
        assert rc == 0 and n == (0, 0) and np.all(summ["min_pair"] == NONE) and np.all(np.isposinf(summ["min_distance"]))
        assert np.all(rec["status"] == 0x80000000) and np.all(np.isposinf(rec["distance"])) and not summ["n_skipped"].any()
        got = _device_nearest(torch_cuda, pkg, scene, tf, req)
        _same(got[0], summ, "device form without pairs")
        _same(got[1], rec, "device form min records without pairs")
    finally:
        scene.close()
        lib.close()
    # every body far from every other: a configuration evaluates its seed and what lies within the seed's distance
    n_obj = 9
    T = rng.uniform(-0.3, 0.3, (4, n_obj, 3))
    T[..., 0] += np.arange(n_obj) * 40.0
    tf = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, 4 * n_obj), T=T.reshape(-1, 3)).reshape(4, n_obj, 12)
    i, j = np.triu_indices(n_obj, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    lib, scene = _make(pkg, L, (np.arange(n_obj) % 2).astype(np.uint32), pairs)
    try:
        full = _raw_distance(pkg, scene, tf, req)
        rc, summ, rec, n = _check(pkg, scene, tf, req, full)
        assert rc == 0 and n[0] == 4 and n[1] < 4 * n_obj
        _same(summ["min_pair"], full[2]["min_pair"], "far apart")
        # a NaN upper bound and a null summary are refused before any work
        tab = np.ascontiguousarray(tf)
        before = sum(lib.last_bucket_counts().values())
        d = pkg.engine.dll()
        k = (C.c_size_t * 2)(5, 5)
        s = np.zeros(4, dtype=abi.SCENE_SUMMARY_DTYPE)
        assert d.hfcl_scene_nearest(scene._h, abi.ptr(tab), C.c_size_t(4), C.byref(req), C.c_double(np.nan), abi.ptr(s), None, k) == abi.ERR_INVALID_ARGUMENT
        assert "upper_bound" in pkg.engine.last_error()
        assert d.hfcl_scene_nearest(scene._h, abi.ptr(tab), C.c_size_t(4), C.byref(req), C.c_double(1.0), None, None, k) == abi.ERR_INVALID_ARGUMENT
        assert d.hfcl_scene_nearest(scene._h, abi.ptr(tab), C.c_size_t(4), None, C.c_double(1.0), abi.ptr(s), None, k) == abi.ERR_INVALID_ARGUMENT
        assert tuple(k) == (5, 5) and not s.view(np.uint8).any() and sum(lib.last_bucket_counts().values()) == before
        # no configuration: HFCL_OK, nothing written but the counts
        assert d.hfcl_scene_nearest(scene._h, abi.ptr(tab), C.c_size_t(0), C.byref(req), C.c_double(np.inf), abi.ptr(s), None, k) == abi.OK
        assert tuple(k) == (0, 0) and not s.view(np.uint8).any()
    finally:
        scene.close()
        lib.close()


def test_long_pair_list(pkg, torch_cuda):
    """A pair list of several fold pieces (600 pairs): the seeds and both folds go through partials; chunks that cut pieces."""
    rng = np.random.default_rng(31)
    L = pkg.ShapeLibrary()
    for r in rng.uniform(0.1, 0.3, 6):
        L.add_sphere(float(r))
    for s in rng.uniform(0.2, 0.5, (3, 3)):
        L.add_box(*map(float, s))
    n_obj, n_conf = 40, 4
    obj_shape = rng.integers(0, 9, n_obj).astype(np.uint32)
    tf = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, n_conf * n_obj), T=rng.uniform(-4, 4, (n_conf * n_obj, 3))).reshape(n_conf, n_obj, 12)
    i, j = np.triu_indices(n_obj, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)[::-1][:600].copy()  # (the late pairs first: seeds beyond the first piece)
    lib, scene = _make(pkg, L, obj_shape, pairs)
    try:
        req = pkg.abi.default_distance_request()
        full = _raw_distance(pkg, scene, tf, req)
        base = _check(pkg, scene, tf, req, full)
        _same(base[1]["min_pair"], full[2]["min_pair"], "long list")
        for scene_chunk, cull_chunk in ((64, 257), (3, 700)):
            lib.set_option("scene_chunk", scene_chunk)
            lib.set_option("scene_cull_chunk", cull_chunk)
            got = _raw_nearest(pkg, scene, tf, req)
            assert got[3] == base[3]
            _same(got[1], base[1], "summaries in chunks")
            _same(got[2], base[2], "min records in chunks")
    finally:
        lib.set_option("scene_chunk", 0)
        lib.set_option("scene_cull_chunk", 0)
        scene.close()
        lib.close()


# ---- g. meshes ---------------------------------------------------------------------------------------------------------------------------
def test_meshes_and_solids(pkg, torch_cuda):
    """Six solids and two small BVHModel<OBBRSS>: mesh x mesh, mesh x solid and solid x solid pairs in one list.  The min records of the
    configurations whose closest pair has a mesh carry its triangle ids."""
    abi = pkg.abi
    meshes = pkg.workloads.mesh_variants(2, 8, 6)
    rng = np.random.default_rng(37)
    L = pkg.ShapeLibrary()
    for k, m in enumerate(meshes):
        L.add_bvh(k, len(m.vertices))
    for r in rng.uniform(0.2, 0.4, 2):
        L.add_sphere(float(r))
    for s in rng.uniform(0.3, 0.6, (2, 3)):
        L.add_box(*map(float, s))
    for s in rng.uniform(0.2, 0.4, (2, 2)):
        L.add_capsule(*map(float, s))
    n_obj, n_conf = 8, 6
    T = rng.uniform(-3.5, 3.5, (n_conf, n_obj, 3))
    T[0, :2] = [[0, 0, 0], [2.6, 0, 0]]  # configuration 0: the two meshes side by side, the solids in a row far from them and each other
    T[0, 2:] = np.stack([np.arange(6) * 3.0, np.full(6, 8.0), np.zeros(6)], axis=1)
    tf = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, n_conf * n_obj), T=T.reshape(-1, 3)).reshape(n_conf, n_obj, 12)
    i, j = np.triu_indices(n_obj, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    lib, scene = _make(pkg, L, np.arange(n_obj, dtype=np.uint32), pairs, meshes)
    try:
        req = abi.default_distance_request()
        full = _raw_distance(pkg, scene, tf, req)
        assert full[0] == 0
        rc, summ, rec, n = _check(pkg, scene, tf, req, full)
        assert rc == 0
        _same(summ["min_distance"], full[2]["min_distance"], "mesh scene min_distance")
        _same(summ["min_pair"], full[2]["min_pair"], "mesh scene min_pair")
        assert summ["min_pair"][0] == 0 and rec["b1"][0] >= 0 and rec["b2"][0] >= 0  # (mesh x mesh: both triangle ids)
        print("mesh scene: %d + %d of %d queries evaluated" % (n[0], n[1], n_conf * len(pairs)))
        got = _device_nearest(torch_cuda, pkg, scene, tf, req)
        _same(got[0], summ, "device form")
        _same(got[1], rec, "device form min records")
    finally:
        scene.close()
        lib.close()


# ---- front ends ----------------------------------------------------------------------------------------------------------------------------
def test_compat_distance_scene_nearest(pkg, torch_cuda):
    """compat.distance_scene(..., nearest=True): per configuration the DistanceResult DistanceCallBackDefault leaves behind."""
    fcl = pkg.compat
    rng = np.random.default_rng(21)
    geoms = [fcl.Box(0.6, 0.8, 1.0), fcl.Sphere(0.5), fcl.Capsule(0.3, 1.2), fcl.Ellipsoid(0.4, 0.6, 0.8)]
    objs = []
    for k in range(12):
        t = fcl.Transform3f()
        t.setTranslation(rng.uniform(-4, 4, 3))
        objs.append(fcl.CollisionObject(geoms[k % 4], t))
    i, j = np.triu_indices(12, 1)
    pr = np.stack([i, j], axis=1)
    req = fcl.DistanceRequest()
    dist, rec, summ = fcl.distance_scene(objs, pr, req)
    res = fcl.distance_scene(objs, pr, req, nearest=True)
    assert len(res) == 1
    p = int(summ["min_pair"][0])
    r = res[0]
    assert r.min_distance == dist[0].min() == summ["min_distance"][0] and p == int(dist[0].argmin())
    assert r.o1 is geoms[pr[p][0] % 4] and r.o2 is geoms[pr[p][1] % 4]
    assert np.array_equal(r.nearest_points[0], rec["p1"][p]) and np.array_equal(r.nearest_points[1], rec["p2"][p]) and np.array_equal(r.normal, rec["normal"][p])
    # a bound below the minimum: the result stays as DistanceResult() leaves it
    far = fcl.distance_scene(objs, pr, req, nearest=True, upper_bound=float(summ["min_distance"][0]) - 0.5)[0]
    assert far.min_distance == np.finfo(np.float64).max and far.o1 is None


def test_cpp_shim_nearest(tmp_path):
    """include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene::nearest against the unculled Scene::distance (g++ build)."""
    exe = str(tmp_path / "test_nearest_shim")
    libdir = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_nearest", "test_nearest_shim.cpp"), "-L" + libdir, "-lhppfcl_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("same") == 2 and "DIFFERENT" not in r.stdout
