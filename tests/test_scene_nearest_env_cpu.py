"""The clearance of the moving objects among an environment kept on the device (include/hppfcl_amd_nearest_env.h) without a GPU: the
exports, bindings, header placement and refusals; the numpy model of tests/nearest_env_model.py held against nearest_model.select on
the explicit list P_env and against nearest_self_model.select with the extra environment group, with the oracle's records; the header
(hpp-fcl_amd/csrc/hfcl_nearest_env.hpp) built with g++ (tests/nearest_env_harness) -- set-time terms, seed partials and their combine,
count and emit of both passes, every span length and chunk, with and without groups, with and without pruning -- against the model
byte for byte; and the pruning property on its own: Lt <= L(i, j) for every pair of a cell, Lt = -inf whenever a pair has L = -inf."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import env_model
import nearest_env_model as model
import nearest_model
import nearest_self_model
import pairs_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
FILL32, FILL64 = 0xABABABAB, 0xABABABABABABABAB
SRC = os.path.join(ROOT, "tests", "nearest_env_harness", "nearest_env_harness.cpp")
SYMBOLS = ["hfcl_scene_nearest_env", "hfcl_scene_nearest_env_device", "hfcl_scene_nearest_env_device_f32", "hfcl_scene_nearest_env_f32"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nearest_env_harness") / "libnearest_env_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-o", out, SRC])
    d = C.CDLL(out)
    d.neh_sweep.restype = C.c_uint64
    d.neh_sizes.restype = C.c_uint64
    d.neh_terms.restype = C.c_uint32
    return d


_SCENES = {}


def _scene(pkg, oracle, n_moving, n_env, with_groups=False):
    """Drawn again (the next seed) until the scene holds what it promises; built once, shared, not modified."""
    key = (n_moving, n_env, with_groups)
    if key not in _SCENES:
        if "lib" not in _SCENES:
            _SCENES["lib"] = pairs_model.mixed_library(pkg)
        groups = env_model.robot_groups(n_moving, n_moving + n_env) if with_groups else None
        last = None
        for seed in range(8):
            try:
                sc = model.NearestEnvScene(pkg, oracle, _SCENES["lib"], n_moving, n_env, seed, groups)
                sc.checked = sc.check()
            except AssertionError as e:
                last = e
                continue
            _SCENES[key] = sc
            break
        else:
            raise AssertionError("no scene of %r holds what it promises: %s" % (key, last))
    return _SCENES[key]


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_bindings_and_header_placement(pkg, harness):
    pkg.engine.build_native()
    lib = pkg.engine.dll()
    e = pkg.engine
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_nearest_env.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_scene_nearest_env[a-z0-9_]*)\s*\(", hdr)))
    assert syms == sorted(e.NEAREST_ENV_SYMBOLS) == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s
    assert not set(syms) & set(e.EXPORTED_SYMBOLS + e.CULL_SYMBOLS + e.NEAREST_SYMBOLS + e.PAIRS_SYMBOLS + e.GROUPS_SYMBOLS + e.NEAREST_SELF_SYMBOLS +
                               e.ENV_SYMBOLS)
    env_hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_env.h")).read()
    assert "nearest_env" not in env_hdr and len(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]+)\s*\(", env_hdr))) == 17
    main = open(os.path.join(ROOT, "include", "hppfcl_amd.h")).read()
    assert main.count('#include "hppfcl_amd_nearest_env.h"') == 1
    assert main.index("hppfcl_amd_env.h") < main.index('#include "hppfcl_amd_nearest_env.h"') < main.index('#include "hppfcl_amd_pairs.h"')
    assert "hfcl_scene_nearest_env" not in main
    assert lib.hfcl_abi_version() == 5
    for m in ("nearest_env", "nearest_env_device", "nearest_env_device_f32"):
        assert hasattr(e.Scene, m), m
    assert "scene_nearest_env_prune" in e.option_keys()
    assert harness.neh_sizes(0) == 24 == pkg.abi.SCENE_CLEARANCE_DTYPE.itemsize and harness.neh_sizes(1) == 16
    assert harness.neh_sizes(2) == model.TILE and harness.neh_sizes(3) == model.ROWS
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd.h")])
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd_nearest_env.h")])


def test_refusals(pkg):
    """No CPU fallback: without a device every entry point says so.  With one: a NaN bound and a null scene -- whatever the bound -- are
    invalid arguments (tests/test_scene_nearest_env_gpu.py, which has a scene, holds the others).  Nothing is written."""
    d, abi = pkg.engine.dll(), pkg.abi
    req = abi.default_distance_request()
    tf = np.zeros((2, 12))
    out = np.full(24, 0x5A, dtype=np.uint8).view(abi.SCENE_CLEARANCE_DTYPE)
    before = out.tobytes()
    n = (C.c_size_t * 2)(7, 7)
    n1 = C.c_size_t(1)
    no_device = pkg.engine.device_count() == 0
    for bound, word in ((np.inf, "null scene"), (0.5, "null scene"), (np.nan, "upper_bound")):
        calls = [
            (d.hfcl_scene_nearest_env, (None, abi.ptr(tf), n1, C.byref(req), C.c_double(bound), abi.ptr(out), None, n)),
            (d.hfcl_scene_nearest_env_f32, (None, None, n1, C.byref(req), C.c_double(bound), abi.ptr(out), None, n)),
            (d.hfcl_scene_nearest_env_device, (None, None, n1, C.byref(req), C.c_double(bound), None, None, n, None)),
            (d.hfcl_scene_nearest_env_device_f32, (None, None, n1, C.byref(req), C.c_double(bound), None, None, n, None)),
        ]
        assert sorted(fn.__name__ for fn, _ in calls) == SYMBOLS
        for fn, args in calls:
            assert fn(*args) == (abi.ERR_NO_DEVICE if no_device else abi.ERR_INVALID_ARGUMENT), fn.__name__
            assert ("no CPU fallback" if no_device else word) in pkg.engine.last_error(), (fn.__name__, pkg.engine.last_error())
    assert out.tobytes() == before and tuple(n) == (7, 7)


def test_shim_method_compiles(tmp_path):
    src = tmp_path / "shim.cpp"
    src.write_text('#include "hppfcl_amd_compat.hpp"\n'
                   "void use(hpp::fcl::amd::Scene& s, const hpp::fcl::Transform3f* t, std::vector<hfcl_scene_clearance>& c, "
                   "std::vector<hpp::fcl::DistanceResult>& m) { size_t n[2]; s.nearestEnv(t, 1, hpp::fcl::DistanceRequest(), 0.5, c, &m, n); "
                   "s.nearestEnv(t, 1, hpp::fcl::DistanceRequest(), 1.0 / 0.0, c); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src)])


def test_option_is_described(pkg):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`scene_nearest_env_prune`" in text


# ---- 2. the model: the scenes, and the definitions already proven -------------------------------------------------------------------------
@pytest.mark.parametrize("n_moving,n_env", model.SIZES)
def test_scenes_hold_what_they_promise(pkg, oracle, n_moving, n_env):
    """Asserted on the model's output (NearestEnvScene.check): hover has no touching box, a positive clearance, a pass 1 of exactly
    the seed and -- scenes of at least 100 candidates -- at most 25 % of its candidates evaluated; graze has touching boxes and a
    positive clearance; some EnvScene configuration collides; every environment tile holds an evaluated pair; with more than one
    tile some pass-2 sweep drops a cell by Lt and keeps another."""
    sc = _scene(pkg, oracle, n_moving, n_env)
    share, d1, d2, cells = sc.checked
    print("(%d, %d): %d candidates a configuration, hover evaluates %.2f %%, cells dropped by Lt: pass 1 %d, pass 2 %d of %d; clearances %s"
          % (n_moving, n_env, len(sc.P), 100 * share, d1, d2, cells, sc.select()["clearance"]["min_distance"]))
    assert sc.kinds == ["far", "among", "among", "hover", "graze"]
    if n_moving + n_env >= 2:
        assert sc.has_graze


def _check_against_list(abi, sc, D, r=nearest_model.R64):
    """The model against nearest_model.select on P_env and against nearest_self_model.select with the environment group."""
    sel = model.select(abi, sc.boxes, sc.n_moving, sc.groups, sc.records, D, r)
    P, n_pairs = sc.P, len(sc.P)
    key = lambda ij: (ij[:, 0].astype(np.uint64) << np.uint64(32)) | ij[:, 1].astype(np.uint64)  # noqa: E731
    if n_pairs:
        old = nearest_model.select(abi, nearest_model.query_bounds(sc.boxes, P, r), sc.records, D)
        assert np.array_equal(sel["seed"], key(P[old["seed"].astype(np.int64)]))
        assert sel["thr"].tobytes() == old["thr"].tobytes()
        for l in ("1", "2"):
            ids = old["ids" + l].astype(np.int64)
            assert sel["conf_begin" + l].tobytes() == old["conf_begin" + l].tobytes()
            assert np.array_equal(sel["pairs" + l], P[ids % n_pairs])
            assert np.array_equal(pairs_model.conf_of(sel["conf_begin" + l]), ids // n_pairs)
        s, clear = old["summary"], sel["clearance"]
        assert clear["min_distance"].tobytes() == s["min_distance"].tobytes()
        has = s["min_pair"] != NONE
        assert np.array_equal(clear["min_i"][has], P[s["min_pair"][has].astype(np.int64), 0])
        assert np.array_equal(clear["min_j"][has], P[s["min_pair"][has].astype(np.int64), 1])
        assert np.all(clear["min_i"][~has] == NONE) and np.all(clear["min_j"][~has] == NONE)
        assert np.array_equal(clear["n_skipped"], s["n_skipped"])
        assert np.array_equal(clear["n_evaluated"], np.diff(old["conf_begin1"].astype(np.int64)) + np.diff(old["conf_begin2"].astype(np.int64)))
    # nearest_self on the full table with groups that forbid exactly the environment x environment pairs: the same candidates, so the
    # same list P and the same records
    full_groups = model.env_groups(sc.n_moving, sc.n, sc.groups)
    assert np.array_equal(nearest_self_model.explicit_list(sc.n, full_groups), P)
    ref = nearest_self_model.select(abi, sc.boxes, full_groups, sc.records, D, r)
    for k in ("seed", "pairs1", "conf_begin1", "thr", "pairs2", "conf_begin2", "clearance", "min_records"):
        assert sel[k].dtype == ref[k].dtype and sel[k].tobytes() == ref[k].tobytes(), k
    return sel


# (with groups: env_model.robot_groups -- a group per link, at most 63, and one for the environment)
WITH_GROUPS = [(1, 1, True), (5, 255, True), (17, 257, True)]


@pytest.mark.parametrize("n_moving,n_env,with_groups", [s + (False,) for s in model.SIZES] + WITH_GROUPS)
def test_model_equals_the_selections_already_proven(pkg, oracle, n_moving, n_env, with_groups):
    sc = _scene(pkg, oracle, n_moving, n_env, with_groups)
    for D in (np.inf, 0.5, 0.0):
        for r in (nearest_model.R64, nearest_model.R32):
            sel = _check_against_list(pkg.abi, sc, D, r)
            if len(sc.P):
                beyond = nearest_self_model.check_against_full(pkg.abi, sel, sc.P, sc.records, D)
                assert beyond < sc.n_conf or D < np.inf


# ---- 3. the header's host build ---------------------------------------------------------------------------------------------------------
def _terms(harness, pkg, env_boxes):
    b = np.ascontiguousarray(env_boxes, dtype=np.float64).reshape(-1, 6)
    tiles = (len(b) + model.TILE - 1) // model.TILE
    tb, et, tt, plain = np.full((tiles, 6), 123.0), np.full((len(b), 2), 123.0), np.full((tiles, 2), 123.0), np.full((len(b), 3), 123.0)
    p = pkg.abi.ptr
    assert harness.neh_terms(p(b) if len(b) else None, C.c_uint32(len(b)), p(tb) if tiles else None, p(et) if len(b) else None,
                             p(tt) if tiles else None, p(plain) if len(b) else None) == tiles
    return tb, et, tt, plain


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _special_boxes(rng, n_env):
    big = np.finfo(np.float64).max
    mid = rng.uniform(-20, 20, (n_env, 3))
    half = rng.uniform(0.0, 2.0, (n_env, 3))
    boxes = np.concatenate([mid - half, mid + half], axis=1)
    cases = {"plain": boxes}
    nan = boxes.copy()
    nan[(3 * n_env) // 4, 1] = np.nan
    cases["nan"] = nan
    inf = boxes.copy()
    inf[n_env // 2] = [-np.inf, -np.inf, -big, np.inf, big, np.inf]
    cases["inf"] = inf
    plane = boxes.copy()
    plane[n_env // 3] = [-big, -big, 5, big, big, 5]  # finite coordinates, a diagonal that overflows
    cases["plane"] = plane
    return cases


def test_set_time_terms_bit_for_bit(pkg, harness):
    """Box terms and tile terms from the harness: nearest_box_terms per member, packed by nself_pack_largest; the numpy model's."""
    rng = np.random.default_rng(11)
    for n_env in (1, 255, 256, 257, 513, 600):
        for name, b in _special_boxes(rng, n_env).items():
            tb, et, tt, plain = _terms(harness, pkg, b)
            assert _bits(tb) == _bits(env_model.tile_boxes(b)), (n_env, name)
            finite = plain[:, 2] == 1.0
            assert np.array_equal(finite, np.isfinite(b).all(axis=1))
            assert _bits(et[:, 0]) == _bits(plain[:, 0]) and _bits(et[:, 1]) == _bits(np.where(finite, plain[:, 1], -1.0)), (n_env, name)
            assert _bits(et) == _bits(model.box_terms(b)), (n_env, name)
            assert _bits(tt) == _bits(model.tile_terms(b)), (n_env, name)
            for t in range(len(tt)):  # ... and per tile from the members' plain terms
                m = slice(t * model.TILE, (t + 1) * model.TILE)
                wild = not finite[m].all()
                assert tt[t, 1] == (-1.0 if wild else plain[m, 1].max()), (n_env, name, t)
                if not wild:
                    assert tt[t, 0] == plain[m, 0].max()
            assert (tt[:, 1] < 0).any() == (name in ("nan", "inf"))


def _header_run(harness, pkg, sc, D, r, chunk_rows, span, prune, confs=None):
    """The whole call on the host: seeds, the list of pass 1, its ranked fold, thresholds, the list of pass 2, its fold, the combination."""
    abi = pkg.abi
    confs = list(range(sc.n_conf)) if confs is None else confs
    n_conf, nm, ne, n = len(confs), sc.n_moving, sc.n_env, sc.n
    P = sc.P
    records = sc.records.reshape(sc.n_conf, len(P))[confs].reshape(-1)
    index = np.full((max(nm, 1), max(n, 1)), -1, dtype=np.int64)
    index[P[:, 0], P[:, 1]] = np.arange(len(P))
    moving = np.ascontiguousarray(sc.boxes[confs][:, :nm])
    env = np.ascontiguousarray(sc.boxes[0, nm:])
    grp = np.ascontiguousarray(sc.groups[0], dtype=np.uint8) if sc.groups is not None else None
    words = np.ascontiguousarray(sc.groups[1], dtype=np.uint64) if sc.groups is not None else None
    seed = np.full(n_conf, FILL64, dtype=np.uint64)
    thr = np.full(n_conf, np.nan)
    cap = max(n_conf * len(P), 1)
    stats = np.zeros(3, dtype=np.uint64)

    def sweep(mode, pairs, cb):
        return harness.neh_sweep(abi.ptr(moving) if moving.size else None, C.c_uint32(nm), abi.ptr(env) if env.size else None, C.c_uint32(ne),
                                 C.c_uint64(n_conf), abi.ptr(grp), C.c_uint32(len(words) if words is not None else 0), abi.ptr(words),
                                 C.c_double(r), C.c_double(D), C.c_int(mode), C.c_int(prune), C.c_uint64(chunk_rows), C.c_uint32(span),
                                 C.c_uint32(256), abi.ptr(seed), abi.ptr(thr), abi.ptr(pairs), C.c_uint64(cap if pairs is not None else 0),
                                 abi.ptr(cb), abi.ptr(stats))

    sweep(0, None, None)
    out = dict(seed=seed.copy(), dropped=[], never=0)
    sums, recs = [], []
    for l in (1, 2):
        pairs = np.full((cap + 3, 2), FILL32, dtype=np.uint32)  # (three guard entries)
        cb = np.full(n_conf + 1, FILL64, dtype=np.uint64)
        k = sweep(l, pairs, cb)
        out["dropped"].append((int(stats[0]), int(stats[1])))
        out["never"] += int(stats[2])
        assert np.all(pairs[k:] == FILL32) and cb[-1] == k
        assert sweep(l, None, np.zeros(n_conf + 1, dtype=np.uint64)) == k  # (the count alone)
        pairs = np.ascontiguousarray(pairs[:k])
        assert np.all(index[pairs[:, 0], pairs[:, 1]] >= 0)
        rec = records[pairs_model.conf_of(cb) * len(P) + index[pairs[:, 0], pairs[:, 1]]]
        summ = pairs_model.fold_ranked(abi, rec, cb)
        if l == 1:
            harness.neh_threshold(abi.ptr(summ), C.c_uint64(n_conf), C.c_double(D), abi.ptr(thr))
            out["thr"] = thr.copy()
        out["pairs%d" % l], out["conf_begin%d" % l] = pairs, cb
        sums.append(summ)
        recs.append(np.ascontiguousarray(rec))
    clear = np.full(n_conf * 24, 0xAB, dtype=np.uint8).view(abi.SCENE_CLEARANCE_DTYPE)
    mins = np.full(n_conf * 96, 0xAB, dtype=np.uint8).view(abi.RESULT_DTYPE)
    harness.neh_combine(C.c_uint64(n_conf), abi.ptr(sums[0]), abi.ptr(sums[1]), abi.ptr(out["pairs1"]), abi.ptr(out["pairs2"]),
                        abi.ptr(out["conf_begin1"]), abi.ptr(out["conf_begin2"]), abi.ptr(recs[0]), abi.ptr(recs[1]), abi.ptr(clear), abi.ptr(mins))
    out["clearance"], out["min_records"] = clear, mins
    return out


KEYS = ("seed", "pairs1", "conf_begin1", "thr", "pairs2", "conf_begin2", "clearance", "min_records")


@pytest.mark.parametrize("n_moving,n_env,with_groups", [s + (False,) for s in model.SIZES] + WITH_GROUPS)
def test_header_sweeps_equal_the_model(pkg, oracle, harness, n_moving, n_env, with_groups):
    """Seed partials and their combine, count and emit of both passes: span lengths 1, 2 and automatic, chunks of 16 rows and the whole
    call, with pruning and without -- the same bytes, the model's.  What pruning drops is the model's count; it never holds a pair of
    its pass."""
    sc = _scene(pkg, oracle, n_moving, n_env, with_groups)
    for D, r in ((np.inf, nearest_model.R64), (0.5, nearest_model.R64), (0.0, nearest_model.R32)):
        exp = sc.select(D, r)
        drop1, drop2, _ = model.dropped_cells(exp, sc.boxes, n_moving, r)
        for chunk_rows in (16, 0):
            for span in (1, 2, 0):
                for prune in (1, 0):
                    got = _header_run(harness, pkg, sc, D, r, chunk_rows, span, prune)
                    what = (n_moving, n_env, with_groups, D, chunk_rows, span, prune)
                    for k in KEYS:
                        assert got[k].dtype == exp[k].dtype and got[k].tobytes() == exp[k].tobytes(), (k,) + what
                    assert got["never"] == 0, what
                    if not prune:
                        assert got["dropped"][0][0] == 0 and got["dropped"][1][0] == 0, what
                    elif not with_groups:  # (with groups a cell the groups skip is not looked at: the model counts cells by distance alone)
                        assert got["dropped"][0] == (int(drop1.sum()), drop1.size) and got["dropped"][1] == (int(drop2.sum()), drop2.size), what
        if D == np.inf and sc.n_tiles > 1:
            assert drop2.any() and not drop2.all()


def test_configurations_one_by_one(pkg, oracle, harness):
    """n_conf = 1: every configuration of a five-configuration scene alone gives its part of the whole call's bytes."""
    sc = _scene(pkg, oracle, 17, 257)
    exp = sc.select()
    for c in range(sc.n_conf):
        got = _header_run(harness, pkg, sc, np.inf, nearest_model.R64, 0, 0, 1, confs=[c])
        assert got["clearance"].tobytes() == exp["clearance"][c:c + 1].tobytes()
        assert got["min_records"].tobytes() == exp["min_records"][c:c + 1].tobytes() and got["seed"][0] == exp["seed"][c]
        for l in ("1", "2"):
            lo, hi = int(exp["conf_begin" + l][c]), int(exp["conf_begin" + l][c + 1])
            assert got["pairs" + l].tobytes() == exp["pairs" + l][lo:hi].tobytes()


def test_no_moving_object_and_no_candidate(pkg, oracle, harness):
    """n_moving == 0; groups that allow no pair: no seed, empty lists, the "no record" answers."""
    abi = pkg.abi
    base = _scene(pkg, oracle, 5, 255)

    class Sub:
        pass
    for nm, groups in ((0, None), (5, (np.zeros(base.n, dtype=np.uint8), np.array([0], dtype=np.uint64)))):
        sc = Sub()
        sc.n_moving, sc.n_env, sc.n, sc.n_conf, sc.groups = nm, base.n_env, nm + base.n_env, base.n_conf, groups
        sc.boxes = np.ascontiguousarray(base.boxes[:, base.n_moving - nm:])
        sc.P = model.explicit_list(nm, sc.n, groups)
        sc.records = np.zeros(0, dtype=abi.RESULT_DTYPE)
        assert len(sc.P) == 0
        exp = model.select(abi, sc.boxes, nm, groups, sc.records)
        for prune in (1, 0):
            got = _header_run(harness, pkg, sc, np.inf, nearest_model.R64, 0, 0, prune)
            for k in KEYS:
                assert got[k].tobytes() == exp[k].tobytes(), k
            assert np.all(got["seed"] == model.NO_PAIR) and np.all(np.isposinf(got["clearance"]["min_distance"]))
            assert np.all(got["clearance"]["min_i"] == NONE) and np.all(got["clearance"]["n_evaluated"] == 0)
            assert np.all(got["min_records"]["status"] == 0x80000000) and np.all(np.isposinf(got["min_records"]["distance"]))


# ---- 4. the pruning property, on its own ---------------------------------------------------------------------------------------------------
def _property(harness, pkg, rows, members, r):
    """rows / members: lists of (k, 6) arrays, a cell each -> (Lt, min L, any L = -inf) per cell."""
    abi = pkg.abi
    rb = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.uint64)
    mb = np.concatenate([[0], np.cumsum([len(x) for x in members])]).astype(np.uint64)
    R, M = np.ascontiguousarray(np.concatenate(rows)), np.ascontiguousarray(np.concatenate(members))
    n = len(rows)
    Lt, least, none = np.full(n, np.nan), np.full(n, np.nan), np.full(n, 7, dtype=np.uint8)
    harness.neh_property(abi.ptr(R), abi.ptr(rb), abi.ptr(M), abi.ptr(mb), C.c_uint64(n), C.c_double(r), abi.ptr(Lt), abi.ptr(least), abi.ptr(none))
    return Lt, least, none.astype(bool)


def test_cell_bound_never_exceeds_a_pair_bound(pkg, harness):
    """10^5 random cells (1 .. 16 row boxes, 1 .. 256 member boxes, scales 1e-3 .. 1e5, the tile from touching the block to far from
    it) and cells made by hand: Lt <= L(i, j) for all pairs; Lt = -inf whenever a pair has L = -inf."""
    rng = np.random.default_rng(17)
    big = np.finfo(np.float64).max
    finite_cells = tight = 0
    for r in (nearest_model.R64, nearest_model.R32):
        for batch in range(5):
            n = 10_000
            nr, nmem = rng.integers(1, 17, n), rng.integers(1, 257, n)
            scale = 10.0 ** rng.uniform(-3, 5, n)
            gap = rng.uniform(0.0, 6.0, n) * (rng.random(n) < 0.8)  # (a fifth of the tiles lie on the block)
            direction = rng.normal(size=(n, 3))
            direction /= np.linalg.norm(direction, axis=1, keepdims=True)
            of_row, of_member = np.repeat(np.arange(n), nr), np.repeat(np.arange(n), nmem)
            lo = rng.uniform(-1.0, 1.0, (len(of_row), 3)) * scale[of_row, None]
            rows = np.concatenate([lo, lo + rng.uniform(0.0, 1.0, lo.shape) * scale[of_row, None]], axis=1)
            lo = (rng.uniform(-1.0, 1.0, (len(of_member), 3)) + (gap[:, None] * direction)[of_member]) * scale[of_member, None]
            members = np.concatenate([lo, lo + rng.uniform(0.0, 1.0, lo.shape) * scale[of_member, None]], axis=1)
            Lt, least, none = _property(harness, pkg, np.split(rows, np.cumsum(nr)[:-1]), np.split(members, np.cumsum(nmem)[:-1]), r)
            assert np.all(Lt <= least)
            assert np.all(np.isneginf(Lt[none]))
            finite_cells += int(np.isfinite(Lt).sum())
            ok = np.isfinite(Lt) & (nr * nmem == 1)  # a cell of one pair: the cell's bound is the pair's, bit for bit
            assert _bits(Lt[ok]) == _bits(least[ok])
            tight += int(ok.sum())
    assert finite_cells > 30_000 and tight > 10
    # by hand
    unit = np.array([0, 0, 0, 1, 1, 1.0])
    two = np.stack([unit, unit + [0, 3, 0, 0, 3, 0]])
    hand = [
        (unit[None], (unit + [1, 0, 0, 1, 0, 0])[None], True),                       # touching: a face
        (unit[None], (unit + [1, 1, 0, 1, 1, 0])[None], True),                       # ... an edge
        (unit[None], (unit + [1, 1, 1, 1, 1, 1])[None], True),                       # ... a corner
        (two, np.stack([unit + 5, unit + [1, 3, 0, 1, 3, 0]]), True),                # one member touches one row
        (two, np.stack([unit + 5, unit + 7]), False),
        (unit[None] * 1e300, (unit * 1e300 + [0, 0, 3e300, 0, 0, 3e300])[None], True),    # 1e300: beyond the coordinates the bound takes
        (unit[None] * 1e140, (unit * 1e140 + [0, 0, 3e140, 0, 0, 3e140])[None], False),   # ... below them
        (unit[None], np.array([[-big, -big, 5, big, big, 5.0]]), True),              # +-DBL_MAX: a Plane
        (np.array([[-big] * 3 + [big] * 3]), (unit + 5)[None], True),
        (two, np.stack([unit + 5, [2, 2, 2, np.inf, 3, 3]]), True),                  # a +inf member
        (two, np.stack([[-np.inf, 5, 5, 6, 6, 6], unit + 5]), True),                 # a -inf member
        (two, np.stack([unit + 5, [5, np.nan, 5, 6, 6, 6]]), True),                  # a NaN member
        (np.stack([unit, [0, 3, np.nan, 1, 4, 1]]), np.stack([unit + 5, unit + 7]), True),  # a NaN row
        (np.stack([unit, [np.nan] * 6]), np.stack([unit + 5, unit + 7]), True),
    ]
    for r in (nearest_model.R64, nearest_model.R32):
        Lt, least, none = _property(harness, pkg, [h[0] for h in hand], [h[1] for h in hand], r)
        assert np.all(Lt <= least) and np.all(np.isneginf(Lt[none]))
        assert np.array_equal(np.isneginf(Lt), np.array([h[2] for h in hand])), Lt
        for k, h in enumerate(hand):  # the numpy model's Lt is the header's, bit for bit
            got = model.tile_bound(h[0], env_model.fold_boxes(h[1]), model.tile_terms(h[1])[0], r)
            assert _bits(got) == _bits(Lt[k]), (k, got, Lt[k])
