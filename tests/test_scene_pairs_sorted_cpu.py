"""The self-collision pairs of a scene by sort and sweep along one axis (include/hppfcl_amd_pairs_sorted.h; library option
scene_pairs_sorted) without a GPU: the header (hpp-fcl_amd/csrc/hfcl_pairs_sorted.hpp) built with g++ (tests/pairs_sorted_harness) -- its
key against a numpy model, its whole pipeline on the host against the model of the list (tests/pairs_model.py) byte for byte on the scenes
of tests/test_scene_pairs_gpu.py, the chunk plan's edges --, the two option names and the new query."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import groups_model
import pairs_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL32, FILL64 = 0xABABABAB, 0xABABABABABABABAB
OBJECTS = [1, 2, 5, 63, 64, 65, 130, 257, 600]  # (tests/test_scene_pairs_gpu.py: OBJECTS x CONFS)
CONFS = [1, 3, 37]
AUTO = 3
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pairs_sorted_harness") / "libpairs_sorted_harness.so")
    src = os.path.join(ROOT, "tests", "pairs_sorted_harness", "pairs_sorted_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-o", out, src])
    d = C.CDLL(out)
    d.psh_self_pairs.restype = C.c_uint64
    d.psh_orderable.restype = C.c_uint32
    d.psh_orderable.argtypes = [C.c_float]
    return d


_SCENES = {}


def _scene(pkg, n_objects, n_conf):
    """Built once, shared, not modified (n_conf = 1: the configurations of the three-configuration scene one by one)."""
    key = (n_objects, max(n_conf, 3))
    if key not in _SCENES:
        if "lib" not in _SCENES:
            _SCENES["lib"] = pairs_model.mixed_library(pkg)
        _SCENES[key] = pairs_model.PairScene(pkg, _SCENES["lib"], key[0], key[1])
        _SCENES[key].check_shares()
    return _SCENES[key]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_options_query_and_header(pkg):
    pkg.engine.build_native()
    lib = pkg.engine.dll()
    keys = pkg.engine.option_keys()
    assert "scene_pairs_sorted" in keys and "scene_pairs_sorted_axis" in keys
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`scene_pairs_sorted`" in doc and "`scene_pairs_sorted_axis`" in doc
    hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_pairs_sorted.h")).read()
    syms = sorted(set(re.findall(r"\b(hfcl_scene_[a-z0-9_]+)\s*\(", hdr)))
    assert syms == sorted(pkg.engine.PAIRS_SORTED_SYMBOLS) == ["hfcl_scene_last_pairs_form"]
    assert hasattr(lib, "hfcl_scene_last_pairs_form") and lib.hfcl_scene_last_pairs_form(None) == -1
    assert hasattr(pkg.engine.Scene, "last_pairs_form")
    pairs_hdr = open(os.path.join(ROOT, "include", "hppfcl_amd_pairs.h")).read()
    assert pairs_hdr.count('#include "hppfcl_amd_pairs_sorted.h"') == 1 and "`scene_pairs_sorted`" in pairs_hdr
    assert "WAIT ON `stream`" in hdr and "QUADRATIC" in hdr  # (the contract change and the worst case are written down)
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "hppfcl_amd.h")])
    assert lib.hfcl_abi_version() == 5


# ---- the key ------------------------------------------------------------------------------------------------------------------------
def _model_round_down(x):
    """The largest fp32 number <= x (no NaN): numpy's round-to-nearest conversion, one step down where it went up."""
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
        up = f.astype(np.float64) > x
        f[up] = np.nextafter(f[up], np.float32(-np.inf))
    f[f == 0] = np.float32(0.0)  # (one zero)
    return f


def _model_orderable(f):
    u = f.view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _keys(harness, pkg, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    key, rounded, end = np.zeros(len(x), dtype=np.uint32), np.zeros(len(x), dtype=np.float32), np.zeros(len(x), dtype=np.uint32)
    harness.psh_keys(pkg.abi.ptr(x), C.c_uint64(len(x)), pkg.abi.ptr(key), pkg.abi.ptr(rounded), pkg.abi.ptr(end))
    return key, rounded, end


def _special_values():
    tiny = float(np.finfo(np.float32).tiny)  # the smallest normal fp32 number
    sub = float(np.nextafter(np.float32(0), np.float32(1)))  # the smallest subnormal one
    v = [0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0 - 2.0 ** -30, -1.0 + 2.0 ** -30,
         tiny, -tiny, tiny * (1 - 2.0 ** -30), sub, -sub, sub / 2, -sub / 2, sub * 1.5, -sub * 1.5, 5e-324, -5e-324, 1e-310, -1e-310,
         FLT_MAX, -FLT_MAX, FLT_MAX * (1 + 2.0 ** -30), -FLT_MAX * (1 + 2.0 ** -30), 2.0 ** 128, -2.0 ** 128, 1e300, -1e300,
         np.finfo(np.float64).max, -np.finfo(np.float64).max, 2.0 ** 25 + 1.0, -(2.0 ** 25) - 1.0, 2.0 ** 25 + 5.5]
    return np.array(v, dtype=np.float64)


def test_key_against_the_numpy_model(pkg, harness):
    rng = np.random.default_rng(17)
    x = np.concatenate([_special_values(), rng.normal(0, 1, 4000), rng.normal(0, 1, 2000) * 10.0 ** rng.integers(-45, 45, 2000),
                        rng.integers(-2 ** 26, 2 ** 26, 1000) + rng.random(1000)])
    key, rounded, end = _keys(harness, pkg, x)
    model = _model_round_down(x)
    # float(key) <= min, and it is the LARGEST such fp32 number: the header's key is the model's
    assert np.all(rounded.astype(np.float64) <= x)
    assert rounded.tobytes() == model.tobytes()
    assert key.tobytes() == _model_orderable(model).tobytes()
    with np.errstate(over="ignore"):
        above = np.nextafter(rounded, np.float32(np.inf)).astype(np.float64)
    assert np.all((above > x) | np.isposinf(rounded))
    # the window end of a value is the key of the same value: float(k) <= hi  <=>  k <= end
    assert end.tobytes() == key.tobytes()
    # the uint32 map is monotone, strictly on distinct floats, and one key for the two zeros
    order = np.argsort(x, kind="stable")
    assert np.all(np.diff(key[order].astype(np.int64)) >= 0)
    f = np.unique(np.concatenate([model, -model, np.array([np.inf, -np.inf, 0.0], dtype=np.float32)]))
    k = np.array([harness.psh_orderable(float(v)) for v in f], dtype=np.int64)
    assert np.all(np.diff(k) > 0)
    z = _keys(harness, pkg, [0.0, -0.0])
    assert z[0][0] == z[0][1] == 0x80000000 and z[2][0] == z[2][1] and np.signbit(z[1]).sum() == 0
    # the specials: a NaN min sorts first, a NaN max ends the window last; beyond FLT_MAX: FLT_MAX below, -inf above
    n = _keys(harness, pkg, [np.nan, -np.inf, np.inf, 1e300, -1e300, FLT_MAX, -FLT_MAX, 5e-324, -5e-324])
    assert n[0][0] == n[0][1] == 0x007FFFFF and n[2][0] == n[2][2] == 0xFF800000
    assert np.isneginf(n[1][0]) and n[1][3] == np.float32(FLT_MAX) and np.isneginf(n[1][4]) and n[1][5] == np.float32(FLT_MAX) and n[1][6] == np.float32(-FLT_MAX)
    assert n[1][7] == 0 and n[1][8] == -np.nextafter(np.float32(0), np.float32(1))  # (a subnormal double: +0 below, the first fp32 subnormal above)
    assert np.all(key >= 0x007FFFFF) and np.all(key <= 0xFF800000)


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------
def _header_pairs(harness, pkg, boxes, inflate, chunk_rows=0, axis=AUTO, groups=None, capacity=None, count_only=False):
    n_conf, n = boxes.shape[:2]
    cap = max(n_conf * n * (n - 1) // 2, 1) if capacity is None else capacity
    pairs = np.full((max(cap, 1) + 3, 2), FILL32, dtype=np.uint32)  # (three guard entries)
    cb = np.full(n_conf + 1, FILL64, dtype=np.uint64)
    axes = np.full(max(n_conf, 1), 9, dtype=np.uint32)
    n_chunks = C.c_uint64(0)
    b = np.ascontiguousarray(boxes, dtype=np.float64)
    g, w = (None, None) if groups is None else (np.ascontiguousarray(groups[0], dtype=np.uint8), np.zeros(64, dtype=np.uint64))
    if groups is not None:
        w[:len(groups[1])] = groups[1]
    got = harness.psh_self_pairs(pkg.abi.ptr(b), C.c_uint32(n), C.c_uint64(n_conf), C.c_double(inflate), C.c_uint64(chunk_rows), C.c_uint32(axis),
                                 None if g is None else pkg.abi.ptr(g), None if w is None else pkg.abi.ptr(w),
                                 None if count_only else pkg.abi.ptr(pairs), C.c_uint64(cap), pkg.abi.ptr(cb), C.byref(n_chunks), pkg.abi.ptr(axes))
    return pairs, cb, int(got), int(n_chunks.value), axes


def _cases(sc, n_conf, f32, inflate):
    """(boxes, expected pairs, expected conf_begin): the whole scene, or its first three configurations one by one."""
    boxes = sc.boxes32 if f32 else sc.boxes
    pairs, cb = sc.expected(f32, inflate)
    if n_conf > 1:
        return [(boxes, pairs, cb)]
    return [(boxes[c:c + 1], np.ascontiguousarray(pairs[int(cb[c]):int(cb[c + 1])]), (cb[c:c + 2] - cb[c]).astype(np.uint64)) for c in range(3)]


@pytest.mark.parametrize("n_conf", CONFS)
@pytest.mark.parametrize("n_objects", OBJECTS)
def test_pipeline_equals_the_model(pkg, harness, n_objects, n_conf):
    """keys, std::stable_sort, windows, emit, sort == pairs_model's list, byte for byte; every axis; whole and in chunks of one configuration."""
    sc = _scene(pkg, n_objects, n_conf)
    for f32, inflate in ((False, 0.0), (False, 0.25), (True, 0.0), (True, 0.25)):
        for boxes, exp, exp_cb in _cases(sc, n_conf, f32, inflate):
            for axis, chunk_rows in ((AUTO, 0), (0, 0), (1, 40), (2, 0), (AUTO, 40)) if not f32 else ((AUTO, 0),):
                pairs, cb, n, n_chunks, axes = _header_pairs(harness, pkg, boxes, inflate, chunk_rows, axis)
                what = (n_objects, len(boxes), f32, inflate, axis, chunk_rows)
                assert n == len(exp), what
                assert pairs[:n].tobytes() == exp.tobytes() and cb.tobytes() == exp_cb.tobytes(), what
                assert np.all(pairs[n:] == FILL32), what
                if n_objects >= 2:
                    per = min(len(boxes), max(chunk_rows // n_objects, 1)) if chunk_rows else len(boxes)  # (whole configurations, at least one)
                    assert n_chunks == -(-len(boxes) // per), what
                    assert np.all(axes[:len(boxes)] == axis) if axis < 3 else np.all(axes[:len(boxes)] < 3), what


def test_automatic_axis(pkg, harness):
    """The axis on which the centres spread widest; ties to the lowest; boxes without a finite centre do not count."""
    rng = np.random.default_rng(3)
    for axis in range(3):
        lo = rng.uniform(-1, 1, (1, 50, 3))
        lo[..., axis] *= 7.0
        boxes = np.concatenate([lo, lo + 0.5], axis=2)
        assert _header_pairs(harness, pkg, boxes, 0.0)[4][0] == axis
        boxes[0, 3, (axis + 1) % 3] = -np.inf  # an unbounded box
        boxes[0, 4, (axis + 2) % 3 + 3] = np.nan
        assert _header_pairs(harness, pkg, boxes, 0.0)[4][0] == axis
    cube = np.array([[[0, 0, 0, 1, 1, 1.0], [4, 4, 4, 5, 5, 5.0]]])
    assert _header_pairs(harness, pkg, cube, 0.0)[4][0] == 0
    cube[0, 1, [0, 3]] -= 1.0
    assert _header_pairs(harness, pkg, cube, 0.0)[4][0] == 1
    nothing = np.full((1, 3, 6), np.nan)
    pairs, cb, n, _, axes = _header_pairs(harness, pkg, nothing, 0.0)
    assert axes[0] == 0 and n == 3  # (NaN boxes keep every pair)


def _lattice(shift=0.0, axis=0):
    k = np.arange(6.0)
    lo = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(1, 216, 3)
    lo = lo[:, np.random.default_rng(8).permutation(216)]
    lo[..., axis] += shift
    return np.concatenate([lo, lo + 1.0], axis=2)


def test_special_boxes(pkg, harness):
    """Unbounded boxes, NaNs, a lattice of unit boxes that touch exactly (closed intervals, hundreds of equal keys), the lattice shifted by
    2^25 (the fp32 keys of neighbours collapse), a pair meeting at -0.0 / +0.0, boxes beyond FLT_MAX: the model's list on every axis."""
    sc = _scene(pkg, 130, 3)
    cases = {}
    b = sc.boxes.copy()
    b[:, 17, :3], b[:, 17, 3:] = -np.inf, np.inf  # a tilted Plane's box
    b[2, 40, 0], b[2, 41, 4] = -np.inf, np.inf
    cases["unbounded"] = b
    b = sc.boxes.copy()
    b[0, 7, 1] = np.nan
    b[2, 9, 3] = np.nan
    b[2, 11, 0] = np.nan
    b[2, 12] = np.nan
    cases["nan"] = b
    cases["lattice"] = _lattice()
    for axis in range(3):
        cases["lattice shifted on %d" % axis] = _lattice(2.0 ** 25, axis)
    cases["zeros"] = np.array([[[-1, 0, 0, -0.0, 1, 1], [0.0, 0, 0, 1, 1, 1], [-3, -0.0, 0, -2, 1, 1], [5, -1, 0, 6, -0.0, 1], [5, 0.0, 0, 6, 1, 1.0]]])
    cases["huge"] = np.array([[[1e300, 0, 0, 1.5e300, 1, 1], [1.2e300, 0, 0, 1.3e300, 1, 1], [-1.5e300, 0, 0, -1e300, 1, 1], [-1.2e300, 0, 0, -1.1e300, 1, 1],
                               [1.6e300, 0, 0, 1.7e300, 1, 1], [FLT_MAX, 0, 0, 1e39, 1, 1], [1e39, 0, 0, 1e40, 1, 1.0]]])
    for name, boxes in cases.items():
        for inflate in (0.0, 0.25):
            exp, exp_cb = pairs_model.self_pairs(boxes, inflate)
            for axis, chunk_rows in ((AUTO, 0), (0, 0), (1, 0), (2, 1)):
                pairs, cb, n, _, _ = _header_pairs(harness, pkg, boxes, inflate, chunk_rows, axis)
                assert n == len(exp) and pairs[:n].tobytes() == exp.tobytes() and cb.tobytes() == exp_cb.tobytes(), (name, inflate, axis)
    exp, _ = pairs_model.self_pairs(cases["lattice"], 0.0)
    assert len(exp) == (16 ** 3 - 216) // 2  # (per axis a box meets itself and its neighbours: 2 + 3 + 3 + 3 + 3 + 2 of 6 positions)
    assert [tuple(p) for p in pairs_model.self_pairs(cases["zeros"], 0.0)[0]] == [(0, 1), (3, 4)]
    assert len(pairs_model.self_pairs(cases["nan"], 0.0)[0]) > len(sc.expected()[0])
    # with inflate 0 and no NaN the list is the host broadphase's
    for name in ("unbounded", "lattice", "lattice shifted on 0", "zeros"):
        boxes = cases[name]
        pairs, cb, n, _, _ = _header_pairs(harness, pkg, boxes, 0.0)
        for c in range(len(boxes)):
            host = pkg.engine.broadphase_self_pairs(boxes[c])
            assert pairs[int(cb[c]):int(cb[c + 1])].tobytes() == host.astype(np.uint32).tobytes(), (name, c)


def test_groups_count_only_and_capacity(pkg, harness):
    sc = _scene(pkg, 130, 3)
    exp, exp_cb = sc.expected(False, 0.25)
    layouts = groups_model.layouts(130)
    # a matrix that is NOT symmetric: the rule is about i < j -- bit group[j] of collides[group[i]] -- whichever comes first in the sweep
    m = np.random.default_rng(5).random((8, 8)) < 0.5
    layouts.append(("asymmetric", np.random.default_rng(6).integers(0, 8, 130).astype(np.uint8), groups_model.words_of(m)))
    assert not np.array_equal(m, m.T)
    for name, group, words in layouts:
        e, e_cb = groups_model.filter_list(exp, exp_cb, group, words)
        for axis, chunk_rows in ((AUTO, 0), (1, 130)):
            pairs, cb, n, _, _ = _header_pairs(harness, pkg, sc.boxes, 0.25, chunk_rows, axis, groups=(group, words))
            assert n == len(e) and pairs[:n].tobytes() == e.tobytes() and cb.tobytes() == e_cb.tobytes(), (name, axis)
    pairs, cb, n, _, _ = _header_pairs(harness, pkg, sc.boxes, 0.25, 130, count_only=True)
    assert n == len(exp) and cb.tobytes() == exp_cb.tobytes() and np.all(pairs == FILL32)
    cap = len(exp) // 2
    pairs, cb, n, _, _ = _header_pairs(harness, pkg, sc.boxes, 0.25, 130, capacity=cap)
    assert n == len(exp) and pairs[:cap].tobytes() == exp[:cap].tobytes() and np.all(pairs[cap:] == FILL32) and cb.tobytes() == exp_cb.tobytes()


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def _plan(harness, n, n_conf, option):
    out = np.zeros(6, dtype=np.uint64)
    harness.psh_plan(C.c_uint32(n), C.c_uint64(n_conf), C.c_uint64(option), out.ctypes.data_as(C.c_void_p))
    return dict(zip(("conf_per_chunk", "n_chunks", "chunk_rows", "blocks_per_conf", "conf_bits", "obj_bits"), (int(v) for v in out)))


def test_chunk_plan_edges(harness):
    bits = lambda count: max(int(count) - 1, 0).bit_length()  # noqa: E731
    for n, n_conf, option in ((2, 1, 0), (2, 37, 0), (2, 37, 1), (2, 37, 5), (130, 3, 40), (130, 3, 130), (130, 3, 259), (130, 3, 260), (130, 37, 1000),
                              (64, 3, 0), (65, 1, 0), (600, 37, 0), (100000, 1, 0), (100000, 64, 0), (100000, 64, 1 << 31), (1 << 22, 1, 0), (1 << 22, 3, 0),
                              (1 << 22, 3, 1 << 31), (3, 1 << 20, 0), (2, 1 << 21, 0), (2, 1 << 21, 1 << 31), (70000, 1, 40), (16, 2048, 0), (17, 5, 16)):
        p = _plan(harness, n, n_conf, option)
        what = (n, n_conf, option, p)
        rows = option or (1 << 20)
        # whole configurations, at least one, no more than the call has; every configuration in exactly one chunk
        assert 1 <= p["conf_per_chunk"] <= n_conf, what
        assert p["n_chunks"] == -(-n_conf // p["conf_per_chunk"]), what
        assert p["chunk_rows"] == p["conf_per_chunk"] * n, what
        # the option's rows are kept unless one configuration alone is more; a chunk's rows fit 32 bits
        assert p["chunk_rows"] <= max(rows, n) and p["chunk_rows"] < 1 << 32, what
        if option:
            assert p["conf_per_chunk"] == min(n_conf, max(option // n, 1)), what
        else:  # automatic: equal chunks
            assert p["conf_per_chunk"] * p["n_chunks"] < n_conf + p["n_chunks"], what
        assert p["blocks_per_conf"] == -(-n // 16), what
        assert p["conf_per_chunk"] * p["blocks_per_conf"] < 1 << 31, what  # (a grid of workgroups)
        # the bits in use: both sorted words fit 64 bits
        assert p["conf_bits"] == bits(p["conf_per_chunk"]) and p["obj_bits"] == bits(n), what
        assert 32 + p["conf_bits"] <= 64 and p["conf_bits"] + 2 * p["obj_bits"] <= 64, what
