"""The bucket populations (hfcl_last_bucket_counts) of the host scene calls across the reuse of the per-chunk count slots.  A host scene
call keeps COUNT_SLOTS = 8 pinned slots; chunk k uses slot k % 8 once chunk k - 8 has been added up.  The scene of
test_scene_gpu.py::test_unsupported_pair_kind -- three shapes, seven objects, 21 pairs, 2 configurations: 42 queries -- in chunks of
0 (one chunk), 6, 5 and 2 queries is 1, 7, 9 and 21 chunks: fewer than eight, one more than eight, more than twice eight.  The yardsticks:
the per-pair host call on the expanded arrays (hfcl_scene_distance, hfcl_scene_collide), the same call in one chunk (the culled form,
hfcl_scene_nearest, and the host forms on lists of pairs made on the device: hfcl_scene_collide_self, hfcl_scene_collide_env,
hfcl_scene_nearest_self, hfcl_scene_nearest_env).  Chunks that run split are covered by the cfg5 scene tests at their size."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CHUNKS = [0, 6, 5, 2]
N_CONF = 2


@pytest.fixture(scope="module")
def small(pkg, torch_cuda):
    abi = pkg.abi
    L = pkg.ShapeLibrary()
    L.add_sphere(0.5)
    L.add_box(0.4, 0.5, 0.6)
    L.add_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0])
    obj_shape = np.array([0, 1, 2, 0, 1, 2, 0], dtype=np.uint32)
    rng = np.random.default_rng(9)
    table = pkg.geometry.make_pose(quat=pkg.workloads.uniform_quaternions(rng, 14), T=rng.uniform(-1, 1, (14, 3))).reshape(N_CONF, 7, 12)
    i, j = np.triu_indices(7, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    lib = pkg.Library(L)
    scene = lib.scene(obj_shape, pairs)

    class S:
        pass
    s = S()
    s.lib, s.scene, s.table, s.n_pairs = lib, scene, np.ascontiguousarray(table), len(pairs)
    s.n_tri = int(((obj_shape[i] == 2) | (obj_shape[j] == 2)).sum())
    # the per-pair host call on the expanded arrays: its return code and its populations, computed once
    s1, s2 = np.tile(obj_shape[i], N_CONF), np.tile(obj_shape[j], N_CONF)
    tf1, tf2 = table[:, i].reshape(-1, 12), table[:, j].reshape(-1, 12)
    s.per_pair = {}
    for kind, call, req in (("distance", lib.distance, abi.default_distance_request()), ("collide", lib.collide, abi.default_collision_request())):
        rc = abi.OK
        try:
            call(s1, s2, tf1, tf2, req)
        except pkg.EngineError as e:
            rc = e.code
        s.per_pair[kind] = (rc, lib.last_bucket_counts())
    yield s
    lib.set_option("scene_chunk", 0)
    scene.close()
    lib.close()


def _chunks_of(n, chunk):
    return 1 if chunk == 0 else -(-n // chunk)


def test_chunk_counts_straddle_the_slots():
    assert [_chunks_of(21 * N_CONF, c) for c in CHUNKS] == [1, 7, 9, 21]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind", ["distance", "collide"])
def test_scene_counts_equal_the_per_pair_call(pkg, small, kind, chunk):
    abi, d = pkg.abi, pkg.engine.dll()
    n = N_CONF * small.n_pairs
    small.lib.set_option("scene_chunk", chunk)
    out = np.zeros(n, dtype=abi.RESULT_DTYPE)
    summ = np.zeros(N_CONF, dtype=abi.SCENE_SUMMARY_DTYPE)
    if kind == "distance":
        req = abi.default_distance_request()
        rc = d.hfcl_scene_distance(small.scene._h, abi.ptr(small.table), C.c_size_t(N_CONF), C.byref(req), abi.ptr(out), abi.ptr(summ), None, None)
    else:
        req = abi.default_collision_request()
        rc = d.hfcl_scene_collide(small.scene._h, abi.ptr(small.table), C.c_size_t(N_CONF), C.byref(req), abi.ptr(out), abi.ptr(summ), None, None)
    counts = small.lib.last_bucket_counts()
    ref_rc, ref_counts = small.per_pair[kind]
    print(kind, chunk, rc, counts)
    assert rc == ref_rc, (kind, chunk, rc, ref_rc)
    assert counts == ref_counts, (kind, chunk)
    if kind == "distance":  # distance() has no TriangleP entries
        assert rc == abi.ERR_UNSUPPORTED_PAIR and counts["unsupported"] == N_CONF * small.n_tri > 0


def _culled(pkg, small, chunk):
    abi, d = pkg.abi, pkg.engine.dll()
    n = N_CONF * small.n_pairs
    small.lib.set_option("scene_chunk", chunk)
    req = abi.default_distance_request()
    out = np.zeros(n, dtype=abi.RESULT_DTYPE)
    ids = np.zeros(n, dtype=np.uint64)
    summ = np.zeros(N_CONF, dtype=abi.SCENE_SUMMARY_DTYPE)
    k = C.c_size_t(0)
    # inflate 10: no box of this scene is that far from another -- every query survives, the list has the chunks of the flat range
    rc = d.hfcl_scene_distance_culled(small.scene._h, abi.ptr(small.table), C.c_size_t(N_CONF), C.c_double(10.0), C.byref(req), abi.ptr(out),
                                      C.c_size_t(n), abi.ptr(ids), None, abi.ptr(summ), None, None, C.byref(k))
    return rc, int(k.value), small.lib.last_bucket_counts()


def _nearest(pkg, small, chunk):
    abi, d = pkg.abi, pkg.engine.dll()
    small.lib.set_option("scene_chunk", chunk)
    req = abi.default_distance_request()
    summ = np.zeros(N_CONF, dtype=abi.SCENE_SUMMARY_DTYPE)
    rec = np.zeros(N_CONF, dtype=abi.RESULT_DTYPE)
    k = (C.c_size_t * 2)(0, 0)
    rc = d.hfcl_scene_nearest(small.scene._h, abi.ptr(small.table), C.c_size_t(N_CONF), C.byref(req), C.c_double(np.inf), abi.ptr(summ),
                              abi.ptr(rec), k)
    return rc, (int(k[0]), int(k[1])), small.lib.last_bucket_counts()


@pytest.fixture(scope="module")
def one_chunk(pkg, small):
    return {"culled": _culled(pkg, small, 0), "nearest": _nearest(pkg, small, 0)}


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("form", ["culled", "nearest"])
def test_listed_counts_equal_the_one_chunk_call(pkg, small, one_chunk, form, chunk):
    abi = pkg.abi
    rc, n_listed, counts = (_culled if form == "culled" else _nearest)(pkg, small, chunk)
    ref_rc, ref_listed, ref_counts = one_chunk[form]
    print(form, chunk, rc, n_listed, counts)
    assert n_listed == ref_listed
    if form == "culled":
        assert n_listed == N_CONF * small.n_pairs
        assert counts["unsupported"] == N_CONF * small.n_tri
    assert rc == ref_rc, (form, chunk, rc, ref_rc)
    assert rc == (abi.ERR_UNSUPPORTED_PAIR if counts["unsupported"] else abi.OK)
    assert counts == ref_counts, (form, chunk)


# ---- the host forms on a list of pairs made on the device, and the clearance calls on such lists -------------------------------------
# collide_self / collide_env at inflate 10 list every pair -- 21 a configuration of the seven objects; 6 + 12 = 18 with the first four
# moving and the other three the environment --: 42 and 36 entries, in chunks of 0, 6, 5, 2 entries 1 / 7 / 9 / 21 and 1 / 6 / 8 / 18 chunks.
# nearest_self / nearest_env (no upper bound): scene_chunk cuts each pass's narrow phase.  The yardstick: the same call in one chunk.
N_MOVING = 4


def _made(pkg, small, chunk, env):
    abi, d = pkg.abi, pkg.engine.dll()
    table = np.ascontiguousarray(small.table[:, :N_MOVING]) if env else small.table
    cap = N_CONF * small.n_pairs
    small.lib.set_option("scene_chunk", chunk)
    req = abi.default_collision_request()
    out = np.zeros(cap, dtype=abi.RESULT_DTYPE)
    pairs = np.zeros((cap, 2), dtype=np.uint32)
    summ = np.zeros(N_CONF, dtype=abi.SCENE_SUMMARY_DTYPE)
    k = C.c_size_t(0)
    fn = d.hfcl_scene_collide_env if env else d.hfcl_scene_collide_self
    rc = fn(small.scene._h, abi.ptr(table), C.c_size_t(N_CONF), C.c_double(10.0), C.byref(req), abi.ptr(out), C.c_size_t(cap), abi.ptr(pairs),
            None, abi.ptr(summ), None, None, C.byref(k))
    return rc, int(k.value), small.lib.last_bucket_counts()


def _clearance(pkg, small, chunk, env):
    abi, d = pkg.abi, pkg.engine.dll()
    table = np.ascontiguousarray(small.table[:, :N_MOVING]) if env else small.table
    small.lib.set_option("scene_chunk", chunk)
    req = abi.default_distance_request()
    out = np.zeros(N_CONF, dtype=abi.SCENE_CLEARANCE_DTYPE)
    rec = np.zeros(N_CONF, dtype=abi.RESULT_DTYPE)
    k = (C.c_size_t * 2)(0, 0)
    fn = d.hfcl_scene_nearest_env if env else d.hfcl_scene_nearest_self
    rc = fn(small.scene._h, abi.ptr(table), C.c_size_t(N_CONF), C.byref(req), C.c_double(np.inf), abi.ptr(out), abi.ptr(rec), k)
    return rc, (int(k[0]), int(k[1])), small.lib.last_bucket_counts()


MADE_FORMS = {"collide_self": (_made, False), "collide_env": (_made, True), "nearest_self": (_clearance, False), "nearest_env": (_clearance, True)}


def _call(pkg, small, form, chunk):
    """the form's call; for the env forms the first N_MOVING objects move and the others stand where configuration 0 has them"""
    call, env = MADE_FORMS[form]
    if env:
        small.scene.set_environment(N_MOVING, np.ascontiguousarray(small.table[0, N_MOVING:]))
    try:
        return call(pkg, small, chunk, env)
    finally:
        if env:
            small.scene.clear_environment()


@pytest.fixture(scope="module")
def made_one_chunk(pkg, small):
    return {form: _call(pkg, small, form, 0) for form in MADE_FORMS}


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("form", list(MADE_FORMS))
def test_made_list_counts_equal_the_one_chunk_call(pkg, small, made_one_chunk, form, chunk):
    abi = pkg.abi
    rc, n_listed, counts = _call(pkg, small, form, chunk)
    ref_rc, ref_listed, ref_counts = made_one_chunk[form]
    print(form, chunk, rc, n_listed, counts)
    assert n_listed == ref_listed
    if form == "collide_self":
        assert n_listed == N_CONF * small.n_pairs
    if form == "collide_env":
        assert n_listed == N_CONF * (N_MOVING * (N_MOVING - 1) // 2 + N_MOVING * (7 - N_MOVING))
    assert sum(counts.values()) > 0
    assert rc == ref_rc, (form, chunk, rc, ref_rc)
    assert rc == (abi.ERR_UNSUPPORTED_PAIR if counts["unsupported"] else abi.OK)
    assert counts == ref_counts, (form, chunk)
