"""The self-collision pairs of a scene by sort and sweep along one axis on the GPU (include/hppfcl_amd_pairs_sorted.h; library option
scene_pairs_sorted).  The yardsticks are the ones of tests/test_scene_pairs_gpu.py -- the numpy model of the list (tests/pairs_model.py),
byte for byte --, the all-pairs form on the same scene (the option at 0), and the host broadphase on the device's own boxes.  Every test
sets the option and asserts that the list was made by the sorted form (Scene.last_pairs_form() == 2); on a build without the feature the
option key is refused.

Two things the scenes cannot do.  engine.groups_excluding takes scenes of at most 64 objects (one group per object), so the groups of
the 65, 257 and 600 object scenes are engine.groups_between's and groups_excluding has a scene of 64.  A world box has no bound of -0.0
(a box of non-zero size at a pose: lo + t is +0.0 when it is zero), so the boxes here meet at +0.0 and the mixed zeros are the header's
test (tests/test_scene_pairs_sorted_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import groups_model
import pairs_model

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
FILL = 0x5A5A5A5A5A5A5A5A
FILL32 = 0x5A5A5A5A
OBJECTS = [1, 2, 5, 63, 64, 65, 130, 257, 600]
CONFS = [1, 3, 37]
NO_PAIRS = np.zeros((0, 2), dtype=np.uint32)
SORTED, AUTO = 2, 3


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _same(a, b, what):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def _sorted_on(lib, on=1, axis=AUTO, chunk=0):
    lib.set_option("scene_pairs_sorted", on)
    lib.set_option("scene_pairs_sorted_axis", axis)
    lib.set_option("scene_cull_chunk", chunk)


@pytest.fixture(scope="module")
def world(pkg, torch_cuda):
    """One library (cfg5's mix) with the option set and, per (n_objects, n_conf), the model's scene and the device scene.  Made once,
    shared; a test that changes an option or a scene's groups puts them back."""
    L = pairs_model.mixed_library(pkg)
    lib = pkg.Library(L)
    _sorted_on(lib)
    made = {}

    def get(n_objects, n_conf):
        key = (n_objects, max(n_conf, 3))  # (n_conf = 1: the configurations of the three-configuration scene one by one)
        if key not in made:
            ps = pairs_model.PairScene(pkg, L, key[0], key[1])
            ps.check_shares()
            made[key] = (ps, lib.scene(ps.obj_shape, NO_PAIRS))
        return made[key]

    yield dict(lib=lib, L=L, get=get)
    for _, scene in made.values():
        scene.close()
    lib.close()


def _tables(ps, n_conf, f32):
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
    return pairs, d_cb.cpu().numpy().view(np.uint64), int(d_n.cpu().numpy()[0])


# ---- 1. the list is the model's ---------------------------------------------------------------------------------------------------------
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
                assert n_objects < 2 or scene.last_pairs_form() == SORTED, what
                _same(pairs, exp, "host form pairs: " + what)
                _same(cb, exp_cb, "host form conf_begin: " + what)
                got, cb, n = _pairs_device(torch_cuda, scene, table, inflate, len(exp), f32)
                assert n_objects < 2 or scene.last_pairs_form() == SORTED, what
                assert n == len(exp), what
                _same(np.ascontiguousarray(got[:n]), exp, "device form pairs: " + what)
                _same(cb, exp_cb, "device form conf_begin: " + what)
                assert np.all(got[n:] == FILL32), what


# ---- 2. the two forms agree ----------------------------------------------------------------------------------------------------------------
def _both_forms(lib, scene, call):
    """call() with the option at 1 and at 0 on the same scene; the forms that ran."""
    try:
        _sorted_on(lib, 1)
        a = call()
        form_a = scene.last_pairs_form()
        _sorted_on(lib, 0)
        b = call()
        form_b = scene.last_pairs_form()
    finally:
        _sorted_on(lib, 1)
    assert form_a == SORTED and form_b in (0, 1)
    return a, b


@pytest.mark.parametrize("n_objects", [64, 65, 257, 600])
def test_sorted_and_all_pairs_forms_agree(pkg, torch_cuda, world, n_objects):
    """Without groups, with engine.groups_between (two managers) and -- 64 objects: one group per object -- engine.groups_excluding."""
    lib = world["lib"]
    ps, scene = world["get"](n_objects, 3)
    layouts = [None, pkg.engine.groups_between(n_objects // 3, n_objects - n_objects // 3), pkg.engine.groups_between(1, n_objects - 1)]
    if n_objects <= 64:
        rng = np.random.default_rng(2)
        layouts.append(pkg.engine.groups_excluding(n_objects, rng.integers(0, n_objects, (300, 2))))
    try:
        for layout in layouts:
            if layout is None:
                scene.clear_groups()
            else:
                scene.set_groups(*layout)
            for f32, inflate in ((False, 0.0), (True, 0.25)):
                table = ps.pose if f32 else ps.tf
                (p1, cb1), (p0, cb0) = _both_forms(lib, scene, lambda: scene.self_pairs(table, inflate))
                what = "%d objects, groups %s, f32 %d" % (n_objects, "none" if layout is None else len(layout[1]), f32)
                _same(p1, p0, "pairs: " + what)
                _same(cb1, cb0, "conf_begin: " + what)
                exp, exp_cb = ps.expected(f32, inflate)
                if layout is not None:
                    exp, exp_cb = groups_model.filter_list(exp, exp_cb, layout[0], layout[1])
                    assert 0 < len(exp) < len(ps.expected(f32, inflate)[0])
                _same(p1, exp, "the model's pairs: " + what)
                _same(cb1, exp_cb, "the model's conf_begin: " + what)
                exp_len = len(exp)
                got, cb, n = _pairs_device(torch_cuda, scene, table, inflate, exp_len, f32)
                assert n == exp_len and scene.last_pairs_form() == SORTED
                _same(np.ascontiguousarray(got[:n]), exp, "device form: " + what)
                assert np.all(got[n:] == FILL32)
    finally:
        scene.clear_groups()


@pytest.mark.parametrize("kind,f32", [("collide", False), ("distance", False), ("collide", True), ("distance", True)])
def test_self_forms_write_the_same_bytes(pkg, torch_cuda, world, kind, f32):
    """collide_self / distance_self at 130 objects x 3 configurations: records, summaries, pairs and conf_begin in both settings."""
    lib, abi = world["lib"], pkg.abi
    ps, scene = world["get"](130, 3)
    table = ps.pose if f32 else ps.tf
    req = abi.default_distance_request() if kind == "distance" else abi.default_collision_request()
    if kind == "collide":
        req.security_margin = 0.05
    host = scene.distance_self if kind == "distance" else scene.collide_self
    for records in (True, False):
        a, b = _both_forms(lib, scene, lambda: host(table, req, 0.25, records=records))
        exp, exp_cb = ps.expected(f32, 0.25)
        _same(a[1], exp, "pairs")
        _same(a[2], exp_cb, "conf_begin")
        for x, y, what in zip(a, b, ("records", "pairs", "conf_begin", "summaries")):
            if x is None:
                assert y is None and not records
            else:
                _same(x, y, "%s %s records %d" % (kind, what, records))
        assert a[3]["min_pair"][1] != NONE and a[3]["min_pair"][0] == NONE and len(a[1]) > 8385


# ---- 3. axis and chunks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_objects,n_conf", [(5, 37), (65, 3), (130, 37), (600, 3)])
def test_list_does_not_depend_on_axis_or_chunks(pkg, torch_cuda, world, n_objects, n_conf):
    """scene_cull_chunk 40: chunks of one configuration (whole configurations, at least one; 5 objects: eight)."""
    lib = world["lib"]
    ps, scene = world["get"](n_objects, n_conf)
    try:
        for f32, inflate in ((False, 0.0), (True, 0.25)):
            exp, exp_cb = ps.expected(f32, inflate)
            for axis in (0, 1, 2, AUTO):
                for chunk in (0, 40):
                    _sorted_on(lib, 1, axis, chunk)
                    what = "axis %d chunk %d f32 %d" % (axis, chunk, f32)
                    pairs, cb = scene.self_pairs(ps.pose if f32 else ps.tf, inflate)
                    assert scene.last_pairs_form() == SORTED
                    _same(pairs, exp, "pairs, " + what)
                    _same(cb, exp_cb, "conf_begin, " + what)
            got, cb, n = _pairs_device(torch_cuda, scene, ps.pose if f32 else ps.tf, inflate, len(exp), f32)  # (axis AUTO, chunks of 40)
            assert n == len(exp)
            _same(np.ascontiguousarray(got[:n]), exp, "device form in chunks")
            _same(cb, exp_cb, "device form conf_begin in chunks")
    finally:
        _sorted_on(lib)
    with pytest.raises(pkg.EngineError):
        lib.set_option("scene_pairs_sorted_axis", 4)


# ---- 4. special cases ------------------------------------------------------------------------------------------------------------------------
def _against_both(pkg, lib, scene, tf, inflates=(0.0, 0.25), broadphase=True):
    """The sorted form on every axis against the all-pairs form, and -- no NaN -- against the host broadphase on the device's own boxes."""
    out = None
    for inflate in inflates:
        (p1, cb1), (p0, cb0) = _both_forms(lib, scene, lambda: scene.self_pairs(tf, inflate))
        _same(p1, p0, "pairs, inflate %g" % inflate)
        _same(cb1, cb0, "conf_begin, inflate %g" % inflate)
        try:
            for axis in (0, 1, 2):
                for chunk in (0, 1):
                    _sorted_on(lib, 1, axis, chunk)
                    p, cb = scene.self_pairs(tf, inflate)
                    assert scene.last_pairs_form() == SORTED
                    _same(p, p0, "pairs, axis %d chunk %d inflate %g" % (axis, chunk, inflate))
                    _same(cb, cb0, "conf_begin, axis %d chunk %d inflate %g" % (axis, chunk, inflate))
        finally:
            _sorted_on(lib)
        if inflate == 0.0:
            out = (p1, cb1)
            if broadphase:
                boxes = scene.world_aabbs(tf)
                assert not np.isnan(boxes).any()
                for c in range(len(tf)):
                    host = pkg.engine.broadphase_self_pairs(boxes[c]).astype(np.uint32)
                    _same(np.ascontiguousarray(p1[int(cb1[c]):int(cb1[c + 1])]), np.ascontiguousarray(host.reshape(-1, 2)), "the host broadphase, configuration %d" % c)
    return out


@pytest.mark.parametrize("n_obj", [40, 70])
def test_mesh_and_plane_scene(pkg, torch_cuda, n_obj):
    """The scene of tests/test_scene_pairs_gpu.py::test_mesh_and_plane_scene: a Plane that is not aligned with an axis has an unbounded
    box -- its window is the whole configuration on every axis -- and a mesh has the box of its vertices."""
    wl = pkg.workloads
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
    scene = lib.scene(obj_shape, NO_PAIRS)
    try:
        boxes = scene.world_aabbs(tf)
        exp, exp_cb = pairs_model.self_pairs(boxes, 0.0)
        assert np.isinf(boxes[:, 17]).any() and (exp == i_mesh).any()
        for c in range(n_conf):
            mine = exp[int(exp_cb[c]):int(exp_cb[c + 1])]
            assert ((mine == 17).any(axis=1)).sum() == n_obj - 1, c
        pairs, cb = _against_both(pkg, lib, scene, tf)
        _same(pairs, exp, "the model's pairs")
        _same(cb, exp_cb, "the model's conf_begin")
    finally:
        scene.close()
        lib.close()


def test_a_pose_row_with_a_nan(pkg, torch_cuda, world):
    """A NaN keeps a pair unless a comparison separates it: a NaN translation component makes two NaN bounds, a NaN rotation six."""
    lib = world["lib"]
    ps, scene = world["get"](130, 3)
    tf = ps.tf.copy()
    tf[0, 7, 10] = np.nan  # configuration 0 has no pair without it
    tf[2, 9, 9] = np.nan
    tf[2, 100, :9] = np.nan
    boxes = scene.world_aabbs(tf)
    assert np.isnan(boxes[0, 7]).sum() == 2 and np.isnan(boxes[2, 100]).all()
    exp, exp_cb = pairs_model.self_pairs(boxes, 0.0)
    assert exp_cb[1] >= 1 and ((exp[int(exp_cb[2]):] == 100).any(axis=1)).sum() == 129
    pairs, cb = _against_both(pkg, lib, scene, tf, broadphase=False)
    _same(pairs, exp, "the model's pairs")
    _same(cb, exp_cb, "the model's conf_begin")


def _lattice_scene(pkg):
    """216 unit boxes on a 6 x 6 x 6 lattice, identity rotations: the world boxes are exact and touch exactly; in a shuffled order."""
    L = pkg.geometry.ShapeLibrary()
    L.add_box(1.0, 1.0, 1.0)
    k = np.arange(6.0)
    T = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(216, 3) + 0.5
    return L, T[np.random.default_rng(8).permutation(216)]


def test_lattices_and_zero(pkg, torch_cuda):
    """Closed intervals and hundreds of equal keys (36 boxes share every key of the lattice); the lattice shifted by 2^25 along each axis
    in turn -- the fp32 keys of neighbours collapse: a spacing of 1 is below the fp32 spacing of 4 there --; boxes that meet at 0.0."""
    L, T = _lattice_scene(pkg)
    shifted = [T + 2.0 ** 25 * np.eye(3)[axis] for axis in range(3)]
    tf = pkg.geometry.make_pose(T=np.concatenate([T] + shifted)).reshape(4, 216, 12)
    lib = pkg.Library(L)
    scene = lib.scene(np.zeros(216, dtype=np.uint32), NO_PAIRS)
    try:
        boxes = scene.world_aabbs(tf)
        assert np.array_equal(boxes[0, :, 3:] - boxes[0, :, :3], np.ones((216, 3))) and np.array_equal(boxes[1, :, 0], boxes[0, :, 0] + 2.0 ** 25)
        assert len(np.unique(boxes[1, :, 0].astype(np.float32))) < 6  # (collapsed)
        pairs, cb = _against_both(pkg, lib, scene, tf, inflates=(0.0,))
        assert list(np.diff(cb.astype(np.int64))) == [(16 ** 3 - 216) // 2] * 4  # (every box meets its up to 26 neighbours)
    finally:
        scene.close()
    # [-1, 0] and [0, 1] on x, [-2, 0] and [0, 0.5] on y, a box around the origin, one apart
    tz = np.array([[-0.5, 0.25, 0], [0.5, 0.25, 0], [10, -1.0, 0], [10, 0.25, 0], [0, 0, 0], [3, 3, 3.0]])
    L.add_box(1.0, 2.0, 1.0)
    L.add_box(1.0, 0.5, 1.0)
    lib2 = pkg.Library(L)
    scene = lib2.scene(np.array([0, 0, 1, 2, 0, 0], dtype=np.uint32), NO_PAIRS)
    try:
        tf = pkg.geometry.make_pose(T=tz).reshape(1, 6, 12)
        boxes = scene.world_aabbs(tf)
        assert boxes[0, 0, 3] == 0.0 == boxes[0, 1, 0] and boxes[0, 2, 4] == 0.0 == boxes[0, 3, 1]
        pairs, cb = _against_both(pkg, lib2, scene, tf, inflates=(0.0,))
        assert [tuple(p) for p in pairs] == [(0, 1), (0, 4), (1, 4), (2, 3)]
    finally:
        scene.close()
        lib2.close()
        lib.close()


# ---- 5. count only, short capacity, refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_objects", [5, 64, 257])
def test_count_only_and_short_capacity(pkg, torch_cuda, world, n_objects):
    ps, scene = world["get"](n_objects, 3)
    exp, exp_cb = ps.expected(False, 0.0)
    got, cb, n = _pairs_device(torch_cuda, scene, ps.tf, 0.0, 0, count_only=True)
    assert n == len(exp) and np.all(got == FILL32) and scene.last_pairs_form() == SORTED
    _same(cb, exp_cb, "count-only conf_begin")
    n_host = C.c_size_t(0)
    tab = np.ascontiguousarray(ps.tf)
    fn = pkg.engine.dll().hfcl_scene_self_pairs
    assert fn(scene._h, pkg.abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), None, C.c_size_t(0), None, C.byref(n_host)) == 0 and n_host.value == len(exp)
    # a capacity below the count.  Device form: the count is true, the entries below the capacity are right, the words behind it untouched --
    # whole and in chunks of one configuration (the capacity ends inside a chunk; the last chunk lies behind it)
    cap = len(exp) // 2
    try:
        for chunk in (0, 1):
            _sorted_on(world["lib"], 1, AUTO, chunk)
            got, cb, n = _pairs_device(torch_cuda, scene, ps.tf, 0.0, cap)
            assert n == len(exp) and len(got) == cap + 4
            _same(np.ascontiguousarray(got[:cap]), np.ascontiguousarray(exp[:cap]), "pairs below the capacity")
            assert np.all(got[cap:] == FILL32)
            _same(cb, exp_cb, "conf_begin with a short capacity")
    finally:
        _sorted_on(world["lib"])
    # host form: HFCL_ERR_LIMIT, the count set, the buffers untouched
    pairs = np.full((cap, 2), FILL32, dtype=np.uint32)
    cbh = np.full(4, FILL, dtype=np.uint64)
    rc = fn(scene._h, pkg.abi.ptr(tab), C.c_size_t(3), C.c_double(0.0), pkg.abi.ptr(pairs), C.c_size_t(cap), pkg.abi.ptr(cbh), C.byref(n_host))
    assert rc == pkg.abi.ERR_LIMIT and n_host.value == len(exp) and np.all(pairs == FILL32) and np.all(cbh == FILL)
    assert scene.last_pairs_form() == SORTED


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
    lib = pkg.Library(L, options={"scene_pairs_sorted": 1})
    stale = lib.scene(ps.obj_shape, NO_PAIRS)
    try:
        pairs, _ = stale.self_pairs(ps.tf, 0.0)
        assert stale.last_pairs_form() == SORTED and pairs.tobytes() == ps.expected()[0].tobytes()
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


# ---- 6. indices above 2^16 ---------------------------------------------------------------------------------------------------------------
def test_seventy_thousand_objects(pkg, torch_cuda):
    """70 000 objects of cfg5's mix in a cube of side 72, one configuration: 229 415 pairs (counted on the host when the seed was chosen),
    28 357 of them with an index of 2^16 or more; the list is the host broadphase's on the host's boxes, entry for entry."""
    b = pkg.workloads.cfg5_broadphase_scene(n_objects=70000, target_pairs=200000, seed=7, nper=16)
    sc = b.scene
    exp = np.ascontiguousarray(sc["pairs"].astype(np.uint32))
    assert len(exp) == 229415 and (exp >= 65536).any(axis=1).sum() == 28357
    lib = pkg.Library(b.lib, options={"scene_pairs_sorted": 1})
    scene = lib.scene(sc["obj_shape"], NO_PAIRS)
    try:
        tf = sc["obj_tf"].reshape(1, 70000, 12)
        _same(scene.world_aabbs(tf).reshape(-1, 6), sc["aabbs"], "the device's boxes are the host's")
        pairs, cb = scene.self_pairs(tf, 0.0)
        assert scene.last_pairs_form() == SORTED
        _same(pairs, exp, "pairs")
        assert list(cb) == [0, len(exp)]
        got, cb, n = _pairs_device(torch_cuda, scene, tf, 0.0, len(exp))
        assert n == len(exp) and np.all(got[n:] == FILL32)
        _same(np.ascontiguousarray(got[:n]), exp, "device form pairs")
    finally:
        scene.close()
        lib.close()
