"""The batch dispatcher (hpp-fcl_amd/csrc/hfcl_host_batch.hip: run_batch_one and its stages) at the sizes it branches on, not at workload size.
Every case asserts (a) the kernel names of the last batch, in order (last_kernel_breakdown), against a literal list, and (b) where two
settings of an option only rearrange streams, that the record arrays of the two runs are byte-equal.

Origin of the literal lists: this file was run once against the library of the commit BEFORE the dispatcher became stages (selected with
HFCL_LIB_PATH); the lists below are what that library printed.  The byte-equal pairs were run on that library first as well: each held there.

Every batch goes through the host entry points as ONE chunk (set_host_chunk(n)): the calls wait for their records, so consecutive batches
are synchronised."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOT = {}  # key -> the names of the runs of the test that is running
EXPECTED = {
    'direct fp64 epa_direct_max=0': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'direct fp64 epa_direct_max=4096': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<full>', 'k_unsupported'],
    'direct fp32 epa_direct_max=0': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'direct fp32 epa_direct_max=4096': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'fan fp64 gjk_beside_max=0': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'fan fp64 gjk_beside_max=120000': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'fan fp32 gjk_beside_max=0': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'fan fp32 gjk_beside_max=120000': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'staged fp32 epa_records_aside=0': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa_prepare', 'k_epa<fast>', 'k_epa_records', 'k_epa<full>', 'k_epa_resume_cc', 'k_unsupported'],
    'staged fp32 epa_records_aside=1': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa_prepare', 'k_epa<fast>', 'k_epa_records', 'k_epa<full>', 'k_epa_resume_cc', 'k_unsupported'],
    'staged fp64 epa64_two_streams=0': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'staged fp64 epa64_two_streams=1': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'split 1': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'split 2': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'split 2 gjk_beside_max=1 set late': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<fast>', 'k_epa<full>', 'k_unsupported'],
    'mixed n=300 mesh_beside=0': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_bvh_shape', 'k_bvh_collide', 'k_epa<full>', 'k_unsupported'],
    'mixed n=300 mesh_beside=4': ['k_classify', 'k_bvh_collide', 'k_bvh_shape', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<full>', 'k_unsupported'],
    'mixed n=200 mesh_beside=0': ['k_classify', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_bvh_shape', 'k_bvh_collide', 'k_epa<full>', 'k_unsupported'],
    'mixed n=200 mesh_beside=4': ['k_classify', 'k_bvh_collide', 'k_bvh_shape', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<full>', 'k_unsupported'],
    'distance bvhd_pool=0 shape_dist_pool=0': ['k_classify', 'k_bvh_shape_distance', 'k_bvh_distance', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<full>', 'k_unsupported'],
    'distance bvhd_pool=1 shape_dist_pool=0': ['k_classify', 'k_bvh_shape_distance', 'k_bvh_distance', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<full>', 'k_unsupported'],
    'distance bvhd_pool=0 shape_dist_pool=1': ['k_classify', 'k_bvh_shape_distance', 'k_bvh_distance', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<full>', 'k_unsupported'],
    'distance bvhd_pool=1 shape_dist_pool=1': ['k_classify', 'k_bvh_shape_distance', 'k_bvh_distance', 'k_closed', 'k_gjk_prim', 'k_gjk_cvx<cc>', 'k_gjk_cvx<pc>', 'k_gjk_cvx<cp>', 'k_epa<full>', 'k_unsupported'],
}


@pytest.fixture(scope="module")
def mix(pkg):
    """cfg5's mix (box, sphere, capsule, ellipsoid, convex32: closed forms + the three iterative kinds of buckets, curved shapes among them) at the
    largest size used here; the cases take its first n pairs.  Shared, not modified."""
    return pkg.workloads.cfg5_mixed(n=131072, seed=21, nper=32)


@pytest.fixture(scope="module")
def mixed_library(pkg):
    """Two small meshes (200 triangles each) plus boxes, spheres and a hull -- no Plane / Halfspace, so the pooled distance() forms apply --
    and 300 queries over all pair kinds in both operand orders.  Shared, not modified."""
    wl, geometry = pkg.workloads, pkg.geometry
    rng = np.random.default_rng(77)
    meshes = wl.mesh_variants(2, 10, 10)
    lib = geometry.ShapeLibrary()
    for k, m in enumerate(meshes):
        lib.add_bvh(k, len(m.vertices))
    for s in rng.uniform(0.2, 0.9, (4, 3)):
        lib.add_box(*map(float, s))
    for r in rng.uniform(0.1, 0.6, 4):
        lib.add_sphere(float(r))
    lib.add_convex(wl.fibonacci_sphere(24) * np.array([0.5, 0.4, 0.3]))
    n = 300
    kind = rng.integers(0, 3, n)  # solid x solid, mesh x solid (both operand orders), mesh x mesh
    mesh, solid, swap = rng.integers(0, 2, (2, n)), rng.integers(2, len(lib), (2, n)), rng.random(n) < 0.5
    s1 = np.where(kind == 0, solid[0], np.where((kind == 1) & swap, solid[0], mesh[0]))
    s2 = np.where(kind == 0, solid[1], np.where((kind == 1) & ~swap, solid[1], mesh[1]))
    q1, T1, q2, T2 = wl._poses(rng, n, 1.0)
    b = wl.Batch("dispatch_mixed_library", lib, s1, s2, q1, T1, q2, T2, "collide")
    b.meshes = meshes
    assert all((kind[:200] == k).sum() >= 20 for k in (0, 1, 2))  # (every kind in the first 200 already)
    return b


def _run(pkg, b, n, options, key, f32=False, kind=None, then=None, lib=None):
    """One library (or `lib`), the first n pairs of b twice as one chunk; returns the records of the second call.  Notes the kernel names under
    `key` for _check_names, which every test ends with."""
    wl, abi = pkg.workloads, pkg.abi
    kind = kind or b.kind
    req = abi.default_distance_request() if kind == "distance" else abi.default_collision_request()
    own = lib is None
    if own:
        lib = wl.make_library(pkg, b, options=options)
    try:
        lib.set_host_chunk(n)
        fn = getattr(lib, kind + ("_f32" if f32 else ""))
        p1, p2 = (b.pose1_f32, b.pose2_f32) if f32 else (b.tf1, b.tf2)
        first = fn(b.s1[:n], b.s2[:n], p1[:n], p2[:n], req)
        again = fn(b.s1[:n], b.s2[:n], p1[:n], p2[:n], req)
        names = [k for k, _ in lib.last_kernel_breakdown()]
        GOT[key] = names
        assert first.tobytes() == again.tobytes(), key
        assert not np.any((again["status"] >> 31) & 1), key
        if then is not None:
            then(lib)
        return again
    finally:
        if own:
            lib.close()


def _check_names():
    got = dict(GOT)
    GOT.clear()
    for key, names in got.items():
        print("    %r: %r," % (key, names))  # (the figure before the assertion)
    assert got == {key: EXPECTED.get(key) for key in got}


def _pair(pkg, b, n, option, values, tag, f32=False, equal=True):
    recs = [_run(pkg, b, n, {option: v}, "%s %s=%s" % (tag, option, v), f32=f32) for v in values]
    if equal:
        assert all(r.tobytes() == recs[0].tobytes() for r in recs[1:]), (tag, option)
    return recs


def test_direct_epa(pkg, mix):
    """2 000 pairs: below epa_direct_max every seed goes to the full-capacity tier alone (fp64).  fp32 does not read the option (launch_epa: `direct` is
    fp64 only, its tiers are contracted code), so its two runs are the same launches and the same bytes."""
    recs = _pair(pkg, mix, 2000, "epa_direct_max", (0, 4096), "direct fp64")
    assert (recs[0]["num_contacts"] > 0).mean() > 0.05  # (penetrating pairs: the EPA section has work)
    _pair(pkg, mix, 2000, "epa_direct_max", (0, 4096), "direct fp32", f32=True)
    _check_names()


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_gjk_fan_out_and_one_kernel_epa(pkg, mix, f32):
    """8 192 pairs: the solids' kernels fanned out over four streams against in line; the one-kernel EPA forms behind them."""
    _pair(pkg, mix, 8192, "gjk_beside_max", (0, 120000), "fan " + ("fp32" if f32 else "fp64"), f32=f32)
    _check_names()


def test_staged_epa(pkg, mix):
    """40 000 pairs, above both *_staged_min: the staged convex x convex tier of fp32 with its records aside or in line; the two fp64 fast-tier
    kernels (the mix has curved shapes) on two streams or one."""
    _pair(pkg, mix, 40000, "epa_records_aside", (0, 1), "staged fp32", f32=True)
    _pair(pkg, mix, 40000, "epa64_two_streams", (0, 1), "staged fp64")
    _check_names()


def test_split_batch(pkg, mix):
    """131 072 pairs (the smallest batch that splits) of a library with three iterative buckets: one stream against two halves on two; then
    gjk_beside_max set AFTER the first split batch -- the helper exists by then and follows it."""
    n = 131072
    one = _run(pkg, mix, n, {"split": 1}, "split 1", then=lambda l: _assert_parts(l, 1))
    lib = pkg.workloads.make_library(pkg, mix, options={"split": 2})
    try:
        two = _run(pkg, mix, n, None, "split 2", lib=lib, then=lambda l: _assert_parts(l, 2))
        assert two.tobytes() == one.tobytes()
        lib.set_option("gjk_beside_max", 1)
        late = _run(pkg, mix, n, None, "split 2 gjk_beside_max=1 set late", lib=lib, then=lambda l: _assert_parts(l, 2))
        assert late.tobytes() == one.tobytes()
    finally:
        lib.close()
    _check_names()


def _assert_parts(lib, parts):
    assert lib.last_split_parts() == parts


def test_mixed_library(pkg, mixed_library):
    """Meshes and solids in one library, fp64 collide(): 300 queries (the split plan starts at 256), then 200; the mesh walks in line (0), beside
    the solids' kernels by the previous batch's counts (2) or always (4)."""
    b = mixed_library
    for n in (300, 200):
        recs = {}
        for beside in (0, 2, 4):
            if beside == 2:  # (not pinned: which order setting 2 takes hangs on the batch before)
                lib = pkg.workloads.make_library(pkg, b, options={"mesh_beside": 2})
                try:
                    lib.set_host_chunk(n)
                    req = pkg.abi.default_collision_request()
                    lib.collide(b.s1[:n], b.s2[:n], b.tf1[:n], b.tf2[:n], req)
                    recs[2] = lib.collide(b.s1[:n], b.s2[:n], b.tf1[:n], b.tf2[:n], req)
                finally:
                    lib.close()
            else:
                recs[beside] = _run(pkg, b, n, {"mesh_beside": beside}, "mixed n=%d mesh_beside=%d" % (n, beside))
        assert recs[2].tobytes() == recs[0].tobytes() and recs[4].tobytes() == recs[0].tobytes(), n
        assert (recs[0]["num_contacts"] > 0).any() and (recs[0]["num_contacts"] == 0).any()
    _check_names()


@pytest.mark.parametrize("bvhd_pool", [0, 1])
@pytest.mark.parametrize("shape_dist_pool", [0, 1])
def test_mesh_distance(pkg, mixed_library, bvhd_pool, shape_dist_pool):
    """The same library, 300 distance() queries: the lane form of mesh x solid and the mesh x mesh walk with their continuations (pooled or a wave
    per walk).  Names only: that the forms agree is the distance tests' statement."""
    b = mixed_library
    seen = []
    _run(pkg, b, 300, {"bvhd_pool": bvhd_pool, "shape_dist_pool": shape_dist_pool}, "distance bvhd_pool=%d shape_dist_pool=%d" % (bvhd_pool, shape_dist_pool),
         kind="distance", then=lambda lib: seen.append(lib.last_ordered_reruns()))
    print("    reruns", seen)
    assert seen[0]["mesh_continued"] > 0 and seen[0]["solid_continued"] > 0  # (walks of both kinds go past their budget: the continuations run)
    _check_names()
