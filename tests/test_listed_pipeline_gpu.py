"""The listed-leaf pipeline that height fields and octrees share (csrc/hfcl_listed.hpp, csrc/hfcl_host_listed.hpp): what the two kinds
have in common on the host and nothing else checks -- the timer names each call reports, that the two kinds keep separate state on one
library, and the device forms' contact read-back at its three input shapes.  The arithmetic is held by test_hfield_gpu.py,
test_octree_gpu.py, test_octree_distance_gpu.py and test_scene_terrain_gpu.py.

The smallest world that reaches every kernel: a 3 x 3 height field and an octree of four occupied voxels at depth 3; solids that sit
over the field's middle vertex (four cells) or between the voxels, the others far off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HF_NAMES = ["k_hf_walk<emit>", "k_hf_leaf", "k_hf_fold", "k_hf_scan<contacts>", "k_hf_fold<contacts>"]
OCT_NAMES = ["k_oct_walk<emit>", "k_oct_leaf", "k_oct_fold", "k_hf_scan<contacts>", "k_oct_fold<contacts>"]


@pytest.fixture(scope="module")
def world(pkg, torch_cuda):
    L = pkg.geometry.ShapeLibrary()
    solids = [L.add_sphere(0.4), L.add_box(0.5, 0.6, 0.7)]
    lib = pkg.Library(L)
    field = lib.add_hfield(2.0, 2.0, np.array([[1.0, 1.2, 1.0], [1.1, 1.5, 1.2], [1.0, 1.3, 1.1]]), 0.0)
    voxels = np.array([[0.125, 0.125, 0.125], [-0.125, 0.125, 0.125], [0.125, -0.125, 0.125], [0.125, 0.125, -0.125]])
    tree = lib.add_octree(pkg.engine.octree_from_points(voxels, 0.25, 3), 0.25, 3)
    yield dict(lib=lib, field=field, tree=tree, solids=solids)
    lib.close()


def _queries(pkg, w, n, kind):
    """n queries of one kind: the even ones touch (the solid dips into the field's middle, or sits among the voxels), the odd ones are
    far off; every third in the caller's order (solid, container)"""
    rng = np.random.default_rng(100 + n + len(kind))
    T = np.zeros((n, 3))
    for i in range(n):
        near = (rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 1.6 if kind == "hfield" else rng.uniform(-0.1, 0.1))
        T[i] = near if i % 2 == 0 else (20.0 + i, -15.0, 9.0)
    ids = np.full(n, w["field"] if kind == "hfield" else w["tree"], dtype=np.uint32)
    shape = np.array([w["solids"][i % 2] for i in range(n)], dtype=np.uint32)
    swapped = (np.arange(n) % 3 == 2).astype(np.uint8)
    return ids, shape, pkg.geometry.make_pose(T=np.zeros((n, 3))), pkg.geometry.make_pose(T=T), swapped


def _request(pkg, num_max_contacts):
    req = pkg.abi.default_collision_request()
    req.num_max_contacts = num_max_contacts
    return req


def _host(lib, kind, q, req, cap):
    ids, shape, tfc, tfs, swapped = q
    call = lib.hfield_collide if kind == "hfield" else lib.octree_collide
    return call(ids, shape, tfc, tfs, req, swapped=swapped, max_contacts=cap)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_timer_names(pkg, world):
    lib = world["lib"]
    lib.set_kernel_timing(True)
    req = _request(pkg, 2)
    names = lambda: [name for name, _ in lib.last_kernel_breakdown()]  # noqa: E731
    rec, _, _, nc = _host(lib, "hfield", _queries(pkg, world, 8, "hfield"), req, 16)
    assert names() == HF_NAMES
    assert nc > 0 and (rec["num_contacts"] > 0).tolist() == [True, False] * 4
    q = _queries(pkg, world, 8, "octree")
    rec, _, _, nc = _host(lib, "octree", q, req, 16)
    assert names() == OCT_NAMES
    assert nc > 0 and (rec["num_contacts"] > 0).tolist() == [True, False] * 4
    lib.octree_distance(*q[:4], swapped=q[4])
    assert names() == ["k_oct_distance"]


def test_the_two_kinds_do_not_share_state(pkg, world):
    lib = world["lib"]
    req = _request(pkg, 4)
    qa, qb = _queries(pkg, world, 13, "hfield"), _queries(pkg, world, 13, "octree")
    sc = lib.scene(np.array(world["solids"] * 3, dtype=np.uint32), np.zeros((0, 2), dtype=np.uint32))
    try:
        sc.set_terrain(world["field"], pkg.geometry.make_pose().reshape(12))
        table = np.ascontiguousarray(qa[3][:12].reshape(2, 6, 12))
        auto_a, auto_b = _host(lib, "hfield", qa, req, 64), _host(lib, "octree", qb, req, 64)
        assert auto_a[3] >= 3 and auto_b[3] >= 3
        lib.set_option("hfield_chunk", 3)
        lib.set_option("hfield_items", 2)
        lib.set_option("octree_chunk", 5)
        lib.set_option("octree_items", 3)
        first_a = _host(lib, "hfield", qa, req, 64)
        first_b = _host(lib, "octree", qb, req, 64)
        assert sc.collide_terrain(table, req, max_contacts=64)[4] > 0
        again_a = _host(lib, "hfield", qa, req, 64)
        again_b = _host(lib, "octree", qb, req, 64)
        assert _same(again_a, first_a) and _same(again_b, first_b)
        assert _same(first_a, auto_a) and _same(first_b, auto_b)
    finally:
        for key in ("hfield_chunk", "hfield_items", "octree_chunk", "octree_items"):
            lib.set_option(key, 0)
        sc.close()


@pytest.mark.parametrize("kind", ["hfield", "octree"])
def test_device_form_on_a_stream_with_n_contacts_out(pkg, torch_cuda, world, kind):
    torch, lib, abi = torch_cuda, world["lib"], pkg.abi
    req = _request(pkg, 4)
    q = _queries(pkg, world, 13, kind)
    want, want_dlb, want_con, produced = _host(lib, kind, q, req, 64)
    assert 3 <= produced <= 64
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_in = [t(q[0].view(np.int32)), t(q[1].view(np.int32)), t(q[2]), t(q[3])]
    d_sw = t(q[4])
    call = lib.hfield_collide_device if kind == "hfield" else lib.octree_collide_device
    stream = torch.cuda.Stream()
    # a capacity below the produced count; no contact buffer but a count; neither
    for cap, want_count in ((1, True), (0, True), (0, False)):
        d_out = torch.full((13 * 96,), 0x5A, dtype=torch.uint8, device=dev)
        d_dlb = torch.full((13,), -7.0, dtype=torch.float64, device=dev)
        d_con = torch.full(((cap + 2) * 96,), 0x5A, dtype=torch.uint8, device=dev) if cap else None  # (two guard records behind the capacity)
        torch.cuda.synchronize()
        nc = call(*d_in, 13, req, d_out, d_swapped=d_sw, d_bound=d_dlb, d_contacts=d_con, max_contacts=cap, want_count=want_count,
                  stream=stream.cuda_stream)
        stream.synchronize()
        assert nc == (produced if want_count else None), (cap, want_count)
        assert d_out.cpu().numpy().tobytes() == want.tobytes() and d_dlb.cpu().numpy().tobytes() == want_dlb.tobytes(), (cap, want_count)
        if cap:
            con = d_con.cpu().numpy()
            assert con[:cap * 96].tobytes() == want_con[:cap].tobytes() and (con[cap * 96:] == 0x5A).all()
    assert abi.CONTACT_DTYPE.itemsize == 96 and abi.RESULT_DTYPE.itemsize == 96
