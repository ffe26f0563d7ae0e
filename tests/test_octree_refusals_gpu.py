"""What the eight octree entry points and the two height-field ones refuse, and in which order (csrc/hfcl_host_listed.hpp: the bodies
they share; csrc/hfcl_host_octree.hip: the kinds): one row per (entry point, fault or pair of faults) -- the return code, the exact
hfcl_last_error() text, every output byte left as it was (0x5A), and the contact count as the refusal leaves it (77: never written; 0:
the refusal came after it was zeroed).  The expected columns (WANT_COLLIDE, WANT_DISTANCE) were recorded from the library as it stood
BEFORE the distance() bodies and the mesh check were written once (every row run through _call on that library), so they hold the
order of two faults in one call as well as each alone.  ACCEPTED is the one row whose text moved with that change; the parent's
answer stands beside it in WANT_COLLIDE.  Beside the table: the timer name of the mesh distance() call, and the host distance forms
in chunks of two queries against one chunk, byte for byte.

The world: a depth-3 tree of four voxels, a 3 x 3 height field, a sphere and a box, a one-triangle mesh, and on a second library a
chain mesh one level deeper than the mesh walk's stack.  Shape rows 2, 3, 4 name the meshes 0, 1, 2: the first library registers
mesh 0, the second meshes 0 and 1, so row 4 names no registered mesh on either.

Not in the table: the device check (it needs a machine without a GPU), and "batch too large" for hfcl_octree_mesh_collide_batch (its
mesh check reads shape[0, n) first: n = 2^32 there is a read past the arrays, before and after)."""
import ctypes as C

import numpy as np
import pytest

import octree_mesh_cases as omc

pytestmark = pytest.mark.gpu

SPHERE, BOX, TRI, DEEP, NO_MESH = range(5)  # the shape rows
N = 3
HF = ("hfcl_hfield_collide_batch", "hfcl_hfield_collide_batch_device")
OCT_C = ("hfcl_octree_collide_batch", "hfcl_octree_collide_batch_device")
OCTM_C = ("hfcl_octree_mesh_collide_batch", "hfcl_octree_mesh_collide_batch_device")
OCT_D = ("hfcl_octree_distance_batch", "hfcl_octree_distance_batch_device")
OCTM_D = ("hfcl_octree_mesh_distance_batch", "hfcl_octree_mesh_distance_batch_device")

# The faults of a row, "+"-joined:
#   lib, req   a null library, a null request           guess    gjk_initial_guess = CachedGuess (a request refusal that names the call)
#   deep       the second library; shape[2] = DEEP      bvh      shape[1] = NO_MESH
#   n0, big    n = 0, n = 2^32                          buf      out = NULL          noshape   shape = NULL
#   id, id2    the container id of query 0 / 2 = 99     solid0, solid   query 0 / 2 names a shape the kind has no evaluator for
COLLIDE_SOLID = ["lib", "req", "lib+req", "lib+guess", "guess", "guess+n0", "n0", "n0+buf", "buf", "big", "buf+big"]
COLLIDE_SOLID_HOST = ["id", "solid", "buf+id", "big+id", "id+solid", "solid0+id2"]
COLLIDE_MESH = ["lib", "req", "lib+req", "lib+guess", "guess", "deep", "req+deep", "guess+deep", "deep+n0", "guess+n0", "n0", "n0+buf", "buf",
                "deep+buf"]
COLLIDE_MESH_HOST = ["bvh", "req+bvh", "guess+bvh", "deep+bvh", "bvh+n0", "bvh+buf", "noshape", "bvh+noshape", "deep+noshape", "id", "solid",
                     "buf+id", "deep+id", "bvh+id", "bvh+solid0", "id+solid", "solid0+id2"]
COLLIDE_MESH_DEVICE = ["big", "buf+big", "deep+big"]
DISTANCE = ["lib", "req", "lib+req", "lib+guess", "guess", "req+n0", "guess+n0", "n0", "n0+buf", "buf", "big", "buf+big"]
DISTANCE_HOST = ["id", "solid", "buf+id", "big+id", "id+solid", "solid0+id2"]
DISTANCE_MESH = ["deep", "buf+deep", "big+deep", "guess+deep", "deep+n0"]
DISTANCE_MESH_HOST = ["bvh", "buf+bvh", "deep+bvh", "deep+id", "bvh+id", "bvh+solid0", "bvh+n0"]


def _rows():
    rows = []
    for host, device in (HF, OCT_C):
        rows += [(host, f) for f in COLLIDE_SOLID + COLLIDE_SOLID_HOST] + [(device, f) for f in COLLIDE_SOLID]
    rows += [(OCTM_C[0], f) for f in COLLIDE_MESH + COLLIDE_MESH_HOST] + [(OCTM_C[1], f) for f in COLLIDE_MESH + COLLIDE_MESH_DEVICE]
    rows += [(OCT_D[0], f) for f in DISTANCE + DISTANCE_HOST] + [(OCT_D[1], f) for f in DISTANCE]
    rows += [(OCTM_D[0], f) for f in DISTANCE + DISTANCE_HOST + DISTANCE_MESH + DISTANCE_MESH_HOST]
    rows += [(OCTM_D[1], f) for f in DISTANCE + DISTANCE_MESH]
    return rows


ROWS = _rows()


@pytest.fixture(scope="module")
def world(pkg, torch_cuda):
    def library(meshes):
        L = pkg.geometry.ShapeLibrary()
        assert [L.add_sphere(0.4), L.add_box(0.5, 0.6, 0.7)] == [SPHERE, BOX]
        assert [L.add_bvh(k, 3) for k in range(3)] == [TRI, DEEP, NO_MESH]
        lib = pkg.Library(L)
        for k, m in enumerate(meshes):
            assert lib.add_bvh(m) == k
        voxels = np.array([[0.125, 0.125, 0.125], [-0.125, 0.125, 0.125], [0.125, -0.125, 0.125], [0.125, 0.125, -0.125]])
        assert lib.add_octree(pkg.engine.octree_from_points(voxels, 0.25, 3), 0.25, 3) == 0
        assert lib.add_hfield(2.0, 2.0, np.array([[1.0, 1.2, 1.0], [1.1, 1.5, 1.2], [1.0, 1.3, 1.1]]), 0.0) == 0
        return lib

    lib, lib2 = library([omc.one_triangle()]), library([omc.one_triangle(), omc.chain_mesh(omc.DEPTH_LIMIT + 1)])
    yield dict(lib=lib, lib2=lib2)
    lib.close()
    lib2.close()


def _call(pkg, torch, w, fn, faults):
    """One call of entry point `fn` with `faults`: (code, hfcl_last_error() or None, the contact count afterwards or None); asserts that a
    call that refused, or had no query, left every output byte as it was"""
    abi = pkg.abi
    f = set(faults.split("+"))
    device, distance, mesh = fn.endswith("_device"), "_distance_" in fn, "_mesh_" in fn
    lib = w["lib2" if "deep" in f else "lib"]
    ids = np.zeros(N, dtype=np.uint32)
    shape = np.array([TRI] * N if mesh else [SPHERE, BOX, SPHERE], dtype=np.uint32)
    for name, at in (("id", 0), ("id2", 2)):
        if name in f:
            ids[at] = 99
    for name, at, row in (("deep", 2, DEEP), ("bvh", 1, NO_MESH), ("solid0", 0, SPHERE if mesh else TRI), ("solid", 2, SPHERE if mesh else TRI)):
        if name in f:
            shape[at] = row
    tf_c = pkg.geometry.make_pose(T=np.zeros((N, 3)))
    tf_s = pkg.geometry.make_pose(T=np.array([[0.1, 0.0, 1.6], [20.0, -15.0, 9.0], [0.0, 0.1, 0.05]]))
    req = abi.default_distance_request() if distance else abi.default_collision_request()
    if "guess" in f:
        req.q.gjk_initial_guess = abi.CachedGuess
    n = 0 if "n0" in f else 1 << 32 if "big" in f else N
    # the outputs: records, then the bounds (collide) or the visited counts (distance), then the contacts (collide), all bytes 0x5A
    sizes = [N * 96, N * 4] if distance else [N * 96, N * 8, 4 * 96]
    if device:
        dev = torch.device("cuda:0")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        keep = [t(ids.view(np.int32)), t(shape.view(np.int32)), t(tf_c), t(tf_s)]
        outs = [torch.full((s,), 0x5A, dtype=torch.uint8, device=dev) for s in sizes]
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        torch.cuda.synchronize()
    else:
        keep = [ids, shape, np.ascontiguousarray(tf_c), np.ascontiguousarray(tf_s)]
        outs = [np.full(s, 0x5A, dtype=np.uint8) for s in sizes]
        p = abi.ptr
    args = [None if "lib" in f else lib._h, p(keep[0]), None if "noshape" in f else p(keep[1]), p(keep[2]), p(keep[3]), C.c_size_t(n), None,
            None if "req" in f else C.byref(req), None if "buf" in f else p(outs[0]), p(outs[1])]
    nc = C.c_size_t(77)
    if not distance:
        args += [p(outs[2]), C.c_size_t(4), C.byref(nc)]
    if device:
        args.append(None)  # the stream
    rc = getattr(pkg.engine.dll(), fn)(*args)
    if device:
        torch.cuda.synchronize()
        outs = [o.cpu().numpy() for o in outs]
    if rc or n == 0:
        assert all((o == 0x5A).all() for o in outs), "an output byte was written"
    return rc, pkg.engine.last_error() if rc else None, None if distance else int(nc.value)


# The texts; {who}: the entry point
TEXTS = {
    "null": "{who}: null library / request",
    "lib": "{who}: null library",
    "req": "null request",
    "guess": "{who}: gjk_initial_guess must be DefaultGuess (a cached guess chains from leaf to leaf inside a query, a bounding-volume guess "
             "changes the leaf set-up: not done)",
    "guess hfield": "{who}: gjk_initial_guess must be DefaultGuess (a cached guess chains from leaf to leaf inside a query: not done)",
    "buffer": "{who}: null buffer",
    "large": "batch too large (max 2^32-16 queries per call)",
    "id": "{who}: {noun} / shape id outside the library at query 0",
    "solid": "{verb} function between {a_noun} and node type {type} is not yet supported.",
    "deep": "{who}: the BVH of mesh 1 has 65 levels (limit 64)",
    "bvh": "{who}: bvh_index outside the registered meshes at query 1",
}
# faults: (code, text, the contact count afterwards), as recorded from the parent library.  The answer to a set of
# faults was the same in every entry point of a column that has the row: host and device form, height field and octree
WANT_COLLIDE = {
    "lib": (1, "null", 77), "req": (1, "null", 77), "lib+req": (1, "null", 77), "lib+guess": (1, "null", 77), "guess": (5, "guess", 77),
    "guess+n0": (5, "guess", 77), "n0": (0, None, 0), "n0+buf": (0, None, 0), "buf": (1, "buffer", 0), "big": (5, "large", 0),
    "buf+big": (1, "buffer", 0), "id": (1, "id", 0), "solid": (2, "solid", 0), "buf+id": (1, "buffer", 0), "big+id": (5, "large", 0),
    "id+solid": (1, "id", 0), "solid0+id2": (2, "solid", 0),
    # the mesh kinds: the mesh check stands between the request and the zeroing of the count
    "deep": (5, "deep", 77), "req+deep": (1, "null", 77), "guess+deep": (5, "guess", 77), "deep+n0": (0, None, 0), "deep+buf": (5, "deep", 77),
    "deep+big": (5, "deep", 77), "bvh": (1, "bvh", 77), "req+bvh": (1, "bvh", 77), "guess+bvh": (5, "guess", 77), "deep+bvh": (5, "deep", 77),
    "bvh+n0": (0, None, 0), "bvh+buf": (1, "bvh", 77), "noshape": (1, "buffer", 0), "bvh+noshape": (1, "buffer", 0),
    "deep+noshape": (1, "buffer", 0), "deep+id": (5, "deep", 77), "bvh+id": (1, "bvh", 77), "bvh+solid0": (1, "bvh", 77),
}
WANT_DISTANCE = {
    "lib": (1, "lib"), "req": (1, "req"), "lib+req": (1, "lib"), "lib+guess": (1, "lib"), "guess": (5, "guess"), "req+n0": (1, "req"),
    "guess+n0": (5, "guess"), "n0": (0, None), "n0+buf": (0, None), "buf": (1, "buffer"), "big": (5, "large"), "buf+big": (1, "buffer"),
    "id": (1, "id"), "solid": (2, "solid"), "buf+id": (1, "buffer"), "big+id": (5, "large"), "id+solid": (1, "id"), "solid0+id2": (2, "solid"),
    # the mesh kinds: the mesh check stands behind the arrays
    "deep": (5, "deep"), "buf+deep": (1, "buffer"), "big+deep": (5, "large"), "guess+deep": (5, "guess"), "deep+n0": (0, None),
    "bvh": (1, "bvh"), "buf+bvh": (1, "buffer"), "deep+bvh": (5, "deep"), "deep+id": (5, "deep"), "bvh+id": (1, "bvh"), "bvh+solid0": (1, "bvh"),
    "bvh+n0": (0, None),
}
# The one row that moved: the mesh collide wrapper ran its bvh_index loop in front of the shared body, behind a guard that did not look
# at the request; the loop is now part of the body's mesh check, behind the null checks.  The same code, another text
ACCEPTED = {("hfcl_octree_mesh_collide_batch", "req+bvh"): (1, "null", 77)}


def _expected(fn, faults, table):
    """(code, text, count) of a row as _call returns it"""
    distance, mesh, hfield = "_distance_" in fn, "_mesh_" in fn, "_hfield_" in fn
    code, key, count = (table[faults] + (None,))[:3]
    if key == "guess" and hfield:
        key = "guess hfield"
    text = key and TEXTS[key].format(who=fn, noun="height field" if hfield else "octree", a_noun="a height field" if hfield else "an octree",
                                     verb="Distance" if distance else "Collision", type=10 if mesh else 5)  # (a sphere among meshes, a mesh among solids)
    return code, text, count


def test_the_tables_are_used_and_the_accepted_row_is_a_row():
    for table, distance in ((WANT_COLLIDE, False), (WANT_DISTANCE, True)):
        assert set(table) == {f for fn, f in ROWS if ("_distance_" in fn) == distance}
    assert set(ACCEPTED) <= set(ROWS) and all(ACCEPTED[fn, f][0] == WANT_COLLIDE[f][0] and ACCEPTED[fn, f] != WANT_COLLIDE[f] for fn, f in ACCEPTED)
    assert len(ROWS) == len(set(ROWS)) and {fn for fn, _ in ROWS} == set(HF + OCT_C + OCTM_C + OCT_D + OCTM_D)


@pytest.mark.parametrize("fn,faults", ROWS, ids=["%s-%s" % (fn[5:], f) for fn, f in ROWS])
def test_refusal(pkg, torch_cuda, world, fn, faults):
    table = {faults: ACCEPTED[fn, faults]} if (fn, faults) in ACCEPTED else WANT_DISTANCE if "_distance_" in fn else WANT_COLLIDE
    assert _call(pkg, torch_cuda, world, fn, faults) == _expected(fn, faults, table)


def _distance_queries(pkg, mesh):
    """five queries near the voxels (the second far off), the second and the fifth in the caller's order (solid or mesh, OcTree)"""
    T = np.array([[0.6, 0.1, 0.0], [20.0, -15.0, 9.0], [0.1, 0.1, 0.1], [-0.7, 0.3, 0.2], [0.0, 0.0, 0.9]])
    shape = np.array([TRI] * 5 if mesh else [SPHERE, BOX, SPHERE, BOX, SPHERE], dtype=np.uint32)
    return np.zeros(5, dtype=np.uint32), shape, pkg.geometry.make_pose(T=np.zeros((5, 3))), pkg.geometry.make_pose(T=T), np.array([0, 1, 0, 0, 1], dtype=np.uint8)


def test_mesh_distance_timer_name(pkg, world):
    lib = world["lib"]  # (kernel timing is on: a library's default, and no test of this file switches it)
    q = _distance_queries(pkg, True)
    lib.octree_mesh_distance(*q[:4], swapped=q[4])
    assert [name for name, _ in lib.last_kernel_breakdown()] == ["k_octm_distance"]


@pytest.mark.parametrize("mesh", [False, True], ids=["solids", "meshes"])
def test_host_distance_in_chunks_of_two(pkg, world, mesh):
    lib = world["lib"]
    call = lib.octree_mesh_distance if mesh else lib.octree_distance
    q = _distance_queries(pkg, mesh)
    try:
        whole, whole_visited = call(*q[:4], swapped=q[4], want_visited=True)
        lib.set_option("octree_chunk", 2)
        parts, parts_visited = call(*q[:4], swapped=q[4], want_visited=True)
        plain = call(*q[:4])  # (swapped: NULL, no visited counts)
    finally:
        lib.set_option("octree_chunk", 0)
    assert parts.tobytes() == whole.tobytes() and parts_visited.tobytes() == whole_visited.tobytes()
    assert (whole_visited[[0, 2, 3, 4]] >= 1).all() and (whole["status"] & pkg.abi.STATUS_SWAPPED != 0).tolist() == [False, True, False, False, True]
    assert (plain["status"] & pkg.abi.STATUS_SWAPPED == 0).all() and plain["distance"].tobytes() == whole["distance"].tobytes()
