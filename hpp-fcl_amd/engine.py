"""ctypes front-end of csrc/libhppfcl_amd.so (the C ABI of include/hppfcl_amd.h).

Plumbing only: argument marshalling and device-pointer hand-off.  All compute is in the HIP
library.  There is NO fallback: a missing library or a missing GPU raises."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("HFCL_LIB_PATH", os.path.join(_CSRC, "libhppfcl_amd.so"))  # override: A/B builds

EXPORTED_SYMBOLS = [
    "hfcl_abi_version", "hfcl_device_count", "hfcl_last_error", "hfcl_collision_request_init",
    "hfcl_distance_request_init", "hfcl_lib_create", "hfcl_lib_destroy", "hfcl_lib_num_shapes", "hfcl_lib_device", "hfcl_lib_climb_min",
    "hfcl_lib_add_bvh", "hfcl_collide_batch", "hfcl_distance_batch", "hfcl_collide_batch_device",
    "hfcl_distance_batch_device", "hfcl_distance_batch_device_f32", "hfcl_collide_batch_device_f32", "hfcl_collide_batch_f32", "hfcl_distance_batch_f32",
    "hfcl_collide_batch_contacts", "hfcl_last_kernel_ms", "hfcl_last_kernel_name", "hfcl_bvh_build",
    "hfcl_world_aabbs", "hfcl_broadphase_self_pairs", "hfcl_broadphase_pairs_between", "hfcl_pairlist_size",
    "hfcl_pairlist_data", "hfcl_pairlist_free", "hfcl_lib_set_kernel_timing", "hfcl_pair_supported", "hfcl_last_kernel_breakdown", "hfcl_last_bucket_counts", "hfcl_last_ordered_reruns", "hfcl_last_epa_handed_over", "hfcl_last_redo_count", "hfcl_lib_set_split", "hfcl_lib_get_split", "hfcl_lib_last_split_parts",
    "hfcl_collide_batch_qt", "hfcl_distance_batch_qt", "hfcl_lib_set_host_chunk", "hfcl_lib_set_shapes",
    "hfcl_lib_set_convex_neighbors", "hfcl_compact_results_device", "hfcl_compact_results_device_f32",
 "hfcl_shard_range", "hfcl_multi_create", "hfcl_multi_destroy", "hfcl_multi_size", "hfcl_multi_replica",
    "hfcl_multi_set_shapes", "hfcl_multi_set_convex_neighbors", "hfcl_multi_add_bvh", "hfcl_collide_batch_multi", "hfcl_distance_batch_multi",
    "hfcl_collide_batch_multi_device", "hfcl_distance_batch_multi_device", "hfcl_collide_batch_multi_f32", "hfcl_distance_batch_multi_f32",
    "hfcl_lib_set_option", "hfcl_lib_option_key", "hfcl_has_ab_forms", "hfcl_multi_set_option", "hfcl_multi_last_gather",
    "hfcl_contact_patch_request_init", "hfcl_patch_supported", "hfcl_contact_patch_max_points", "hfcl_contact_patch_max_points_shapes",
    "hfcl_contact_patch_batch", "hfcl_contact_patch_batch_device",
    "hfcl_scene_create", "hfcl_scene_set_pairs", "hfcl_scene_destroy", "hfcl_scene_num_objects", "hfcl_scene_num_pairs",
    "hfcl_scene_collide", "hfcl_scene_distance", "hfcl_scene_collide_device", "hfcl_scene_distance_device",
    "hfcl_scene_collide_f32", "hfcl_scene_distance_f32", "hfcl_scene_collide_device_f32", "hfcl_scene_distance_device_f32",
]
# include/hppfcl_amd_cull.h (included by hppfcl_amd.h): the pair list culled per configuration on the device
CULL_SYMBOLS = [
    "hfcl_scene_world_aabbs", "hfcl_scene_world_aabbs_f32", "hfcl_scene_world_aabbs_device", "hfcl_scene_world_aabbs_device_f32",
    "hfcl_scene_cull", "hfcl_scene_cull_f32", "hfcl_scene_cull_device", "hfcl_scene_cull_device_f32",
    "hfcl_scene_collide_listed_device", "hfcl_scene_distance_listed_device", "hfcl_scene_collide_listed_device_f32",
    "hfcl_scene_distance_listed_device_f32", "hfcl_scene_collide_culled", "hfcl_scene_distance_culled", "hfcl_scene_collide_culled_f32",
    "hfcl_scene_distance_culled_f32",
]
# include/hppfcl_amd_nearest.h (included by hppfcl_amd.h): the per-configuration minimum distance with box-bound pruning
NEAREST_SYMBOLS = [
    "hfcl_scene_nearest", "hfcl_scene_nearest_f32", "hfcl_scene_nearest_device", "hfcl_scene_nearest_device_f32",
]
# include/hppfcl_amd_pairs.h (included by hppfcl_amd.h): the self-collision pairs per configuration made on the device, the calls on such a list
PAIRS_SYMBOLS = [
    "hfcl_scene_self_pairs", "hfcl_scene_self_pairs_f32", "hfcl_scene_self_pairs_device", "hfcl_scene_self_pairs_device_f32",
    "hfcl_scene_collide_pairs_device", "hfcl_scene_distance_pairs_device", "hfcl_scene_collide_pairs_device_f32",
    "hfcl_scene_distance_pairs_device_f32", "hfcl_scene_collide_self", "hfcl_scene_distance_self", "hfcl_scene_collide_self_f32",
    "hfcl_scene_distance_self_f32",
]
# include/hppfcl_amd_pairs_sorted.h (included by hppfcl_amd_pairs.h): the same list by sort and sweep (option scene_pairs_sorted)
PAIRS_SORTED_SYMBOLS = [
    "hfcl_scene_last_pairs_form",
]
# include/hppfcl_amd_groups.h (included by hppfcl_amd.h): object groups and a group matrix for the device-made pair lists
GROUPS_SYMBOLS = [
    "hfcl_scene_set_groups", "hfcl_scene_clear_groups", "hfcl_scene_num_groups",
]
# include/hppfcl_amd_nearest_self.h (included by hppfcl_amd.h): the clearance per configuration on device-made pairs
NEAREST_SELF_SYMBOLS = [
    "hfcl_scene_nearest_self", "hfcl_scene_nearest_self_f32", "hfcl_scene_nearest_self_device", "hfcl_scene_nearest_self_device_f32",
]
# include/hppfcl_amd_env.h (included by hppfcl_amd.h): a static environment kept on the device, the calls on the moving objects' poses alone
ENV_SYMBOLS = [
    "hfcl_scene_set_environment", "hfcl_scene_set_environment_f32", "hfcl_scene_clear_environment", "hfcl_scene_n_moving",
    "hfcl_scene_environment_aabbs", "hfcl_scene_env_pairs", "hfcl_scene_env_pairs_f32", "hfcl_scene_env_pairs_device",
    "hfcl_scene_env_pairs_device_f32", "hfcl_scene_collide_env_pairs_device", "hfcl_scene_distance_env_pairs_device",
    "hfcl_scene_collide_env_pairs_device_f32", "hfcl_scene_distance_env_pairs_device_f32", "hfcl_scene_collide_env",
    "hfcl_scene_distance_env", "hfcl_scene_collide_env_f32", "hfcl_scene_distance_env_f32",
]
# include/hppfcl_amd_nearest_env.h (included by hppfcl_amd.h): the clearance of the moving objects among the environment kept on the device
NEAREST_ENV_SYMBOLS = [
    "hfcl_scene_nearest_env", "hfcl_scene_nearest_env_f32", "hfcl_scene_nearest_env_device", "hfcl_scene_nearest_env_device_f32",
]
# include/hppfcl_amd_hfield.h (included by hppfcl_amd.h): HeightField<AABB> against convex solids
HFIELD_SYMBOLS = [
    "hfcl_hfield_build", "hfcl_lib_add_hfield", "hfcl_lib_hfield_count", "hfcl_lib_clear_hfields", "hfcl_hfield_local_aabb", "hfcl_hfield_pair_supported",
    "hfcl_hfield_collide_batch", "hfcl_hfield_collide_batch_device",
]
# include/hppfcl_amd_terrain.h (included by hppfcl_amd.h): a height-field terrain under a scene's moving objects
TERRAIN_SYMBOLS = [
    "hfcl_scene_set_terrain", "hfcl_scene_clear_terrain", "hfcl_scene_n_terrain_objects", "hfcl_scene_collide_terrain",
    "hfcl_scene_collide_terrain_device",
]
# include/hppfcl_amd_octree.h (included by hppfcl_amd.h): an occupancy OcTree against convex solids
OCTREE_SYMBOLS = [
    "hfcl_octree_validate", "hfcl_octree_from_points", "hfcl_lib_add_octree", "hfcl_lib_octree_set_thresholds", "hfcl_lib_octree_count",
    "hfcl_lib_clear_octrees", "hfcl_octree_root_box", "hfcl_octree_pair_supported", "hfcl_octree_collide_batch",
    "hfcl_octree_collide_batch_device",
]
# include/hppfcl_amd_octree_distance.h (included by hppfcl_amd.h): distance() between a registered OcTree and a convex solid
OCTREE_DISTANCE_SYMBOLS = ["hfcl_octree_distance_pair_supported", "hfcl_octree_distance_batch", "hfcl_octree_distance_batch_device"]
# include/hppfcl_amd_octree_mesh.h (included by hppfcl_amd.h): collide() between a registered OcTree and a registered BVHModel<OBBRSS>
OCTREE_MESH_SYMBOLS = ["hfcl_octree_mesh_pair_supported", "hfcl_octree_mesh_collide_batch", "hfcl_octree_mesh_collide_batch_device"]
OCTREE_MESH_MAX_BVH_DEPTH = 64  # HFCL_OCTREE_MESH_MAX_BVH_DEPTH
# include/hppfcl_amd_octree_mesh_distance.h (included by hppfcl_amd.h): distance() between a registered OcTree and a registered BVHModel<OBBRSS>
OCTREE_MESH_DISTANCE_SYMBOLS = ["hfcl_octree_mesh_distance_pair_supported", "hfcl_octree_mesh_distance_batch", "hfcl_octree_mesh_distance_batch_device"]


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hfcl error %d: %s" % (code, msg))
        self.code = code


def build_native(verbose=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-j8", "-C", _CSRC]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


_DLL = None


def dll():
    """Load the native library; raises if it has not been built (no fallback)."""
    global _DLL
    if _DLL is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(abi.ERR_NO_DEVICE, "native library %s is missing: run __graft_entry__.build()" % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.  If torch is going to
        # be used in this process (device tensors, streams, torch.distributed) it must be loaded first
        # so that this library binds to the same runtime; loading ours first makes torch.cuda unusable.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        d = C.CDLL(LIB_PATH)
        d.hfcl_last_error.restype = C.c_char_p
        d.hfcl_lib_create.restype = C.c_void_p
        d.hfcl_lib_num_shapes.restype = C.c_size_t
        d.hfcl_lib_climb_min.restype = C.c_uint32
        d.hfcl_last_kernel_ms.restype = C.c_double
        d.hfcl_last_kernel_name.restype = C.c_char_p
        d.hfcl_broadphase_self_pairs.restype = C.c_void_p
        d.hfcl_broadphase_pairs_between.restype = C.c_void_p
        d.hfcl_pairlist_size.restype = C.c_size_t
        d.hfcl_pairlist_data.restype = C.c_void_p
        d.hfcl_lib_option_key.restype = C.c_char_p
        if hasattr(d, "hfcl_last_epa_handed_over"):
            d.hfcl_last_epa_handed_over.restype = C.c_uint32
        if hasattr(d, "hfcl_last_redo_count"):
            d.hfcl_last_redo_count.restype = C.c_uint32
        if hasattr(d, "hfcl_scene_create"):  # (an A/B build of an older source tree behind HFCL_LIB_PATH has no scenes: Library.scene raises there)
            d.hfcl_scene_create.restype = C.c_void_p
            d.hfcl_scene_num_objects.restype = C.c_size_t
            d.hfcl_scene_num_pairs.restype = C.c_size_t
        if hasattr(d, "hfcl_scene_num_groups"):
            d.hfcl_scene_num_groups.restype = C.c_size_t
        if hasattr(d, "hfcl_scene_n_moving"):
            d.hfcl_scene_n_moving.restype = C.c_size_t
        if hasattr(d, "hfcl_lib_hfield_count"):
            d.hfcl_lib_hfield_count.restype = C.c_size_t
        if hasattr(d, "hfcl_lib_octree_count"):
            d.hfcl_lib_octree_count.restype = C.c_size_t
        if hasattr(d, "hfcl_scene_n_terrain_objects"):
            d.hfcl_scene_n_terrain_objects.restype = C.c_size_t
        _DLL = d
    return _DLL


def last_error():
    return dll().hfcl_last_error().decode()


def device_count():
    return int(dll().hfcl_device_count())


def patch_supported(t1, t2):
    """hfcl_patch_supported: does computeContactPatch have a function for (node_type1, node_type2)?"""
    return bool(dll().hfcl_patch_supported(C.c_int32(int(t1)), C.c_int32(int(t2))))


def contact_patch_request_init():
    """hfcl_contact_patch_request_init: the C library's ContactPatchRequest defaults."""
    r = abi.PatchRequest()
    dll().hfcl_contact_patch_request_init(C.byref(r))
    return r


def contact_patch_max_points_shapes(shapes, req=None):
    """hfcl_contact_patch_max_points_shapes: the patch-size bound of a shape table (no device needed)."""
    shapes = np.ascontiguousarray(shapes)
    cap = C.c_uint32(0)
    _check(dll().hfcl_contact_patch_max_points_shapes(abi.ptr(shapes), C.c_size_t(len(shapes)),
                                                      C.byref(req or abi.default_patch_request()), C.byref(cap)))
    return int(cap.value)


def hfield_pair_supported(node_type):
    """hfcl_hfield_pair_supported: does collide() have a height-field row for a solid of this node type?"""
    return bool(dll().hfcl_hfield_pair_supported(C.c_int32(int(node_type))))


def hfield_build(x_dim, y_dim, heights, min_height=0.0):
    """hfcl_hfield_build: (nodes[HFIELD_NODE_DTYPE], x_grid, y_grid) of HeightField<AABB>(x_dim, y_dim, heights, min_height) (host, no
    GPU needed).  heights: (ny, nx), row 0 = the north edge."""
    h = np.ascontiguousarray(heights, dtype=np.float64)
    if h.ndim != 2:
        raise ValueError("heights: a (ny, nx) matrix")
    ny, nx = h.shape
    n = C.c_size_t(0)
    _check(dll().hfcl_hfield_build(C.c_double(x_dim), C.c_double(y_dim), abi.ptr(h), C.c_size_t(ny), C.c_size_t(nx), C.c_double(min_height),
                                   None, C.byref(n), None, None))
    nodes = np.zeros(n.value, dtype=abi.HFIELD_NODE_DTYPE)
    xg, yg = np.zeros(nx), np.zeros(ny)
    _check(dll().hfcl_hfield_build(C.c_double(x_dim), C.c_double(y_dim), abi.ptr(h), C.c_size_t(ny), C.c_size_t(nx), C.c_double(min_height),
                                   abi.ptr(nodes), C.byref(n), abi.ptr(xg), abi.ptr(yg)))
    return nodes, xg, yg


def octree_pair_supported(node_type):
    """hfcl_octree_pair_supported: does collide() have an octree row for a solid of this node type?"""
    return bool(dll().hfcl_octree_pair_supported(C.c_int32(int(node_type))))


def octree_distance_pair_supported(node_type):
    """hfcl_octree_distance_pair_supported: does distance() have an octree row for a solid of this node type?"""
    return bool(dll().hfcl_octree_distance_pair_supported(C.c_int32(int(node_type))))


def octree_mesh_pair_supported(node_type):
    """hfcl_octree_mesh_pair_supported: does collide() have an octree row for a mesh of this node type?  (BV_OBBRSS alone)"""
    return bool(dll().hfcl_octree_mesh_pair_supported(C.c_int32(int(node_type))))


def octree_mesh_distance_pair_supported(node_type):
    """hfcl_octree_mesh_distance_pair_supported: does hfcl_octree_mesh_distance_batch take a mesh of this node type?  (BV_OBBRSS alone)"""
    return bool(dll().hfcl_octree_mesh_distance_pair_supported(C.c_int32(int(node_type))))


def _octree_nodes(nodes):
    nodes = np.ascontiguousarray(nodes, dtype=abi.OCTREE_NODE_DTYPE)
    if nodes.ndim != 1:
        raise ValueError("nodes: a 1-d array of OCTREE_NODE_DTYPE")
    return nodes


def octree_validate(nodes, depth):
    """hfcl_octree_validate: raises EngineError (last_error names the rule) unless the node array is one tree of at most `depth` levels
    (host, no GPU needed)."""
    nodes = _octree_nodes(nodes)
    _check(dll().hfcl_octree_validate(abi.ptr(nodes) if len(nodes) else None, C.c_size_t(len(nodes)), C.c_uint32(int(depth))))


def octree_from_points(points, resolution, depth=abi.OCTREE_MAX_DEPTH):
    """hfcl_octree_from_points: nodes[OCTREE_NODE_DTYPE] of makeOctree(points, resolution) without octomap (host, no GPU needed): one
    leaf at level `depth` per voxel hit, nodes in depth-first preorder."""
    xyz = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = C.c_size_t(0)
    args = (abi.ptr(xyz) if len(xyz) else None, C.c_size_t(len(xyz)), C.c_double(resolution), C.c_uint32(int(depth)))
    _check(dll().hfcl_octree_from_points(*args, None, C.c_size_t(0), C.byref(n)))
    nodes = np.zeros(n.value, dtype=abi.OCTREE_NODE_DTYPE)
    if n.value:
        _check(dll().hfcl_octree_from_points(*args, abi.ptr(nodes), C.c_size_t(n.value), C.byref(n)))
    return nodes


def has_ab_forms():
    """Does the loaded build carry the forms kept only as identity references (hfcl_has_ab_forms)?"""
    return bool(dll().hfcl_has_ab_forms())


def option_keys():
    """The names hfcl_lib_set_option accepts (hfcl_lib_option_key)."""
    out, i = [], 0
    while True:
        k = dll().hfcl_lib_option_key(C.c_int(i))
        if k is None:
            return out
        out.append(k.decode())
        i += 1


def bvh_build(vertices, triangles, n_threads=0):
    """hfcl_bvh_build: (nodes[BVH_NODE_DTYPE], primitive_indices) of BVHModel<OBBRSS> (host, no GPU needed)."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    nodes = np.zeros(max(2 * len(t) - 1, 0), dtype=abi.BVH_NODE_DTYPE)
    prim = np.zeros(len(t), dtype=np.uint32)
    _check(dll().hfcl_bvh_build(C.c_void_p(v.ctypes.data), C.c_size_t(len(v)), C.c_void_p(t.ctypes.data),
                                C.c_size_t(len(t)), C.c_void_p(nodes.ctypes.data), C.c_void_p(prim.ctypes.data),
                                C.c_int(n_threads)))
    return nodes, prim


def world_aabbs(shape_library, object_shape, object_tf, n_threads=0):
    """hfcl_world_aabbs: (n, 6) world AABBs (min, max) of posed objects (host)."""
    shapes = np.ascontiguousarray(shape_library.shapes_array())
    verts = np.ascontiguousarray(shape_library.vertices_array(), dtype=np.float64)
    ids = np.ascontiguousarray(object_shape, dtype=np.uint32)
    tf = np.ascontiguousarray(object_tf, dtype=np.float64).reshape(-1, 12)
    out = np.zeros((len(ids), 6), dtype=np.float64)
    _check(dll().hfcl_world_aabbs(abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), abi.ptr(ids), abi.ptr(tf),
                                  C.c_size_t(len(ids)), abi.ptr(out), C.c_int(n_threads)))
    return out


def _take_pairlist(h):
    d = dll()
    h = C.c_void_p(h)
    n = d.hfcl_pairlist_size(h)
    if n:
        buf = (C.c_uint32 * (2 * n)).from_address(d.hfcl_pairlist_data(h))
        out = np.frombuffer(buf, dtype=np.uint32).reshape(-1, 2).copy()
    else:
        out = np.zeros((0, 2), dtype=np.uint32)
    d.hfcl_pairlist_free(h)
    return out


def broadphase_self_pairs(aabbs, n_threads=0):
    """All (i < j) with overlapping AABBs: what DynamicAABBTreeCollisionManager::collide reports."""
    a = np.ascontiguousarray(aabbs, dtype=np.float64).reshape(-1, 6)
    return _take_pairlist(dll().hfcl_broadphase_self_pairs(abi.ptr(a), C.c_size_t(len(a)), C.c_int(n_threads)))


def broadphase_pairs_between(aabbs_a, aabbs_b, n_threads=0):
    a = np.ascontiguousarray(aabbs_a, dtype=np.float64).reshape(-1, 6)
    b = np.ascontiguousarray(aabbs_b, dtype=np.float64).reshape(-1, 6)
    return _take_pairlist(dll().hfcl_broadphase_pairs_between(abi.ptr(a), C.c_size_t(len(a)), abi.ptr(b),
                                                              C.c_size_t(len(b)), C.c_int(n_threads)))


def _check(rc):
    if rc != 0:
        raise EngineError(rc, last_error())


def group_words(collides):
    """A group matrix as hfcl_scene_set_groups takes it: uint64[G] from a (G, G) bool matrix (bit h of word g = collides[g][h]) or from
    G words, which pass through."""
    c = np.asarray(collides)
    if c.ndim == 2:
        if c.shape[0] != c.shape[1] or not 1 <= c.shape[0] <= 64:
            raise ValueError("a group matrix is (G, G) with 1 <= G <= 64")
        bits = np.uint64(1) << np.arange(c.shape[0], dtype=np.uint64)
        return np.array([bits[row].sum(dtype=np.uint64) for row in c.astype(bool)], dtype=np.uint64)
    if c.ndim != 1:
        raise ValueError("collides: a (G, G) bool matrix or G uint64 words")
    return np.ascontiguousarray(c, dtype=np.uint64)


def groups_between(n_a, n_b):
    """(object_group, collides) of two managers in one scene: objects [0, n_a) are group 0, [n_a, n_a + n_b) group 1, and only pairs
    of one object of each are listed -- DynamicAABBTreeCollisionManager::collide(otherManager, callback)."""
    group = np.zeros(n_a + n_b, dtype=np.uint8)
    group[n_a:] = 1
    return group, np.array([2, 1], dtype=np.uint64)


def groups_excluding(n_objects, excluded_pairs):
    """(object_group, collides) with one group per object (n_objects <= 64): every pair of distinct objects is allowed but the
    excluded ones -- a robot's allowed-collision matrix."""
    if not 1 <= n_objects <= 64:
        raise ValueError("one group per object takes scenes of 1 to 64 objects")
    m = ~np.eye(n_objects, dtype=bool)
    for i, j in np.asarray(excluded_pairs, dtype=np.int64).reshape(-1, 2):
        m[i, j] = m[j, i] = False
    return np.arange(n_objects, dtype=np.uint8), group_words(m)


def _dptr(x):
    """Device pointer of a torch tensor / int / None."""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, int):
        return C.c_void_p(x)
    return C.c_void_p(x.data_ptr())


def _listed_arrays(ids, shape, tf_container, tf_shape, swapped):
    """The host arrays of a height-field / octree batch as the library takes them: (ids, shape, container poses, shape poses, swapped or
    None, n)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    shape = np.ascontiguousarray(shape, dtype=np.uint32)
    tfc = np.ascontiguousarray(tf_container, dtype=np.float64).reshape(-1, 12)
    tfs = np.ascontiguousarray(tf_shape, dtype=np.float64).reshape(-1, 12)
    n = len(ids)
    if not (len(shape) == len(tfc) == len(tfs) == n):
        raise ValueError("batch arrays must have equal length")
    if swapped is not None:
        swapped = np.ascontiguousarray(swapped, dtype=np.uint8)
        if len(swapped) != n:
            raise ValueError("swapped: one byte per query")
    return ids, shape, tfc, tfs, swapped, n


class Library:
    """hfcl_lib: a shape library resident on one GPU."""

    def __init__(self, shape_library, device=0, options=None):
        """options: {key: value} for hfcl_lib_set_option, applied before the first batch."""
        d = dll()
        self._shapes = np.ascontiguousarray(shape_library.shapes_array())
        self._verts = np.ascontiguousarray(shape_library.vertices_array(), dtype=np.float64)
        self.device = device
        h = d.hfcl_lib_create(abi.ptr(self._shapes), C.c_size_t(len(self._shapes)), abi.ptr(self._verts),
                              C.c_size_t(len(self._verts)), C.c_int(device))
        if not h:
            raise EngineError(abi.ERR_NO_DEVICE, last_error())
        self._h = C.c_void_p(h)
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, key, value):
        """hfcl_lib_set_option: a tuning option by name (the same names, upper-cased behind HFCL_, are the environment fallback)."""
        if isinstance(value, bool):
            value = int(value)
        if isinstance(value, (list, tuple)):
            value = ",".join(str(int(x)) for x in value)
        _check(dll().hfcl_lib_set_option(self._h, str(key).encode(), str(value).encode()))

    def close(self):
        if getattr(self, "_h", None):
            dll().hfcl_lib_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_bvh(self, mesh):
        """Register a BVHModel<OBBRSS> (bvh_builder.Mesh); returns its bvh_index."""
        nodes = np.ascontiguousarray(mesh.nodes)
        verts = np.ascontiguousarray(mesh.vertices, dtype=np.float64)
        tris = np.ascontiguousarray(mesh.triangles, dtype=np.uint32)
        idx = dll().hfcl_lib_add_bvh(self._h, abi.ptr(nodes), C.c_size_t(len(nodes)), abi.ptr(verts),
                                     C.c_size_t(len(verts)), abi.ptr(tris), C.c_size_t(len(tris)))
        if idx < 0:
            raise EngineError(abi.ERR_INVALID_ARGUMENT, last_error())
        return idx

    # ---- what the height-field and octree batch calls share (fn: the C entry point) ----
    def _listed_collide(self, fn, ids, shape, tf_container, tf_shape, req, swapped, max_contacts, want_bound):
        """A *_collide_batch call from host arrays: (records, distance_lower_bound or None, contacts[CONTACT_DTYPE], n_produced)."""
        req = req or abi.default_collision_request()
        ids, shape, tfc, tfs, swapped, n = _listed_arrays(ids, shape, tf_container, tf_shape, swapped)
        out = np.zeros(n, dtype=abi.RESULT_DTYPE)
        dlb = np.zeros(n) if want_bound else None
        contacts = np.zeros(int(max_contacts), dtype=abi.CONTACT_DTYPE)
        nc = C.c_size_t(0)
        _check(fn(self._h, abi.ptr(ids), abi.ptr(shape), abi.ptr(tfc), abi.ptr(tfs), C.c_size_t(n), abi.ptr(swapped), C.byref(req), abi.ptr(out),
                  abi.ptr(dlb), abi.ptr(contacts) if max_contacts else None, C.c_size_t(int(max_contacts)), C.byref(nc)))
        return out, dlb, contacts[:min(nc.value, int(max_contacts))], int(nc.value)

    def _listed_collide_device(self, fn, d_ids, d_shape, d_tf_container, d_tf_shape, n, req, d_out, d_swapped, d_bound, d_contacts, max_contacts,
                               want_count, stream):
        """A *_collide_batch_device call: the number of contacts produced when want_count, else None."""
        nc = C.c_size_t(0)
        _check(fn(self._h, _dptr(d_ids), _dptr(d_shape), _dptr(d_tf_container), _dptr(d_tf_shape), C.c_size_t(n), _dptr(d_swapped), C.byref(req),
                  _dptr(d_out), _dptr(d_bound), _dptr(d_contacts), C.c_size_t(int(max_contacts)), C.byref(nc) if want_count else None,
                  C.c_void_p(stream)))
        return int(nc.value) if want_count else None

    def _listed_distance(self, fn, ids, shape, tf_container, tf_shape, req, swapped, want_visited):
        """A *_distance_batch call from host arrays: the records, or (records, n_visited) when want_visited."""
        req = req or abi.default_distance_request()
        ids, shape, tfc, tfs, swapped, n = _listed_arrays(ids, shape, tf_container, tf_shape, swapped)
        out = np.zeros(n, dtype=abi.RESULT_DTYPE)
        visited = np.zeros(n, dtype=np.uint32) if want_visited else None
        _check(fn(self._h, abi.ptr(ids), abi.ptr(shape), abi.ptr(tfc), abi.ptr(tfs), C.c_size_t(n), abi.ptr(swapped), C.byref(req), abi.ptr(out),
                  abi.ptr(visited)))
        return (out, visited) if want_visited else out

    def _listed_distance_device(self, fn, d_ids, d_shape, d_tf_container, d_tf_shape, n, req, d_out, d_swapped, d_visited, stream):
        """A *_distance_batch_device call."""
        _check(fn(self._h, _dptr(d_ids), _dptr(d_shape), _dptr(d_tf_container), _dptr(d_tf_shape), C.c_size_t(n), _dptr(d_swapped), C.byref(req),
                  _dptr(d_out), _dptr(d_visited), C.c_void_p(stream)))

    # ---- height fields (hfcl_lib_add_hfield, hfcl_hfield_collide_batch*) ----
    def add_hfield(self, x_dim, y_dim, heights, min_height=0.0):
        """Register a HeightField<AABB>; heights: (ny, nx), row 0 = the north edge.  Returns its index on this library."""
        h = np.ascontiguousarray(heights, dtype=np.float64)
        if h.ndim != 2:
            raise ValueError("heights: a (ny, nx) matrix")
        idx = dll().hfcl_lib_add_hfield(self._h, C.c_double(x_dim), C.c_double(y_dim), abi.ptr(h), C.c_size_t(h.shape[0]),
                                        C.c_size_t(h.shape[1]), C.c_double(min_height))
        if idx < 0:
            raise EngineError(abi.ERR_INVALID_ARGUMENT, last_error())
        return idx

    def hfield_count(self):
        return int(dll().hfcl_lib_hfield_count(self._h))

    def clear_hfields(self):
        """Forget every registered height field (indices start at 0 again): hfcl_lib_clear_hfields."""
        _check(dll().hfcl_lib_clear_hfields(self._h))

    def hfield_local_aabb(self, hfield):
        """computeLocalAABB of a registered height field: (min xyz, max xyz)."""
        out = np.zeros(6)
        _check(dll().hfcl_hfield_local_aabb(self._h, C.c_int(int(hfield)), abi.ptr(out)))
        return out

    def hfield_collide(self, hfield, shape, tf_hfield, tf_shape, req=None, swapped=None, max_contacts=0, want_bound=True):
        """Batched collide(HeightField<AABB>, solid) -- swapped[i] = 1: collide(solid, HeightField) -- from host arrays.  Returns
        (records, distance_lower_bound or None, contacts[CONTACT_DTYPE], n_produced)."""
        return self._listed_collide(dll().hfcl_hfield_collide_batch, hfield, shape, tf_hfield, tf_shape, req, swapped, max_contacts, want_bound)

    def hfield_collide_device(self, d_hfield, d_shape, d_tf_hfield, d_tf_shape, n, req, d_out, d_swapped=None, d_bound=None, d_contacts=None,
                              max_contacts=0, want_count=False, stream=0):
        """The same call on device pointers (torch tensors or raw pointers).  Returns the number of contacts produced when want_count
        (the call then waits for the stream), else None."""
        return self._listed_collide_device(dll().hfcl_hfield_collide_batch_device, d_hfield, d_shape, d_tf_hfield, d_tf_shape, n, req, d_out,
                                           d_swapped, d_bound, d_contacts, max_contacts, want_count, stream)

    # ---- octrees (hfcl_lib_add_octree, hfcl_octree_collide_batch*) ----
    def add_octree(self, nodes, resolution, depth=abi.OCTREE_MAX_DEPTH, occupancy_threshold=0.5, free_threshold=0.0):
        """Register an occupancy octree given as a node array (OCTREE_NODE_DTYPE; engine.octree_from_points makes one).  Returns its
        index on this library."""
        nodes = _octree_nodes(nodes)
        idx = dll().hfcl_lib_add_octree(self._h, abi.ptr(nodes) if len(nodes) else None, C.c_size_t(len(nodes)), C.c_double(resolution),
                                        C.c_uint32(int(depth)), C.c_double(occupancy_threshold), C.c_double(free_threshold))
        if idx < 0:
            raise EngineError(abi.ERR_INVALID_ARGUMENT, last_error())
        return idx

    def octree_set_thresholds(self, octree, occupancy_threshold, free_threshold):
        """setOccupancyThres / setFreeThres of a registered octree: hfcl_lib_octree_set_thresholds."""
        _check(dll().hfcl_lib_octree_set_thresholds(self._h, C.c_int(int(octree)), C.c_double(occupancy_threshold), C.c_double(free_threshold)))

    def octree_count(self):
        return int(dll().hfcl_lib_octree_count(self._h))

    def clear_octrees(self):
        """Forget every registered octree (indices start at 0 again): hfcl_lib_clear_octrees."""
        _check(dll().hfcl_lib_clear_octrees(self._h))

    def octree_root_box(self, octree):
        """getRootBV of a registered octree: (min xyz, max xyz)."""
        out = np.zeros(6)
        _check(dll().hfcl_octree_root_box(self._h, C.c_int(int(octree)), abi.ptr(out)))
        return out

    def octree_collide(self, octree, shape, tf_octree, tf_shape, req=None, swapped=None, max_contacts=0, want_bound=True):
        """Batched collide(OcTree, solid) -- swapped[i] = 1: the caller's order was collide(solid, OcTree), which the reference answers
        with the octree-first result (bit 23 of the status alone changes) -- from host arrays.  Returns (records,
        distance_lower_bound or None, contacts[CONTACT_DTYPE], n_produced)."""
        return self._listed_collide(dll().hfcl_octree_collide_batch, octree, shape, tf_octree, tf_shape, req, swapped, max_contacts, want_bound)

    def octree_collide_device(self, d_octree, d_shape, d_tf_octree, d_tf_shape, n, req, d_out, d_swapped=None, d_bound=None, d_contacts=None,
                              max_contacts=0, want_count=False, stream=0):
        """The same call on device pointers (torch tensors or raw pointers).  Returns the number of contacts produced when want_count
        (the call then waits for the stream), else None."""
        return self._listed_collide_device(dll().hfcl_octree_collide_batch_device, d_octree, d_shape, d_tf_octree, d_tf_shape, n, req, d_out,
                                           d_swapped, d_bound, d_contacts, max_contacts, want_count, stream)

    def octree_mesh_collide(self, octree, shape, tf_octree, tf_mesh, req=None, swapped=None, max_contacts=0, want_bound=True):
        """Batched collide(OcTree, BVHModel<OBBRSS>) from host arrays: shape[i] is a BV_OBBRSS row of the library whose bvh_index names
        a mesh registered with add_bvh.  swapped[i] = 1: the caller's order was collide(mesh, OcTree), which the reference answers with
        the octree-first result (bit 23 of the status alone changes).  Returns (records, distance_lower_bound or None,
        contacts[CONTACT_DTYPE] -- b1 the octree node, b2 the triangle --, n_produced)."""
        return self._listed_collide(dll().hfcl_octree_mesh_collide_batch, octree, shape, tf_octree, tf_mesh, req, swapped, max_contacts, want_bound)

    def octree_mesh_collide_device(self, d_octree, d_shape, d_tf_octree, d_tf_mesh, n, req, d_out, d_swapped=None, d_bound=None, d_contacts=None,
                                   max_contacts=0, want_count=False, stream=0):
        """The same call on device pointers (torch tensors or raw pointers).  Returns the number of contacts produced when want_count
        (the call then waits for the stream), else None."""
        return self._listed_collide_device(dll().hfcl_octree_mesh_collide_batch_device, d_octree, d_shape, d_tf_octree, d_tf_mesh, n, req, d_out,
                                           d_swapped, d_bound, d_contacts, max_contacts, want_count, stream)

    def octree_distance(self, octree, shape, tf_octree, tf_shape, req=None, swapped=None, want_visited=False):
        """Batched distance(OcTree, solid) from host arrays: the result of the reference's ordered walk (hppfcl_amd_octree_distance.h).
        swapped[i] = 1: the caller's order was distance(solid, OcTree), which the reference answers with the octree-first result (bit
        23 of the status alone changes).  Returns the records, or (records, n_visited) -- the leaves each walk solved -- when
        want_visited."""
        return self._listed_distance(dll().hfcl_octree_distance_batch, octree, shape, tf_octree, tf_shape, req, swapped, want_visited)

    def octree_distance_device(self, d_octree, d_shape, d_tf_octree, d_tf_shape, n, req, d_out, d_swapped=None, d_visited=None, stream=0):
        """The same call on device pointers (torch tensors or raw pointers): asynchronous on `stream`, nothing is read back."""
        self._listed_distance_device(dll().hfcl_octree_distance_batch_device, d_octree, d_shape, d_tf_octree, d_tf_shape, n, req, d_out,
                                     d_swapped, d_visited, stream)

    def octree_mesh_distance(self, octree, shape, tf_octree, tf_mesh, req=None, swapped=None, want_visited=False):
        """Batched distance(OcTree, BVHModel<OBBRSS>) from host arrays: the result of the reference's ordered dual walk
        (hppfcl_amd_octree_mesh_distance.h).  shape[i] is a BV_OBBRSS row of the library whose bvh_index names a mesh registered with
        add_bvh.  swapped[i] = 1: the caller's order was distance(mesh, OcTree), which the reference answers with the octree-first
        result (bit 23 of the status alone changes).  b1 is the octree node, b2 the triangle.  Returns the records, or (records,
        n_visited) -- the (leaf, triangle) pairs each walk solved -- when want_visited."""
        return self._listed_distance(dll().hfcl_octree_mesh_distance_batch, octree, shape, tf_octree, tf_mesh, req, swapped, want_visited)

    def octree_mesh_distance_device(self, d_octree, d_shape, d_tf_octree, d_tf_mesh, n, req, d_out, d_swapped=None, d_visited=None, stream=0):
        """The same call on device pointers (torch tensors or raw pointers): asynchronous on `stream`, nothing is read back."""
        self._listed_distance_device(dll().hfcl_octree_mesh_distance_batch_device, d_octree, d_shape, d_tf_octree, d_tf_mesh, n, req, d_out,
                                     d_swapped, d_visited, stream)

    def collide_contacts(self, s1, s2, tf1, tf2, req, max_contacts):
        """Batched collide() returning (records, contacts[CONTACT_DTYPE], n_produced)."""
        s1 = np.ascontiguousarray(s1, dtype=np.uint32)
        s2 = np.ascontiguousarray(s2, dtype=np.uint32)
        tf1 = np.ascontiguousarray(tf1, dtype=np.float64).reshape(-1, 12)
        tf2 = np.ascontiguousarray(tf2, dtype=np.float64).reshape(-1, 12)
        n = len(s1)
        out = np.zeros(n, dtype=abi.RESULT_DTYPE)
        contacts = np.zeros(max_contacts, dtype=abi.CONTACT_DTYPE)
        nc = C.c_size_t(0)
        _check(dll().hfcl_collide_batch_contacts(self._h, abi.ptr(s1), abi.ptr(s2), abi.ptr(tf1), abi.ptr(tf2),
                                                 C.c_size_t(n), C.byref(req), abi.ptr(out), abi.ptr(contacts),
                                                 C.c_size_t(max_contacts), C.byref(nc)))
        return out, contacts[:min(nc.value, max_contacts)], int(nc.value)

    # ---- host-buffer entry points (H2D + kernels + D2H inside the call) ----
    def _host(self, fn, s1, s2, tf1, tf2, req, guess_in, want_guess, pose_width=12):
        s1 = np.ascontiguousarray(s1, dtype=np.uint32)
        s2 = np.ascontiguousarray(s2, dtype=np.uint32)
        tf1 = np.ascontiguousarray(tf1, dtype=np.float64).reshape(-1, pose_width)
        tf2 = np.ascontiguousarray(tf2, dtype=np.float64).reshape(-1, pose_width)
        n = len(s1)
        if not (len(s2) == n and len(tf1) == n and len(tf2) == n):
            raise ValueError("batch arrays must have equal length")
        out = np.zeros(n, dtype=abi.RESULT_DTYPE)
        if guess_in is not None:
            guess_in = np.ascontiguousarray(guess_in, dtype=abi.GUESS_DTYPE)
        gout = np.zeros(n, dtype=abi.GUESS_DTYPE) if want_guess else None
        rc = fn(self._h, abi.ptr(s1), abi.ptr(s2), abi.ptr(tf1), abi.ptr(tf2), C.c_size_t(n), C.byref(req),
                abi.ptr(out), abi.ptr(guess_in), abi.ptr(gout))
        _check(rc)
        return (out, gout) if want_guess else out

    def collide(self, s1, s2, tf1, tf2, req=None, guess_in=None, want_guess=False):
        """Batched hpp::fcl::collide (src/collision.cpp:69-130)."""
        return self._host(dll().hfcl_collide_batch, s1, s2, tf1, tf2, req or abi.default_collision_request(),
                          guess_in, want_guess)

    def distance(self, s1, s2, tf1, tf2, req=None, guess_in=None, want_guess=False):
        """Batched hpp::fcl::distance (src/distance.cpp:60-109)."""
        return self._host(dll().hfcl_distance_batch, s1, s2, tf1, tf2, req or abi.default_distance_request(),
                          guess_in, want_guess)

    def _host_f32(self, fn, s1, s2, pose1, pose2, req):
        s1 = np.ascontiguousarray(s1, dtype=np.uint32)
        s2 = np.ascontiguousarray(s2, dtype=np.uint32)
        p1 = np.ascontiguousarray(pose1, dtype=np.float32).reshape(-1, 7)
        p2 = np.ascontiguousarray(pose2, dtype=np.float32).reshape(-1, 7)
        n = len(s1)
        if not (len(s2) == len(p1) == len(p2) == n):
            raise ValueError("array lengths differ")
        out = np.zeros(n, dtype=abi.RESULT_F32_DTYPE)
        _check(fn(self._h, C.c_void_p(s1.ctypes.data), C.c_void_p(s2.ctypes.data), C.c_void_p(p1.ctypes.data), C.c_void_p(p2.ctypes.data),
                  C.c_size_t(n), C.byref(req), C.c_void_p(out.ctypes.data)))
        return out

    def collide_f32(self, s1, s2, pose1, pose2, req=None):
        """collide() through the fp32 path from host arrays: (n, 7) float32 poses (quaternion w, x, y, z + translation), hfcl_result_f32 records."""
        return self._host_f32(dll().hfcl_collide_batch_f32, s1, s2, pose1, pose2, req or abi.default_collision_request())

    def distance_f32(self, s1, s2, pose1, pose2, req=None):
        """distance() through the fp32 path from host arrays (see collide_f32)."""
        return self._host_f32(dll().hfcl_distance_batch_f32, s1, s2, pose1, pose2, req or abi.default_distance_request())

    def collide_qt(self, s1, s2, pose1, pose2, req=None, guess_in=None, want_guess=False):
        """collide() with compact host poses: (n, 7) float64 = quaternion (w, x, y, z) + translation."""
        return self._host(dll().hfcl_collide_batch_qt, s1, s2, pose1, pose2, req or abi.default_collision_request(),
                          guess_in, want_guess, pose_width=7)

    def distance_qt(self, s1, s2, pose1, pose2, req=None, guess_in=None, want_guess=False):
        """distance() with compact host poses: (n, 7) float64 = quaternion (w, x, y, z) + translation."""
        return self._host(dll().hfcl_distance_batch_qt, s1, s2, pose1, pose2, req or abi.default_distance_request(),
                          guess_in, want_guess, pose_width=7)

    def set_convex_neighbors(self, shape_id, offsets, neighbors):
        """ConvexBase::neighbors of one convex shape (CSR: offsets[num_points + 1], vertex indices relative to the
        shape): large hulls that have them hill-climb instead of scanning (hfcl_lib_set_convex_neighbors)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        ids = np.ascontiguousarray(neighbors, dtype=np.uint32)
        _check(dll().hfcl_lib_set_convex_neighbors(self._h, C.c_uint32(int(shape_id)), C.c_void_p(off.ctypes.data),
                                                   C.c_void_p(ids.ctypes.data)))

    def climb_min(self):
        """Smallest hull (vertices) this library answers by hill-climbing a registered adjacency (hfcl_lib_climb_min)."""
        return int(dll().hfcl_lib_climb_min(self._h))

    def set_host_chunk(self, pairs):
        """Pairs per chunk of the host-buffer pipeline (0 = automatic)."""
        dll().hfcl_lib_set_host_chunk(self._h, C.c_size_t(int(pairs)))

    # ---- device-resident entry points (torch tensors or raw device pointers) ----
    def collide_device(self, d_s1, d_s2, d_tf1, d_tf2, n, req, d_out, d_gin=None, d_gout=None, stream=0):
        _check(dll().hfcl_collide_batch_device(self._h, _dptr(d_s1), _dptr(d_s2), _dptr(d_tf1), _dptr(d_tf2),
                                                C.c_size_t(n), C.byref(req), _dptr(d_out), _dptr(d_gin),
                                                _dptr(d_gout), C.c_void_p(stream)))

    def distance_device(self, d_s1, d_s2, d_tf1, d_tf2, n, req, d_out, d_gin=None, d_gout=None, stream=0):
        _check(dll().hfcl_distance_batch_device(self._h, _dptr(d_s1), _dptr(d_s2), _dptr(d_tf1), _dptr(d_tf2),
                                                 C.c_size_t(n), C.byref(req), _dptr(d_out), _dptr(d_gin),
                                                 _dptr(d_gout), C.c_void_p(stream)))

    def distance_device_f32(self, d_s1, d_s2, d_pose1, d_pose2, n, req, d_out, stream=0):
        _check(dll().hfcl_distance_batch_device_f32(self._h, _dptr(d_s1), _dptr(d_s2), _dptr(d_pose1),
                                                     _dptr(d_pose2), C.c_size_t(n), C.byref(req), _dptr(d_out),
                                                     C.c_void_p(stream)))

    def collide_device_f32(self, d_s1, d_s2, d_pose1, d_pose2, n, req, d_out, stream=0):
        _check(dll().hfcl_collide_batch_device_f32(self._h, _dptr(d_s1), _dptr(d_s2), _dptr(d_pose1),
                                                    _dptr(d_pose2), C.c_size_t(n), C.byref(req), _dptr(d_out),
                                                    C.c_void_p(stream)))

    # ---- contact patches of collide() records (hfcl_contact_patch_batch*) ----
    def contact_patch_max_points(self, req=None):
        """Upper bound on the points of any patch of this library under `req` (hfcl_contact_patch_max_points)."""
        cap = C.c_uint32(0)
        _check(dll().hfcl_contact_patch_max_points(self._h, C.byref(req or abi.default_patch_request()), C.byref(cap)))
        return int(cap.value)

    def contact_patch(self, s1, s2, tf1, tf2, records, guesses=None, req=None, points_capacity=None):
        """Batched hpp::fcl::computeContactPatch on the records of collide() for the same pairs.  Returns
        (patches[PATCH_DTYPE], points (n, points_capacity, 2) float64 in each patch's frame).  guesses: the
        GUESS_DTYPE records collide(..., want_guess=True) returned, or None."""
        req = req or abi.default_patch_request()
        s1 = np.ascontiguousarray(s1, dtype=np.uint32)
        s2 = np.ascontiguousarray(s2, dtype=np.uint32)
        tf1 = np.ascontiguousarray(tf1, dtype=np.float64).reshape(-1, 12)
        tf2 = np.ascontiguousarray(tf2, dtype=np.float64).reshape(-1, 12)
        records = np.ascontiguousarray(records, dtype=abi.RESULT_DTYPE)
        n = len(s1)
        if not (len(s2) == len(tf1) == len(tf2) == len(records) == n):
            raise ValueError("batch arrays must have equal length")
        if guesses is not None:
            guesses = np.ascontiguousarray(guesses, dtype=abi.GUESS_DTYPE)
            if len(guesses) != n:
                raise ValueError("guesses must have one record per pair")
        if points_capacity is None:
            points_capacity = self.contact_patch_max_points(req)
        out = np.zeros(n, dtype=abi.PATCH_DTYPE)
        pts = np.zeros((n, int(points_capacity), 2), dtype=np.float64)
        _check(dll().hfcl_contact_patch_batch(self._h, abi.ptr(s1), abi.ptr(s2), abi.ptr(tf1), abi.ptr(tf2), abi.ptr(records),
                                              abi.ptr(guesses), C.c_size_t(n), C.byref(req), C.c_uint32(int(points_capacity)),
                                              abi.ptr(out), abi.ptr(pts)))
        return out, pts

    def contact_patch_device(self, d_s1, d_s2, d_tf1, d_tf2, d_records, n, req, points_capacity, d_out, d_points,
                             d_guesses=None, stream=0):
        """hfcl_contact_patch_batch_device: device buffers (torch tensors or pointers), asynchronous on `stream`.
        d_out: n * 112 bytes (PATCH_DTYPE records), d_points: n * points_capacity * 2 doubles."""
        _check(dll().hfcl_contact_patch_batch_device(self._h, _dptr(d_s1), _dptr(d_s2), _dptr(d_tf1), _dptr(d_tf2),
                                                     _dptr(d_records), _dptr(d_guesses), C.c_size_t(n), C.byref(req),
                                                     C.c_uint32(int(points_capacity)), _dptr(d_out), _dptr(d_points),
                                                     C.c_void_p(stream)))

    def compact_results_device(self, d_records, n, d_out, f32=False, stream=0):
        """Full device records -> hfcl_result_compact{,_f32} records (24 / 8 B): the multi-GPU exchange format."""
        fn = dll().hfcl_compact_results_device_f32 if f32 else dll().hfcl_compact_results_device
        _check(fn(self._h, _dptr(d_records), C.c_size_t(n), _dptr(d_out), C.c_void_p(stream)))

    def scene(self, object_shape, pairs):
        """hfcl_scene_create: the object -> shape table and the (n_pairs, 2) list of object pairs, resident on this
        library's device (see Scene).  Close the scene before the library."""
        return Scene(self, object_shape, pairs)

    # ---- instrumentation ----
    def set_split(self, parts):
        """2: large batches run as two halves on two streams (hfcl_lib_set_split); 1: one stream."""
        dll().hfcl_lib_set_split(self._h, C.c_int(int(parts)))

    def get_split(self):
        return int(dll().hfcl_lib_get_split(self._h))

    def last_split_parts(self):
        """1 or 2: how the last batch actually ran."""
        return int(dll().hfcl_lib_last_split_parts(self._h))

    def set_kernel_timing(self, on):
        """Per-kernel HIP events on/off (on by default; off saves two stream markers per launch)."""
        dll().hfcl_lib_set_kernel_timing(self._h, C.c_int(1 if on else 0))

    def last_kernel_ms(self):
        return float(dll().hfcl_last_kernel_ms(self._h))

    def last_kernel_name(self):
        return dll().hfcl_last_kernel_name(self._h).decode()

    def last_kernel_breakdown(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_double * 16)()
        k = dll().hfcl_last_kernel_breakdown(self._h, names, ms, 16)
        return [(names[i].decode(), float(ms[i])) for i in range(k)]

    def last_bucket_counts(self):
        out = (C.c_uint32 * 12)()
        dll().hfcl_last_bucket_counts(self._h, out)
        keys = ["closed", "prim", "cc", "pc", "cp", "bvh", "unsupported", "large", "bvh_shape", "tri", "epa_queue", "epa_overflow"]
        counts = dict(zip(keys, [int(v) for v in out]))
        if hasattr(dll(), "hfcl_last_redo_count"):  # fp32 calls: pairs solved again in fp64
            counts["redo"] = int(dll().hfcl_last_redo_count(self._h))
        return counts


    def last_epa_handed_over(self):
        """fp32 convex x convex polytopes of the last call that outgrew k_epa_loop's block and were continued by the next tier."""
        return int(dll().hfcl_last_epa_handed_over(self._h))

    def last_ordered_reruns(self):
        """distance() on meshes, last call: walks a wave continued / of those re-run in the reference's order, mesh x mesh then mesh x solid."""
        out = (C.c_uint32 * 4)()
        dll().hfcl_last_ordered_reruns(self._h, out)
        return dict(zip(["mesh_continued", "mesh_rerun", "solid_continued", "solid_rerun"], [int(v) for v in out]))


def spatial_order(centres):
    """A permutation of points (n, 3) by Morton code: 21 bits a coordinate over the points' bounding box, ties by index.  Consecutive
    objects of centres[spatial_order(centres)] are neighbours in space, which is what the tile boxes of Scene.set_environment need."""
    p = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros(0, dtype=np.int64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    scale = np.where(hi > lo, (2 ** 21 - 1) / np.where(hi > lo, hi - lo, 1.0), 0.0)
    q = np.clip(np.nan_to_num((p - lo) * scale), 0, 2 ** 21 - 1).astype(np.uint64)

    def spread(x):  # 21 bits -> every third bit of 63
        x = (x | (x << np.uint64(32))) & np.uint64(0x1F00000000FFFF)
        x = (x | (x << np.uint64(16))) & np.uint64(0x1F0000FF0000FF)
        x = (x | (x << np.uint64(8))) & np.uint64(0x100F00F00F00F00F)
        x = (x | (x << np.uint64(4))) & np.uint64(0x10C30C30C30C30C3)
        x = (x | (x << np.uint64(2))) & np.uint64(0x1249249249249249)
        return x
    code = spread(q[:, 0]) | (spread(q[:, 1]) << np.uint64(1)) | (spread(q[:, 2]) << np.uint64(2))
    return np.argsort(code, kind="stable")


class Scene:
    """hfcl_scene: objects (a shape each), a list of object pairs, and queries that evaluate the list for n_conf pose
    tables.  Query c * n_pairs + p is pair p of configuration c; its record is the per-pair call's record."""

    def __init__(self, library, object_shape, pairs):
        d = dll()
        self.library = library
        ids = np.ascontiguousarray(object_shape, dtype=np.uint32).reshape(-1)
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        h = d.hfcl_scene_create(library._h, abi.ptr(ids), C.c_size_t(len(ids)), abi.ptr(pr), C.c_size_t(len(pr)))
        if not h:  # (hfcl_scene_create has no return code: its message names the causes that are not an invalid argument)
            msg = last_error()
            code = abi.ERR_LIMIT if msg.startswith("HFCL_ERR_LIMIT: ") else abi.ERR_HIP if msg.startswith("HFCL_ERR_HIP: ") else abi.ERR_INVALID_ARGUMENT
            raise EngineError(code, msg)
        self._h = C.c_void_p(h)

    def close(self):
        if getattr(self, "_h", None):
            dll().hfcl_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            if getattr(self.library, "_h", None):  # (a scene must not outlive its library)
                self.close()
        except Exception:
            pass

    @property
    def n_objects(self):
        return int(dll().hfcl_scene_num_objects(self._h))

    @property
    def n_pairs(self):
        return int(dll().hfcl_scene_num_pairs(self._h))

    @property
    def n_groups(self):
        """hfcl_scene_num_groups: 0 without groups."""
        return int(dll().hfcl_scene_num_groups(self._h))

    def set_groups(self, object_group, collides):
        """hfcl_scene_set_groups: a group per object (uint8[n_objects]) and the symmetric group matrix -- a (G, G) bool matrix or G
        uint64 words, bit h of word g set = objects of groups g and h may be listed as a pair.  The lists of self_pairs* / collide_self /
        distance_self then hold the pairs that touch AND whose groups may pair."""
        g = np.asarray(object_group)
        if g.shape != (self.n_objects,) or g.size and (g.min() < 0 or g.max() > 255):
            raise ValueError("object_group: one group in 0..255 per object")
        g = np.ascontiguousarray(g, dtype=np.uint8)
        w = group_words(collides)
        _check(dll().hfcl_scene_set_groups(self._h, abi.ptr(g), C.c_size_t(len(w)), abi.ptr(w)))

    def clear_groups(self):
        """hfcl_scene_clear_groups: back to every touching pair."""
        _check(dll().hfcl_scene_clear_groups(self._h))

    def set_pairs(self, pairs):
        """hfcl_scene_set_pairs: a new pair list over the same objects (a new broadphase pass)."""
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        _check(dll().hfcl_scene_set_pairs(self._h, abi.ptr(pr), C.c_size_t(len(pr))))

    def _table(self, object_tf, dtype, width):
        tf = np.ascontiguousarray(object_tf, dtype=dtype)
        if tf.ndim < 2 or tf.shape[-1] != width:
            raise ValueError("pose table must have shape (n_conf, n_objects, %d) or (n_objects, %d)" % (width, width))
        tf = tf.reshape(-1, self.n_objects, width) if self.n_objects else tf.reshape(0, 0, width)
        return tf

    def _host(self, fn, object_tf, req, records, summary, guess_in, want_guess, f32):
        tf = self._table(object_tf, np.float32 if f32 else np.float64, 7 if f32 else 12)
        n_conf, n = len(tf), len(tf) * self.n_pairs
        out = np.zeros(n, dtype=abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE) if records else None
        summ = np.zeros(n_conf, dtype=abi.SCENE_SUMMARY_DTYPE) if summary else None
        args = [self._h, abi.ptr(tf), C.c_size_t(n_conf), C.byref(req), abi.ptr(out), abi.ptr(summ)]
        gout = None
        if not f32:
            if guess_in is not None:
                guess_in = np.ascontiguousarray(guess_in, dtype=abi.GUESS_DTYPE)
                if len(guess_in) != n:
                    raise ValueError("guess_in must have one record per query")
            gout = np.zeros(n, dtype=abi.GUESS_DTYPE) if want_guess else None
            args += [abi.ptr(guess_in), abi.ptr(gout)]
        _check(fn(*args))
        res = tuple(x for x, on in ((out, records), (summ, summary), (gout, want_guess and not f32)) if on)
        return res[0] if len(res) == 1 else res

    def collide(self, object_tf, req=None, records=True, summary=True, guess_in=None, want_guess=False):
        """hfcl_scene_collide.  Returns what was asked for, in the order (records, summaries, guesses); a single item bare."""
        return self._host(dll().hfcl_scene_collide, object_tf, req or abi.default_collision_request(), records, summary, guess_in,
                          want_guess, False)

    def distance(self, object_tf, req=None, records=True, summary=True, guess_in=None, want_guess=False):
        return self._host(dll().hfcl_scene_distance, object_tf, req or abi.default_distance_request(), records, summary, guess_in,
                          want_guess, False)

    def collide_f32(self, object_pose, req=None, records=True, summary=True):
        """(n_conf, n_objects, 7) float32 poses (quaternion w, x, y, z + translation), hfcl_result_f32 records."""
        return self._host(dll().hfcl_scene_collide_f32, object_pose, req or abi.default_collision_request(), records, summary, None,
                          False, True)

    def distance_f32(self, object_pose, req=None, records=True, summary=True):
        return self._host(dll().hfcl_scene_distance_f32, object_pose, req or abi.default_distance_request(), records, summary, None,
                          False, True)

    # device forms: torch tensors or raw device pointers, asynchronous on `stream`; d_out / d_summary may each be None
    def collide_device(self, d_object_tf, n_conf, req, d_out=None, d_summary=None, d_gin=None, d_gout=None, stream=0):
        _check(dll().hfcl_scene_collide_device(self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), C.byref(req), _dptr(d_out),
                                               _dptr(d_summary), _dptr(d_gin), _dptr(d_gout), C.c_void_p(stream)))

    def distance_device(self, d_object_tf, n_conf, req, d_out=None, d_summary=None, d_gin=None, d_gout=None, stream=0):
        _check(dll().hfcl_scene_distance_device(self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), C.byref(req), _dptr(d_out),
                                                _dptr(d_summary), _dptr(d_gin), _dptr(d_gout), C.c_void_p(stream)))

    def collide_device_f32(self, d_object_pose, n_conf, req, d_out=None, d_summary=None, stream=0):
        _check(dll().hfcl_scene_collide_device_f32(self._h, _dptr(d_object_pose), C.c_size_t(int(n_conf)), C.byref(req), _dptr(d_out),
                                                   _dptr(d_summary), C.c_void_p(stream)))

    def distance_device_f32(self, d_object_pose, n_conf, req, d_out=None, d_summary=None, stream=0):
        _check(dll().hfcl_scene_distance_device_f32(self._h, _dptr(d_object_pose), C.c_size_t(int(n_conf)), C.byref(req), _dptr(d_out),
                                                    _dptr(d_summary), C.c_void_p(stream)))

    # ---- the pair list culled per configuration on the device (include/hppfcl_amd_cull.h) ----
    def _any_table(self, object_tf):
        """The pose table and whether it is the fp32 form: by dtype (float32) or by its last dimension (7)."""
        a = np.asarray(object_tf)
        f32 = a.dtype == np.float32 or (a.ndim >= 2 and a.shape[-1] == 7)
        return self._table(a, np.float32 if f32 else np.float64, 7 if f32 else 12), f32

    def world_aabbs(self, object_tf):
        """hfcl_scene_world_aabbs{,_f32}: (n_conf, n_objects, 6) world boxes (min xyz, max xyz), computed on the device."""
        tf, f32 = self._any_table(object_tf)
        out = np.zeros((len(tf), self.n_objects, 6), dtype=np.float64)
        fn = dll().hfcl_scene_world_aabbs_f32 if f32 else dll().hfcl_scene_world_aabbs
        _check(fn(self._h, abi.ptr(tf), C.c_size_t(len(tf)), abi.ptr(out)))
        return out

    def cull(self, object_tf, inflate=0.0):
        """hfcl_scene_cull{,_f32}: (query_ids uint64 ascending, conf_begin uint64[n_conf + 1]) of the queries q = c * n_pairs + p whose two
        world boxes, each grown by `inflate`, touch."""
        tf, f32 = self._any_table(object_tf)
        fn = dll().hfcl_scene_cull_f32 if f32 else dll().hfcl_scene_cull
        n = C.c_size_t(0)
        conf_begin = np.zeros(len(tf) + 1, dtype=np.uint64)
        capacity = self._list_guess(len(tf))
        while True:  # (at most twice: a list longer than the guess is refused with its length, and the call repeated with that)
            ids = np.zeros(capacity, dtype=np.uint64)
            rc = fn(self._h, abi.ptr(tf), C.c_size_t(len(tf)), C.c_double(inflate), abi.ptr(ids), C.c_size_t(capacity), abi.ptr(conf_begin),
                    C.byref(n))
            if rc != abi.ERR_LIMIT or n.value <= capacity:
                break
            capacity = n.value
        _check(rc)
        return ids[:n.value], conf_begin

    def _list_guess(self, n_conf):
        """Size of the outputs of a culled call when the caller names none: an eighth of the queries (at least 1024, at most all)."""
        total = n_conf * self.n_pairs
        return min(total, max(total // 8, 1024))

    def _culled(self, kind, object_tf, inflate, req, records, summary, guess_in, want_guess, capacity, want_ids):
        tf, f32 = self._any_table(object_tf)
        d = dll()
        n_conf = len(tf)
        fn = getattr(d, "hfcl_scene_%s_culled%s" % (kind, "_f32" if f32 else ""))
        if not (records or want_ids or want_guess):
            capacity = 0  # (summaries only: nothing is sized by the list)
        # no capacity named: a guess; a list that outgrows it is refused after the cull, before any narrow-phase work, with its length,
        # and the call is made once more with that
        retry = capacity is None
        if retry:
            capacity = self._list_guess(n_conf)
        out = np.zeros(capacity, dtype=abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE) if records else None
        ids = np.zeros(capacity, dtype=np.uint64) if records or want_ids or want_guess else None
        conf_begin = np.zeros(n_conf + 1, dtype=np.uint64)
        summ = np.zeros(n_conf, dtype=abi.SCENE_SUMMARY_DTYPE) if summary else None
        n = C.c_size_t(0)
        args = [self._h, abi.ptr(tf), C.c_size_t(n_conf), C.c_double(inflate), C.byref(req), abi.ptr(out), C.c_size_t(capacity), abi.ptr(ids),
                abi.ptr(conf_begin), abi.ptr(summ)]
        gout = None
        if not f32:
            if guess_in is not None:
                guess_in = np.ascontiguousarray(guess_in, dtype=abi.GUESS_DTYPE)
            gout = np.zeros(capacity, dtype=abi.GUESS_DTYPE) if want_guess else None
            args += [abi.ptr(guess_in), abi.ptr(gout)]
        rc = fn(*args, C.byref(n))
        if rc == abi.ERR_LIMIT and retry and n.value > capacity:
            return self._culled(kind, tf, inflate, req, records, summary, guess_in, want_guess, n.value, want_ids)
        _check(rc)
        k = n.value
        res = (out[:k] if records else None, ids[:k] if ids is not None else None, conf_begin, summ)
        return res + (gout[:k],) if want_guess and not f32 else res

    def collide_culled(self, object_tf, inflate=0.0, req=None, records=True, summary=True, guess_in=None, want_guess=False, capacity=None,
                       want_ids=True):
        """hfcl_scene_collide_culled{,_f32}: (records, query_ids, conf_begin, summaries[, guesses]); record k is for query_ids[k] and equals
        the unculled call's record of that query.  records / summary False: None in its place.  capacity: size of the outputs; a smaller one
        than the list raises ERR_LIMIT.  Default: an eighth of the queries -- one call, the table crosses the link once; a list longer
        than that costs a second call (the first is refused after the cull, before any narrow-phase work).  records=False, want_ids=False: the summaries (and conf_begin) alone, one call, no record
        or id leaves the device."""
        return self._culled("collide", object_tf, inflate, req or abi.default_collision_request(), records, summary, guess_in, want_guess, capacity,
                            want_ids)

    def distance_culled(self, object_tf, inflate=0.0, req=None, records=True, summary=True, guess_in=None, want_guess=False, capacity=None,
                        want_ids=True):
        return self._culled("distance", object_tf, inflate, req or abi.default_distance_request(), records, summary, guess_in, want_guess, capacity,
                            want_ids)

    # device forms: torch tensors or raw device pointers, asynchronous on `stream`
    def world_aabbs_device(self, d_object_tf, n_conf, d_aabbs, f32=False, stream=0):
        fn = dll().hfcl_scene_world_aabbs_device_f32 if f32 else dll().hfcl_scene_world_aabbs_device
        _check(fn(self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), _dptr(d_aabbs), C.c_void_p(stream)))

    def cull_device(self, d_object_tf, n_conf, inflate, d_query_ids, capacity, d_conf_begin, d_n_listed, f32=False, stream=0):
        """hfcl_scene_cull_device{,_f32}: *d_n_listed is the true count, ids past `capacity` are not written; nothing is read back."""
        fn = dll().hfcl_scene_cull_device_f32 if f32 else dll().hfcl_scene_cull_device
        _check(fn(self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), C.c_double(inflate), _dptr(d_query_ids), C.c_size_t(int(capacity)),
                  _dptr(d_conf_begin), _dptr(d_n_listed), C.c_void_p(stream)))

    def collide_listed_device(self, d_object_tf, n_conf, d_query_ids, n_listed, d_conf_begin, req, d_out=None, d_summary=None, d_gin=None,
                              d_gout=None, stream=0):
        """hfcl_scene_collide_listed_device: the ids (ascending, below n_conf * n_pairs) are not checked."""
        _check(dll().hfcl_scene_collide_listed_device(self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), _dptr(d_query_ids),
                                                      C.c_size_t(int(n_listed)), _dptr(d_conf_begin), C.byref(req), _dptr(d_out),
                                                      _dptr(d_summary), _dptr(d_gin), _dptr(d_gout), C.c_void_p(stream)))

    def distance_listed_device(self, d_object_tf, n_conf, d_query_ids, n_listed, d_conf_begin, req, d_out=None, d_summary=None, d_gin=None,
                               d_gout=None, stream=0):
        _check(dll().hfcl_scene_distance_listed_device(self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), _dptr(d_query_ids),
                                                       C.c_size_t(int(n_listed)), _dptr(d_conf_begin), C.byref(req), _dptr(d_out),
                                                       _dptr(d_summary), _dptr(d_gin), _dptr(d_gout), C.c_void_p(stream)))

    def collide_listed_device_f32(self, d_object_pose, n_conf, d_query_ids, n_listed, d_conf_begin, req, d_out=None, d_summary=None, stream=0):
        _check(dll().hfcl_scene_collide_listed_device_f32(self._h, _dptr(d_object_pose), C.c_size_t(int(n_conf)), _dptr(d_query_ids),
                                                          C.c_size_t(int(n_listed)), _dptr(d_conf_begin), C.byref(req), _dptr(d_out),
                                                          _dptr(d_summary), C.c_void_p(stream)))

    def distance_listed_device_f32(self, d_object_pose, n_conf, d_query_ids, n_listed, d_conf_begin, req, d_out=None, d_summary=None, stream=0):
        _check(dll().hfcl_scene_distance_listed_device_f32(self._h, _dptr(d_object_pose), C.c_size_t(int(n_conf)), _dptr(d_query_ids),
                                                           C.c_size_t(int(n_listed)), _dptr(d_conf_begin), C.byref(req), _dptr(d_out),
                                                           _dptr(d_summary), C.c_void_p(stream)))

    # ---- the self-collision pairs per configuration, made on the device (include/hppfcl_amd_pairs.h) ----
    def _pairs_guess(self, n_conf):
        """Size of the outputs of a self-pairs call when the caller names none: 16 entries per (configuration, object), at most all pairs."""
        n = self.n_objects
        return min(n_conf * (n * (n - 1) // 2), max(16 * n_conf * n, 1024))

    def self_pairs(self, object_tf, inflate=0.0):
        """hfcl_scene_self_pairs{,_f32}: (pairs uint32 (n_listed, 2), conf_begin uint64[n_conf + 1]) -- for configuration c, then i, then j
        ascending, every (i < j) whose two world boxes, each grown by `inflate`, touch.  The scene's own pair list plays no part."""
        tf, f32 = self._any_table(object_tf)
        fn = dll().hfcl_scene_self_pairs_f32 if f32 else dll().hfcl_scene_self_pairs
        n = C.c_size_t(0)
        conf_begin = np.zeros(len(tf) + 1, dtype=np.uint64)
        capacity = self._pairs_guess(len(tf))
        while True:  # (at most twice: a list longer than the guess is refused with its length, and the call repeated with that)
            pairs = np.zeros((capacity, 2), dtype=np.uint32)
            rc = fn(self._h, abi.ptr(tf), C.c_size_t(len(tf)), C.c_double(inflate), abi.ptr(pairs), C.c_size_t(capacity), abi.ptr(conf_begin),
                    C.byref(n))
            if rc != abi.ERR_LIMIT or n.value <= capacity:
                break
            capacity = n.value
        _check(rc)
        return pairs[:n.value], conf_begin

    def _self(self, kind, object_tf, inflate, req, records, capacity=None, want_guess=False):
        tf, f32 = self._any_table(object_tf)
        n_conf = len(tf)
        fn = getattr(dll(), "hfcl_scene_%s_self%s" % (kind, "_f32" if f32 else ""))
        retry = capacity is None
        if retry:
            capacity = self._pairs_guess(n_conf)
        out = np.zeros(capacity, dtype=abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE) if records else None
        pairs = np.zeros((capacity, 2), dtype=np.uint32)
        conf_begin = np.zeros(n_conf + 1, dtype=np.uint64)
        summ = np.zeros(n_conf, dtype=abi.SCENE_SUMMARY_DTYPE)
        n = C.c_size_t(0)
        args = [self._h, abi.ptr(tf), C.c_size_t(n_conf), C.c_double(inflate), C.byref(req), abi.ptr(out), C.c_size_t(capacity), abi.ptr(pairs),
                abi.ptr(conf_begin), abi.ptr(summ)]
        gout = None
        if not f32:
            gout = np.zeros(capacity, dtype=abi.GUESS_DTYPE) if want_guess else None
            args += [None, abi.ptr(gout)]  # (no guesses in)
        rc = fn(*args, C.byref(n))
        if rc == abi.ERR_LIMIT and retry and n.value > capacity:
            return self._self(kind, tf, inflate, req, records, n.value, want_guess)
        _check(rc)
        k = n.value
        res = (out[:k] if records else None), pairs[:k], conf_begin, summ
        return res + (gout[:k],) if gout is not None else res

    def collide_self(self, object_tf, req=None, inflate=0.0, records=True, want_guess=False):
        """hfcl_scene_collide_self{,_f32}: (records, pairs, conf_begin, summaries) of collide() on the self-collision pairs of every
        configuration; record k is for pairs[k] in the configuration whose conf_begin span holds k, min_pair / first_contact of a summary
        are ranks inside the configuration (pairs[conf_begin[c] + rank]).  records=False: None in their place, no record leaves the device.
        want_guess (fp64 poses): the guesses the records hand out, as a fifth item."""
        return self._self("collide", object_tf, inflate, req or abi.default_collision_request(), records, want_guess=want_guess)

    def distance_self(self, object_tf, req=None, inflate=0.0, records=True, want_guess=False):
        return self._self("distance", object_tf, inflate, req or abi.default_distance_request(), records, want_guess=want_guess)

    def last_pairs_form(self):
        """hfcl_scene_last_pairs_form: how this scene's last list of self pairs was made -- 0 the tiled all-pairs test, 1 its
        wave-per-configuration form, 2 sort and sweep (library option scene_pairs_sorted); -1: none yet."""
        return int(dll().hfcl_scene_last_pairs_form(self._h))

    # device forms: torch tensors or raw device pointers, asynchronous on `stream` (with the library option scene_pairs_sorted set,
    # self_pairs_device waits on `stream` once per chunk: include/hppfcl_amd_pairs_sorted.h)
    def self_pairs_device(self, d_object_tf, n_conf, inflate, d_pairs, capacity, d_conf_begin, d_n_listed, f32=False, stream=0):
        """hfcl_scene_self_pairs_device{,_f32}: *d_n_listed is the true count, entries past `capacity` are not written; nothing is read back."""
        fn = dll().hfcl_scene_self_pairs_device_f32 if f32 else dll().hfcl_scene_self_pairs_device
        _check(fn(self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), C.c_double(inflate), _dptr(d_pairs), C.c_size_t(int(capacity)),
                  _dptr(d_conf_begin), _dptr(d_n_listed), C.c_void_p(stream)))

    def _pairs_device(self, kind, f32, d_object_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, d_gin, d_gout, stream):
        fn = getattr(dll(), "hfcl_scene_%s_pairs_device%s" % (kind, "_f32" if f32 else ""))
        args = [self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), _dptr(d_pairs), C.c_size_t(int(n_listed)), _dptr(d_conf_begin),
                C.byref(req), _dptr(d_out), _dptr(d_summary)]
        if not f32:
            args += [_dptr(d_gin), _dptr(d_gout)]
        _check(fn(*args, C.c_void_p(stream)))

    def collide_pairs_device(self, d_object_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out=None, d_summary=None, d_gin=None,
                             d_gout=None, stream=0):
        """hfcl_scene_collide_pairs_device: the list (i < j < n_objects, conf_begin its spans) is not checked."""
        self._pairs_device("collide", False, d_object_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, d_gin, d_gout, stream)

    def distance_pairs_device(self, d_object_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out=None, d_summary=None, d_gin=None,
                              d_gout=None, stream=0):
        self._pairs_device("distance", False, d_object_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, d_gin, d_gout, stream)

    def collide_pairs_device_f32(self, d_object_pose, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out=None, d_summary=None, stream=0):
        self._pairs_device("collide", True, d_object_pose, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, None, None, stream)

    def distance_pairs_device_f32(self, d_object_pose, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out=None, d_summary=None, stream=0):
        self._pairs_device("distance", True, d_object_pose, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, None, None, stream)

    # ---- a static environment kept on the device (include/hppfcl_amd_env.h) ----
    @property
    def n_moving(self):
        """hfcl_scene_n_moving: the objects in front of the environment; n_objects when none is set."""
        return int(dll().hfcl_scene_n_moving(self._h))

    def set_environment(self, n_moving, env_tf):
        """hfcl_scene_set_environment{,_f32}: objects [n_moving, n_objects) stand still at the poses env_tf -- (n_env, 12) float64 or
        (n_env, 7) float32, the dtype choosing the precision of the _env calls that may follow.  Copied to the device once, with the world
        boxes and a box per tile of 256 consecutive environment objects: put the moving objects first and the environment in a spatial
        order (spatial_order), or the tile boxes skip nothing."""
        a = np.asarray(env_tf)
        f32 = a.dtype == np.float32 or (a.ndim >= 2 and a.shape[-1] == 7)
        width = 7 if f32 else 12
        a = np.ascontiguousarray(a, dtype=np.float32 if f32 else np.float64).reshape(-1, width)
        if len(a) != max(self.n_objects - int(n_moving), 0) and 0 <= int(n_moving) <= self.n_objects:
            raise ValueError("env_tf: one pose row per environment object (n_objects - n_moving)")
        fn = dll().hfcl_scene_set_environment_f32 if f32 else dll().hfcl_scene_set_environment
        _check(fn(self._h, C.c_size_t(int(n_moving)), abi.ptr(a) if len(a) else None))

    def clear_environment(self):
        _check(dll().hfcl_scene_clear_environment(self._h))

    def environment_aabbs(self):
        """hfcl_scene_environment_aabbs: (boxes (n_env, 6), tile boxes (ceil(n_env / 256), 6))."""
        n_env = self.n_objects - self.n_moving
        boxes = np.zeros((n_env, 6), dtype=np.float64)
        tiles = np.zeros(((n_env + 255) // 256, 6), dtype=np.float64)
        _check(dll().hfcl_scene_environment_aabbs(self._h, abi.ptr(boxes), abi.ptr(tiles)))
        return boxes, tiles

    def _moving_table(self, moving_tf):
        """The (n_conf, n_moving, W) table of an _env call and whether it is the fp32 form."""
        a = np.asarray(moving_tf)
        f32 = a.dtype == np.float32 or (a.ndim >= 2 and a.shape[-1] == 7)
        width, k = (7 if f32 else 12), self.n_moving
        a = np.ascontiguousarray(a, dtype=np.float32 if f32 else np.float64)
        if a.ndim < 2 or a.shape[-1] != width:
            raise ValueError("pose table must have shape (n_conf, n_moving, %d)" % width)
        if k == 0:
            return a.reshape(a.shape[0] if a.ndim == 3 else 0, 0, width), f32
        return a.reshape(-1, k, width), f32

    def _env_guess(self, n_conf):
        k = self.n_moving
        return min(n_conf * (k * (k - 1) // 2 + k * (self.n_objects - k)), max(16 * n_conf * k, 1024))

    def env_pairs(self, moving_tf, inflate=0.0):
        """hfcl_scene_env_pairs{,_f32}: (pairs, conf_begin) as self_pairs gives them for the full tables -- moving_tf[c] followed by the
        environment's rows --, less every entry with i >= n_moving."""
        tf, f32 = self._moving_table(moving_tf)
        fn = dll().hfcl_scene_env_pairs_f32 if f32 else dll().hfcl_scene_env_pairs
        n = C.c_size_t(0)
        conf_begin = np.zeros(len(tf) + 1, dtype=np.uint64)
        capacity = self._env_guess(len(tf))
        while True:  # (at most twice, as self_pairs)
            pairs = np.zeros((capacity, 2), dtype=np.uint32)
            rc = fn(self._h, abi.ptr(tf), C.c_size_t(len(tf)), C.c_double(inflate), abi.ptr(pairs), C.c_size_t(capacity), abi.ptr(conf_begin),
                    C.byref(n))
            if rc != abi.ERR_LIMIT or n.value <= capacity:
                break
            capacity = n.value
        _check(rc)
        return pairs[:n.value], conf_begin

    def env_pairs_device(self, d_moving_tf, n_conf, inflate, d_pairs, capacity, d_conf_begin, d_n_listed, f32=False, stream=0):
        """hfcl_scene_env_pairs_device{,_f32}: *d_n_listed is the true count, entries past `capacity` are not written; nothing is read back."""
        fn = dll().hfcl_scene_env_pairs_device_f32 if f32 else dll().hfcl_scene_env_pairs_device
        _check(fn(self._h, _dptr(d_moving_tf), C.c_size_t(int(n_conf)), C.c_double(inflate), _dptr(d_pairs), C.c_size_t(int(capacity)),
                  _dptr(d_conf_begin), _dptr(d_n_listed), C.c_void_p(stream)))

    def _env(self, kind, moving_tf, inflate, req, records, capacity=None, want_guess=False):
        tf, f32 = self._moving_table(moving_tf)
        n_conf = len(tf)
        fn = getattr(dll(), "hfcl_scene_%s_env%s" % (kind, "_f32" if f32 else ""))
        retry = capacity is None
        if retry:
            capacity = self._env_guess(n_conf)
        out = np.zeros(capacity, dtype=abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE) if records else None
        pairs = np.zeros((capacity, 2), dtype=np.uint32)
        conf_begin = np.zeros(n_conf + 1, dtype=np.uint64)
        summ = np.zeros(n_conf, dtype=abi.SCENE_SUMMARY_DTYPE)
        n = C.c_size_t(0)
        args = [self._h, abi.ptr(tf), C.c_size_t(n_conf), C.c_double(inflate), C.byref(req), abi.ptr(out), C.c_size_t(capacity), abi.ptr(pairs),
                abi.ptr(conf_begin), abi.ptr(summ)]
        gout = None
        if not f32:
            gout = np.zeros(capacity, dtype=abi.GUESS_DTYPE) if want_guess else None
            args += [None, abi.ptr(gout)]  # (no guesses in)
        rc = fn(*args, C.byref(n))
        if rc == abi.ERR_LIMIT and retry and n.value > capacity:
            return self._env(kind, tf, inflate, req, records, n.value, want_guess)
        _check(rc)
        k = n.value
        res = (out[:k] if records else None), pairs[:k], conf_begin, summ
        return res + (gout[:k],) if gout is not None else res

    def collide_env(self, moving_tf, req=None, inflate=0.0, records=True, want_guess=False):
        """hfcl_scene_collide_env{,_f32}: collide_self on the env list of a (n_conf, n_moving, W) table."""
        return self._env("collide", moving_tf, inflate, req or abi.default_collision_request(), records, want_guess=want_guess)

    def distance_env(self, moving_tf, req=None, inflate=0.0, records=True, want_guess=False):
        return self._env("distance", moving_tf, inflate, req or abi.default_distance_request(), records, want_guess=want_guess)

    def _env_pairs_device(self, kind, f32, d_moving_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, d_gin, d_gout, stream):
        fn = getattr(dll(), "hfcl_scene_%s_env_pairs_device%s" % (kind, "_f32" if f32 else ""))
        args = [self._h, _dptr(d_moving_tf), C.c_size_t(int(n_conf)), _dptr(d_pairs), C.c_size_t(int(n_listed)), _dptr(d_conf_begin),
                C.byref(req), _dptr(d_out), _dptr(d_summary)]
        if not f32:
            args += [_dptr(d_gin), _dptr(d_gout)]
        _check(fn(*args, C.c_void_p(stream)))

    def collide_env_pairs_device(self, d_moving_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out=None, d_summary=None, d_gin=None,
                                 d_gout=None, stream=0):
        """hfcl_scene_collide_env_pairs_device: the list (i < n_moving, i < j < n_objects, conf_begin its spans) is not checked."""
        self._env_pairs_device("collide", False, d_moving_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, d_gin, d_gout, stream)

    def distance_env_pairs_device(self, d_moving_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out=None, d_summary=None, d_gin=None,
                                  d_gout=None, stream=0):
        self._env_pairs_device("distance", False, d_moving_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, d_gin, d_gout, stream)

    def collide_env_pairs_device_f32(self, d_moving_pose, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out=None, d_summary=None, stream=0):
        self._env_pairs_device("collide", True, d_moving_pose, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, None, None, stream)

    def distance_env_pairs_device_f32(self, d_moving_pose, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out=None, d_summary=None, stream=0):
        self._env_pairs_device("distance", True, d_moving_pose, n_conf, d_pairs, n_listed, d_conf_begin, req, d_out, d_summary, None, None, stream)

    # ---- a height-field terrain under the moving objects (include/hppfcl_amd_terrain.h) ----
    @property
    def n_terrain_objects(self):
        """hfcl_scene_n_terrain_objects: the objects tested against the terrain; 0 when none is set."""
        return int(dll().hfcl_scene_n_terrain_objects(self._h))

    def set_terrain(self, hfield, tf, objects=None):
        """hfcl_scene_set_terrain: height field `hfield` of the library (Library.add_hfield) at pose tf (12 doubles) is the ground under
        the objects listed in `objects` -- strictly ascending object indices; None: every moving object.  Replaces a terrain set before."""
        tf = np.ascontiguousarray(tf, dtype=np.float64).reshape(-1)
        if tf.shape != (12,):
            raise ValueError("tf: one pose row of 12 doubles")
        if objects is None:
            ids, n = None, 0
        else:
            ids = np.ascontiguousarray(objects, dtype=np.uint32).reshape(-1)
            n = len(ids)
            if n == 0:
                ids = np.zeros(1, dtype=np.uint32)  # (an empty list, not "every object": the pointer must not be NULL)
        _check(dll().hfcl_scene_set_terrain(self._h, C.c_uint32(int(hfield)), abi.ptr(tf), abi.ptr(ids), C.c_size_t(n)))

    def clear_terrain(self):
        _check(dll().hfcl_scene_clear_terrain(self._h))

    def collide_terrain(self, moving_tf, req=None, records=True, bounds=True, max_contacts=0):
        """hfcl_scene_collide_terrain on a (n_conf, n_moving, 12) table: query c * n_terrain_objects + k is the terrain against listed
        object k under configuration c.  Returns (records or None, bounds or None, summaries, contacts[CONTACT_DTYPE], n_produced);
        summaries[c]: min_distance the smallest bound of the configuration, min_pair / first_contact OBJECT indices."""
        req = req or abi.default_collision_request()
        tf = np.ascontiguousarray(moving_tf, dtype=np.float64)
        k = self.n_moving
        if tf.ndim < 2 or tf.shape[-1] != 12:
            raise ValueError("pose table must have shape (n_conf, n_moving, 12)")
        tf = tf.reshape(-1, k, 12) if k else tf.reshape(tf.shape[0] if tf.ndim == 3 else 0, 0, 12)
        n_conf, n = len(tf), len(tf) * self.n_terrain_objects
        out = np.zeros(n, dtype=abi.RESULT_DTYPE) if records else None
        dlb = np.zeros(n) if bounds else None
        summ = np.zeros(n_conf, dtype=abi.SCENE_SUMMARY_DTYPE)
        contacts = np.zeros(int(max_contacts), dtype=abi.CONTACT_DTYPE)
        nc = C.c_size_t(0)
        _check(dll().hfcl_scene_collide_terrain(self._h, abi.ptr(tf), C.c_size_t(n_conf), C.byref(req), abi.ptr(out), abi.ptr(dlb), abi.ptr(summ),
                                                abi.ptr(contacts) if max_contacts else None, C.c_size_t(int(max_contacts)), C.byref(nc)))
        return out, dlb, summ, contacts[:min(nc.value, int(max_contacts))], int(nc.value)

    def collide_terrain_device(self, d_moving_tf, n_conf, req, d_out=None, d_bounds=None, d_summary=None, d_contacts=None, max_contacts=0,
                               want_count=False, stream=0):
        """hfcl_scene_collide_terrain_device: torch tensors or raw device pointers, each output may be None.  Returns the number of
        contacts produced when want_count (the call then waits for the stream once more), else None."""
        nc = C.c_size_t(0)
        _check(dll().hfcl_scene_collide_terrain_device(self._h, _dptr(d_moving_tf), C.c_size_t(int(n_conf)), C.byref(req), _dptr(d_out),
                                                       _dptr(d_bounds), _dptr(d_summary), _dptr(d_contacts), C.c_size_t(int(max_contacts)),
                                                       C.byref(nc) if want_count else None, C.c_void_p(stream)))
        return int(nc.value) if want_count else None

    # ---- the per-configuration minimum distance with box-bound pruning (include/hppfcl_amd_nearest.h) ----
    def _nearest(self, object_tf, req, upper_bound, records, f32):
        tf = self._table(object_tf, np.float32 if f32 else np.float64, 7 if f32 else 12)
        n_conf = len(tf)
        summ = np.zeros(n_conf, dtype=abi.SCENE_SUMMARY_DTYPE)
        rec = np.zeros(n_conf, dtype=abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE) if records else None
        n = (C.c_size_t * 2)()
        fn = dll().hfcl_scene_nearest_f32 if f32 else dll().hfcl_scene_nearest
        _check(fn(self._h, abi.ptr(tf), C.c_size_t(n_conf), C.byref(req or abi.default_distance_request()), C.c_double(upper_bound),
                  abi.ptr(summ), abi.ptr(rec), n))
        return summ, rec, (int(n[0]), int(n[1]))

    def nearest(self, object_tf, req=None, upper_bound=float("inf"), records=True):
        """hfcl_scene_nearest: (summaries, min_records, n_evaluated).  min_distance / min_pair of a summary equal those of distance()
        wherever that minimum is <= upper_bound (elsewhere: some value above it, or +inf); min record c is the record of query
        c * n_pairs + min_pair (records=False: None); n_evaluated: the queries the two narrow-phase passes evaluated."""
        return self._nearest(object_tf, req, upper_bound, records, False)

    def nearest_f32(self, object_pose, req=None, upper_bound=float("inf"), records=True):
        """(n_conf, n_objects, 7) float32 poses, hfcl_result_f32 min records."""
        return self._nearest(object_pose, req, upper_bound, records, True)

    def nearest_device(self, d_object_tf, n_conf, req, d_summary, d_min_records=None, upper_bound=float("inf"), stream=0):
        """hfcl_scene_nearest_device: device tensors or pointers, enqueued on `stream`, which the call waits on twice (the two list
        counts).  Returns n_evaluated."""
        n = (C.c_size_t * 2)()
        _check(dll().hfcl_scene_nearest_device(self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), C.byref(req), C.c_double(upper_bound),
                                               _dptr(d_summary), _dptr(d_min_records), n, C.c_void_p(stream)))
        return int(n[0]), int(n[1])

    def nearest_device_f32(self, d_object_pose, n_conf, req, d_summary, d_min_records=None, upper_bound=float("inf"), stream=0):
        n = (C.c_size_t * 2)()
        _check(dll().hfcl_scene_nearest_device_f32(self._h, _dptr(d_object_pose), C.c_size_t(int(n_conf)), C.byref(req),
                                                   C.c_double(upper_bound), _dptr(d_summary), _dptr(d_min_records), n, C.c_void_p(stream)))
        return int(n[0]), int(n[1])

    # ---- the clearance per configuration on device-made pairs (include/hppfcl_amd_nearest_self.h) ----
    def nearest_self(self, object_tf, req=None, upper_bound=float("inf"), records=True):
        """hfcl_scene_nearest_self{,_f32}: (clearance SCENE_CLEARANCE_DTYPE[n_conf], min_records, n_evaluated) from the pose table and the
        scene's groups alone -- no pair list, no inflate.  min_distance / (min_i, min_j) are those of distance() on the explicit list of
        every allowed pair wherever that minimum is <= upper_bound (elsewhere: some value above it, or +inf); min record c is that
        pair's record (records=False: None); n_evaluated: the pairs the two narrow-phase passes evaluated.  (n_conf, n_objects, 7)
        float32 poses take the fp32 path."""
        tf, f32 = self._any_table(object_tf)
        n_conf = len(tf)
        out = np.zeros(n_conf, dtype=abi.SCENE_CLEARANCE_DTYPE)
        rec = np.zeros(n_conf, dtype=abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE) if records else None
        n = (C.c_size_t * 2)()
        fn = dll().hfcl_scene_nearest_self_f32 if f32 else dll().hfcl_scene_nearest_self
        _check(fn(self._h, abi.ptr(tf), C.c_size_t(n_conf), C.byref(req or abi.default_distance_request()), C.c_double(upper_bound),
                  abi.ptr(out), abi.ptr(rec), n))
        return out, rec, (int(n[0]), int(n[1]))

    def nearest_self_device(self, d_object_tf, n_conf, req, d_out, d_min_records=None, upper_bound=float("inf"), stream=0):
        """hfcl_scene_nearest_self_device: device tensors or pointers, enqueued on `stream`, which the call waits on twice (the two list
        counts).  Returns n_evaluated."""
        n = (C.c_size_t * 2)()
        _check(dll().hfcl_scene_nearest_self_device(self._h, _dptr(d_object_tf), C.c_size_t(int(n_conf)), C.byref(req), C.c_double(upper_bound),
                                                    _dptr(d_out), _dptr(d_min_records), n, C.c_void_p(stream)))
        return int(n[0]), int(n[1])

    def nearest_self_device_f32(self, d_object_pose, n_conf, req, d_out, d_min_records=None, upper_bound=float("inf"), stream=0):
        n = (C.c_size_t * 2)()
        _check(dll().hfcl_scene_nearest_self_device_f32(self._h, _dptr(d_object_pose), C.c_size_t(int(n_conf)), C.byref(req),
                                                        C.c_double(upper_bound), _dptr(d_out), _dptr(d_min_records), n, C.c_void_p(stream)))
        return int(n[0]), int(n[1])

    # ---- the clearance of the moving objects among the environment (include/hppfcl_amd_nearest_env.h) ----
    def nearest_env(self, moving_tf, req=None, upper_bound=float("inf"), records=True):
        """hfcl_scene_nearest_env{,_f32}: nearest_self for a scene with an environment set, from a (n_conf, n_moving, W) table of the moving
        objects alone -- (clearance SCENE_CLEARANCE_DTYPE[n_conf], min_records, n_evaluated).  The candidates are the allowed pairs (i, j),
        i < n_moving, i < j < n_objects: never two environment objects; min_i / min_j index the full scene.  Whole tiles of 256 environment
        objects are dropped by a bound of their distance (option scene_nearest_env_prune, default 1): time, never a byte."""
        tf, f32 = self._moving_table(moving_tf)
        n_conf = len(tf)
        out = np.zeros(n_conf, dtype=abi.SCENE_CLEARANCE_DTYPE)
        rec = np.zeros(n_conf, dtype=abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE) if records else None
        n = (C.c_size_t * 2)()
        fn = dll().hfcl_scene_nearest_env_f32 if f32 else dll().hfcl_scene_nearest_env
        _check(fn(self._h, abi.ptr(tf), C.c_size_t(n_conf), C.byref(req or abi.default_distance_request()), C.c_double(upper_bound),
                  abi.ptr(out), abi.ptr(rec), n))
        return out, rec, (int(n[0]), int(n[1]))

    def nearest_env_device(self, d_moving_tf, n_conf, req, d_out, d_min_records=None, upper_bound=float("inf"), stream=0):
        """hfcl_scene_nearest_env_device: device tensors or pointers, enqueued on `stream`, which the call waits on twice (the two list
        counts).  Returns n_evaluated."""
        n = (C.c_size_t * 2)()
        _check(dll().hfcl_scene_nearest_env_device(self._h, _dptr(d_moving_tf), C.c_size_t(int(n_conf)), C.byref(req), C.c_double(upper_bound),
                                                   _dptr(d_out), _dptr(d_min_records), n, C.c_void_p(stream)))
        return int(n[0]), int(n[1])

    def nearest_env_device_f32(self, d_moving_pose, n_conf, req, d_out, d_min_records=None, upper_bound=float("inf"), stream=0):
        n = (C.c_size_t * 2)()
        _check(dll().hfcl_scene_nearest_env_device_f32(self._h, _dptr(d_moving_pose), C.c_size_t(int(n_conf)), C.byref(req),
                                                       C.c_double(upper_bound), _dptr(d_out), _dptr(d_min_records), n, C.c_void_p(stream)))
        return int(n[0]), int(n[1])


def shard_range(n, rank, world):
    """hfcl_shard_range of the C ABI (= sharding.shard_range)."""
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    dll().hfcl_shard_range(C.c_size_t(int(n)), C.c_int(int(rank)), C.c_int(int(world)), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class MultiLibrary:
    """hfcl_multi: replicas of a shape library on several devices of this process (include/hppfcl_amd.h); a batch is cut
    into contiguous shards, one per replica.  `devices` may list a device more than once (host-buffer entry points)."""

    def __init__(self, shape_library, devices=(0,), options=None):
        d = dll()
        self._shapes = np.ascontiguousarray(shape_library.shapes_array())
        self._verts = np.ascontiguousarray(shape_library.vertices_array(), dtype=np.float64)
        self.devices = [int(x) for x in devices]
        dev = (C.c_int * len(self.devices))(*self.devices)
        d.hfcl_multi_create.restype = C.c_void_p
        h = d.hfcl_multi_create(dev, C.c_int(len(self.devices)), abi.ptr(self._shapes), C.c_size_t(len(self._shapes)), abi.ptr(self._verts),
                                C.c_size_t(len(self._verts)))
        if not h:
            raise EngineError(abi.ERR_NO_DEVICE, last_error())
        self._h = C.c_void_p(h)
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, key, value):
        """hfcl_multi_set_option: hfcl_lib_set_option on every replica."""
        if isinstance(value, bool):
            value = int(value)
        if isinstance(value, (list, tuple)):
            value = ",".join(str(int(x)) for x in value)
        _check(dll().hfcl_multi_set_option(self._h, str(key).encode(), str(value).encode()))

    def last_gather(self):
        """hfcl_multi_last_gather: ranks the communicator reports, milliseconds of the all-gather (None: no collective), bytes per rank."""
        ranks, ms, nbytes = C.c_int(0), C.c_double(-1.0), C.c_size_t(0)
        _check(dll().hfcl_multi_last_gather(self._h, C.byref(ranks), C.byref(ms), C.byref(nbytes)))
        return {"ranks": int(ranks.value), "ms": float(ms.value) if ms.value >= 0 else None, "bytes_per_rank": int(nbytes.value)}

    def close(self):
        if getattr(self, "_h", None):
            dll().hfcl_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(dll().hfcl_multi_size(self._h))

    def add_bvh(self, mesh):
        nodes = np.ascontiguousarray(mesh.nodes)
        verts = np.ascontiguousarray(mesh.vertices, dtype=np.float64)
        tris = np.ascontiguousarray(mesh.triangles, dtype=np.uint32)
        idx = dll().hfcl_multi_add_bvh(self._h, abi.ptr(nodes), C.c_size_t(len(nodes)), abi.ptr(verts), C.c_size_t(len(verts)), abi.ptr(tris),
                                       C.c_size_t(len(tris)))
        if idx < 0:
            raise EngineError(abi.ERR_INVALID_ARGUMENT, last_error())
        return idx

    _host = Library._host

    def collide(self, s1, s2, tf1, tf2, req=None, guess_in=None, want_guess=False):
        return self._host(dll().hfcl_collide_batch_multi, s1, s2, tf1, tf2, req or abi.default_collision_request(), guess_in, want_guess)

    def distance(self, s1, s2, tf1, tf2, req=None, guess_in=None, want_guess=False):
        return self._host(dll().hfcl_distance_batch_multi, s1, s2, tf1, tf2, req or abi.default_distance_request(), guess_in, want_guess)

    def collide_f32(self, s1, s2, pose1, pose2, req=None):
        return Library._host_f32(self, dll().hfcl_collide_batch_multi_f32, s1, s2, pose1, pose2, req or abi.default_collision_request())

    def distance_f32(self, s1, s2, pose1, pose2, req=None):
        return Library._host_f32(self, dll().hfcl_distance_batch_multi_f32, s1, s2, pose1, pose2, req or abi.default_distance_request())

    def _gathered(self, fn, d_s1, d_s2, d_tf1, d_tf2, n, req, d_gathered, streams=None):
        """Per-replica lists of device buffers (torch tensors or raw pointers); d_gathered[g]: len(self) * ceil(n / len(self)) records."""
        G = len(self)
        arr = lambda xs: (C.c_void_p * G)(*[_dptr(x) for x in xs])  # noqa: E731
        st = (C.c_void_p * G)(*[C.c_void_p(int(x)) for x in streams]) if streams is not None else None
        _check(fn(self._h, arr(d_s1), arr(d_s2), arr(d_tf1), arr(d_tf2), C.c_size_t(int(n)), C.byref(req), arr(d_gathered), st))

    def collide_device_gathered(self, d_s1, d_s2, d_tf1, d_tf2, n, req, d_gathered, streams=None):
        self._gathered(dll().hfcl_collide_batch_multi_device, d_s1, d_s2, d_tf1, d_tf2, n, req, d_gathered, streams)

    def distance_device_gathered(self, d_s1, d_s2, d_tf1, d_tf2, n, req, d_gathered, streams=None):
        self._gathered(dll().hfcl_distance_batch_multi_device, d_s1, d_s2, d_tf1, d_tf2, n, req, d_gathered, streams)
