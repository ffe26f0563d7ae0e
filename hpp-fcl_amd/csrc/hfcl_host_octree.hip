// hfcl_host_octree.hip -- host side of the octrees (hppfcl_amd_octree.h; the kernels: hfcl_k_octree.hip, the arithmetic:
// hfcl_octree.hpp).  First what the calls are made of: the upload of the tables, the request checks of collide() and of distance(), the
// one check of a batch's meshes (BVH depths, bvh_index), and the four kinds of hfcl_host_listed.hpp -- OctHost and OctMeshHost for
// collide() against solids and against meshes (the listed-leaf pipeline; the mesh kind on a workspace of its own), OctDist and
// OctMeshDist for distance() (one launch per chunk, no workspace, no read-back; the host forms are staged through the collide kinds'
// buffers).  Then the entry points: the validator and the builder from points, the registration on a library, and the eight batch
// calls (hppfcl_amd_octree.h, _octree_distance.h, _octree_mesh.h, _octree_mesh_distance.h), each one call of a body of
// hfcl_host_listed.hpp for its kind.  A further pair kind is a kind struct and two entry points.
#include "hfcl_host_listed.hpp"
#include "hfcl_octree_distance.hpp"
#include "hfcl_octree_mesh_distance.hpp"

#include <cmath>

namespace {

int upload_octrees(hfcl_lib* lib) {
  auto& oc = lib->oct;
  if (!oc.dirty) return HFCL_OK;
  HIP_TRY(hipDeviceSynchronize());  // nothing of this library may still be reading the old tables
  if (oc.h_trees.empty()) {         // (hfcl_lib_clear_octrees: the device buffers stay for the next registration)
    oc.dirty = false;
    return HFCL_OK;
  }
  HIP_TRY(oc.d_trees.grow(oc.h_trees.size()));
  HIP_TRY(oc.d_nodes.grow(std::max<size_t>(oc.h_nodes.size(), 1)));
  HIP_TRY(hipMemcpy(oc.d_trees, oc.h_trees.data(), oc.h_trees.size() * sizeof(hfcl::DOctree), hipMemcpyHostToDevice));
  if (!oc.h_nodes.empty())
    HIP_TRY(hipMemcpy(oc.d_nodes, oc.h_nodes.data(), oc.h_nodes.size() * sizeof(hfcl_octree_node), hipMemcpyHostToDevice));
  oc.dirty = false;
  return HFCL_OK;
}

// what every form checks before any work
int oct_request(const char* who, const hfcl_collision_request* req, QParams<double>& q, bool& skip_all) {
  const int rc = setup_collide<double>(req, q, skip_all);  // num_max_contacts == 0, epa_max_iterations > 64, tolerances, variants
  if (rc) return rc;
  if (req->security_margin < 0 && !skip_all) {  // OctreeCollide (collision_func_matrix.cpp:57-60); NaN is refused by setup_collide's checks or passes as 0 contacts
    set_error(std::string(who) + ": Negative security margin are not handled yet for Octree");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (req->q.gjk_initial_guess != HFCL_GUESS_DEFAULT) {
    set_error(std::string(who) + ": gjk_initial_guess must be DefaultGuess (a cached guess chains from leaf to leaf inside a query, a bounding-volume guess changes the leaf set-up: not done)");
    return HFCL_ERR_LIMIT;
  }
  if (req->distance_upper_bound != Lim<double>::max()) {
    set_error(std::string(who) + ": distance_upper_bound must be its default (a finite bound turns leaf distances into early-stopped bounds: not done)");
    return HFCL_ERR_LIMIT;
  }
  q.gjk.distance_upper_bound = Lim<double>::max();
  return HFCL_OK;
}

// ... and what every distance() form checks
int octd_request(const char* who, const hfcl_distance_request* req, QParams<double>& q) {
  const int rc = setup_distance<double>(req, q);  // a null request, tolerances, epa_max_iterations > 64, variants
  if (rc) return rc;
  if (req->q.gjk_initial_guess != HFCL_GUESS_DEFAULT) {
    set_error(std::string(who) + ": gjk_initial_guess must be DefaultGuess (a cached guess chains from leaf to leaf inside a query, a bounding-volume guess changes the leaf set-up: not done)");
    return HFCL_ERR_LIMIT;
  }
  return HFCL_OK;
}

// What the mesh kinds refuse of a batch: a mesh deeper than the walk's stack, then an OBBRSS row whose bvh_index names no registered
// mesh, each the first in query order.  shape == nullptr (a device form: the ids are not visible): any registered mesh that is too deep,
// lowest index first.  Rows that are no mesh, ids outside the library: refused after this, in the order of every host form
int octm_check_meshes(const char* who, hfcl_lib* lib, const uint32_t* shape, size_t n) {
  auto& depth = lib->oct.mesh_depth;  // the levels of every registered mesh's BVH, computed once per mesh
  for (size_t k = depth.size(); k < lib->h_meshes.size(); ++k) {
    const hfcl_bvh_node* nodes = lib->h_bvh_nodes.data() + lib->h_meshes[k].node_off;
    depth.push_back(hfcl::octm_bvh_depth(lib->h_meshes[k].n_nodes, [&](uint32_t i) { return nodes[i].first_child; }));
  }
  const auto too_deep = [&](size_t k) -> int {
    if (k >= depth.size() || depth[k] <= HFCL_OCTREE_MESH_MAX_BVH_DEPTH) return HFCL_OK;
    set_error(std::string(who) + ": the BVH of mesh " + std::to_string(k) + " has " + (depth[k] == 0xFFFFFFFFu ? std::string("unbounded") : std::to_string(depth[k])) +
              " levels (limit " + std::to_string(HFCL_OCTREE_MESH_MAX_BVH_DEPTH) + ")");
    return HFCL_ERR_LIMIT;
  };
  if (!shape) {
    for (size_t k = 0; k < depth.size(); ++k)
      if (int rc = too_deep(k)) return rc;
    return HFCL_OK;
  }
  const auto is_mesh = [&](size_t i) { return shape[i] < lib->n_shapes && lib->h_shapes[shape[i]].type == HFCL_BV_OBBRSS; };
  for (size_t i = 0; i < n; ++i)
    if (is_mesh(i))
      if (int rc = too_deep(lib->h_shapes[shape[i]].bvh_index)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (is_mesh(i) && size_t(lib->h_shapes[shape[i]].bvh_index) >= lib->h_meshes.size()) {
      set_error(std::string(who) + ": bvh_index outside the registered meshes at query " + std::to_string(i));
      return HFCL_ERR_INVALID_ARGUMENT;
    }
  return HFCL_OK;
}

// ---- the kinds (hfcl_host_listed.hpp) -------------------------------------------------------------------------------------------
struct OctShared {  // what the four have in common
  static constexpr const char* noun = "octree";
  static constexpr const char* a_noun = "an octree";
  static size_t n_containers(const hfcl_lib* lib) { return lib->oct.h_trees.size(); }
  static size_t chunk(const hfcl_lib* lib) { return lib->opt.octree_chunk ? lib->opt.octree_chunk : LISTED_AUTO_CHUNK; }
  static uint64_t item_cap(const hfcl_lib* lib) { return lib->opt.octree_items ? lib->opt.octree_items : LISTED_ITEM_SOFT_CAP; }
  template <class A>
  static void trees(hfcl_lib* lib, A& a) {
    a.n_trees = uint32_t(lib->oct.h_trees.size());
    a.trees = lib->oct.d_trees;
    a.nodes = lib->oct.d_nodes;
  }
};
struct OctMeshShared : OctShared {  // ... and the two against meshes
  static auto& ws(hfcl_lib* lib) { return lib->oct.ws_mesh; }
  static int upload(hfcl_lib* lib) {
    const int rc = upload_octrees(lib);
    return rc ? rc : upload_bvh(lib);
  }
  template <class A>
  static void fill(hfcl_lib* lib, A& a) {
    trees(lib, a);
    a.n_meshes = uint32_t(lib->h_meshes.size());
    a.mnodes = lib->d_nodes64;
    a.mverts = lib->d_bverts64;
    a.mtris = lib->d_btris;
    a.meshes = lib->d_meshes;
  }
  static constexpr auto check = octm_check_meshes;
};

// collide() against solids (hppfcl_amd_octree.h; the kernels: hfcl_k_octree.hip)
struct OctHost : OctShared {
  using Args = hfcl::OctArgs;
  static constexpr const char* limit_who = "hfcl_octree_collide_batch";
  static auto& ws(hfcl_lib* lib) { return lib->oct.ws; }
  static int upload(hfcl_lib* lib) {
    const int rc = upload_octrees(lib);
    return rc ? rc : ensure_local_boxes(lib);
  }
  static void fill(hfcl_lib* lib, Args& a) {
    a.local_boxes = lib->d_local_boxes;
    trees(lib, a);
  }
  static void ids(Args& a, const uint32_t* p) { a.octree = p; }
  static constexpr auto request = oct_request;
  static constexpr auto supported = hfcl_octree_pair_supported;
  static constexpr auto check = listed_no_check;
  static constexpr auto count = launch_oct_count;
  static constexpr auto solve = launch_oct_solve;
};
// collide() against meshes (hppfcl_amd_octree_mesh.h; the kernels: hfcl_k_octree_mesh.hip): a workspace of its own kind of items
struct OctMeshHost : OctMeshShared {
  using Args = hfcl::OctMeshArgs;
  static constexpr const char* limit_who = "hfcl_octree_mesh_collide_batch";
  static void ids(Args& a, const uint32_t* p) { a.octree = p; }
  static constexpr auto request = oct_request;
  static constexpr auto supported = hfcl_octree_mesh_pair_supported;
  static constexpr auto count = launch_octm_count;
  static constexpr auto solve = launch_octm_solve;
};
// distance() to solids (hppfcl_amd_octree_distance.h; the kernel: hfcl_k_octree_distance.hip).  The launches: a workgroup per four
// queries -- the hardware hands the long walks out as they come
struct OctDist : OctShared {
  using Args = hfcl::OctDistArgs;
  static constexpr const char* timer = "k_oct_distance";
  static auto& ws(hfcl_lib* lib) { return lib->oct.ws; }
  static constexpr auto upload = upload_octrees;
  static void fill(hfcl_lib* lib, Args& a) {
    a.verts = lib->d_verts64;
    trees(lib, a);
  }
  static void ptrs(Args& a, const uint32_t* ids, const double* tf_t, const double* tf_s) { a.octree = ids, a.tf_t = tf_t, a.tf_s = tf_s; }
  static constexpr auto request = octd_request;
  static constexpr auto supported = hfcl_octree_distance_pair_supported;
  static constexpr auto check = listed_no_check;
  static void launch(hipStream_t st, const Args& a) { launch_oct_distance(st, a, 1 << 20); }
};
// distance() to meshes (hppfcl_amd_octree_mesh_distance.h; the kernel: hfcl_k_octree_mesh_distance.hip)
struct OctMeshDist : OctMeshShared {
  using Args = hfcl::OctMeshDistArgs;
  static constexpr const char* timer = "k_octm_distance";
  static void ptrs(Args& a, const uint32_t* ids, const double* tf_t, const double* tf_m) { a.octree = ids, a.tf_t = tf_t, a.tf_m = tf_m; }
  static constexpr auto request = octd_request;
  static constexpr auto supported = hfcl_octree_mesh_distance_pair_supported;
  static void launch(hipStream_t st, const Args& a) { launch_octm_distance(st, a, 1 << 20); }
};

}  // namespace

extern "C" {

int hfcl_octree_validate(const hfcl_octree_node* nodes, size_t n_nodes, uint32_t depth) {
  std::string why;
  const int rc = hfcl::oct_validate(nodes, n_nodes, depth, &why);
  if (rc) set_error("hfcl_octree_validate: " + why);
  return rc;
}

int hfcl_octree_from_points(const double* xyz, size_t n, double resolution, uint32_t depth, hfcl_octree_node* nodes_out, size_t capacity,
                            size_t* n_nodes_out) {
  std::vector<hfcl_octree_node> nodes;
  std::string why;
  const int rc = hfcl::oct_from_points(xyz, n, resolution, depth, nodes, &why);
  if (rc) {
    set_error("hfcl_octree_from_points: " + why);
    return rc;
  }
  if (n_nodes_out) *n_nodes_out = nodes.size();
  if (!nodes_out) return HFCL_OK;
  if (capacity < nodes.size()) {
    set_error("hfcl_octree_from_points: " + std::to_string(nodes.size()) + " nodes, room for " + std::to_string(capacity));
    return HFCL_ERR_LIMIT;
  }
  std::copy(nodes.begin(), nodes.end(), nodes_out);
  return HFCL_OK;
}

static bool oct_thresholds_ok(double occupancy_threshold, double free_threshold) {
  return occupancy_threshold == occupancy_threshold && free_threshold == free_threshold;
}

int hfcl_lib_add_octree(hfcl_lib* lib, const hfcl_octree_node* nodes, size_t n_nodes, double resolution, uint32_t depth,
                        double occupancy_threshold, double free_threshold) {
  if (!lib) {
    set_error("hfcl_lib_add_octree: null library");
    return -1;
  }
  std::string why;
  if (hfcl::oct_validate(nodes, n_nodes, depth, &why) != HFCL_OK) {
    set_error("hfcl_lib_add_octree: " + why);
    return -1;
  }
  if (!(resolution > 0.0) || !std::isfinite(resolution) || !oct_thresholds_ok(occupancy_threshold, free_threshold)) {
    set_error("hfcl_lib_add_octree: a resolution that is not positive and finite, or a NaN threshold");
    return -1;
  }
  auto& oc = lib->oct;
  hfcl::DOctree d;
  d.node_off = oc.h_nodes.size();
  d.n_nodes = uint32_t(n_nodes);
  d.depth = depth;
  d.resolution = resolution;
  d.root_half = hfcl::oct_root_half(depth, resolution);
  d.occupancy_threshold = occupancy_threshold;
  d.free_threshold = free_threshold;
  if (n_nodes) oc.h_nodes.insert(oc.h_nodes.end(), nodes, nodes + n_nodes);
  oc.h_trees.push_back(d);
  oc.dirty = true;
  return int(oc.h_trees.size() - 1);
}

int hfcl_lib_octree_set_thresholds(hfcl_lib* lib, int octree, double occupancy_threshold, double free_threshold) {
  if (!lib || octree < 0 || size_t(octree) >= lib->oct.h_trees.size() || !oct_thresholds_ok(occupancy_threshold, free_threshold)) {
    set_error("hfcl_lib_octree_set_thresholds: null library, not an octree of this library, or a NaN threshold");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  lib->oct.h_trees[size_t(octree)].occupancy_threshold = occupancy_threshold;
  lib->oct.h_trees[size_t(octree)].free_threshold = free_threshold;
  lib->oct.dirty = true;
  return HFCL_OK;
}

int hfcl_lib_clear_octrees(hfcl_lib* lib) {
  if (!lib) {
    set_error("hfcl_lib_clear_octrees: null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  lib->oct.h_trees.clear();
  lib->oct.h_nodes.clear();
  lib->oct.dirty = true;
  return HFCL_OK;
}

size_t hfcl_lib_octree_count(const hfcl_lib* lib) { return lib ? lib->oct.h_trees.size() : 0; }

int hfcl_octree_root_box(const hfcl_lib* lib, int octree, double* out6) {
  if (!lib || !out6 || octree < 0 || size_t(octree) >= lib->oct.h_trees.size()) {
    set_error("hfcl_octree_root_box: null argument, or not an octree of this library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  const double d = lib->oct.h_trees[size_t(octree)].root_half;
  for (int k = 0; k < 3; ++k) {
    out6[k] = -d;
    out6[3 + k] = d;
  }
  return HFCL_OK;
}

int hfcl_octree_pair_supported(int32_t t) { return hfcl::oct_kind_supported(t) ? 1 : 0; }

int hfcl_octree_collide_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                     const double* d_tf_shape, size_t n, const uint8_t* d_swapped, const hfcl_collision_request* req,
                                     hfcl_result* d_out, double* d_distance_lower_bound, hfcl_contact* d_contacts, size_t max_contacts_total,
                                     size_t* n_contacts_out, void* stream) {
  return listed_collide_device<OctHost>("hfcl_octree_collide_batch_device", lib, d_octree, d_shape, d_tf_octree, d_tf_shape, n, d_swapped, req, d_out,
                                        d_distance_lower_bound, d_contacts, max_contacts_total, n_contacts_out, (hipStream_t)stream);
}

int hfcl_octree_collide_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_shape, size_t n,
                              const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out, double* distance_lower_bound,
                              hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out) {
  return listed_collide_host<OctHost>("hfcl_octree_collide_batch", lib, octree, shape, tf_octree, tf_shape, n, swapped, req, out, distance_lower_bound,
                                      contacts, max_contacts_total, n_contacts_out);
}

int hfcl_octree_distance_pair_supported(int32_t t) { return hfcl::oct_kind_supported(t) ? 1 : 0; }

int hfcl_octree_distance_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                      const double* d_tf_shape, size_t n, const uint8_t* d_swapped, const hfcl_distance_request* req,
                                      hfcl_result* d_out, uint32_t* d_n_visited, void* stream) {
  return listed_distance_device<OctDist>("hfcl_octree_distance_batch_device", lib, d_octree, d_shape, d_tf_octree, d_tf_shape, n, d_swapped, req, d_out,
                                         d_n_visited, (hipStream_t)stream);
}

int hfcl_octree_distance_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_shape,
                               size_t n, const uint8_t* swapped, const hfcl_distance_request* req, hfcl_result* out, uint32_t* n_visited) {
  return listed_distance_host<OctDist>("hfcl_octree_distance_batch", lib, octree, shape, tf_octree, tf_shape, n, swapped, req, out, n_visited);
}

int hfcl_octree_mesh_pair_supported(int32_t t) { return t == HFCL_BV_OBBRSS ? 1 : 0; }

int hfcl_octree_mesh_collide_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                          const double* d_tf_mesh, size_t n, const uint8_t* d_swapped, const hfcl_collision_request* req,
                                          hfcl_result* d_out, double* d_distance_lower_bound, hfcl_contact* d_contacts, size_t max_contacts_total,
                                          size_t* n_contacts_out, void* stream) {
  return listed_collide_device<OctMeshHost>("hfcl_octree_mesh_collide_batch_device", lib, d_octree, d_shape, d_tf_octree, d_tf_mesh, n, d_swapped, req,
                                            d_out, d_distance_lower_bound, d_contacts, max_contacts_total, n_contacts_out, (hipStream_t)stream);
}

int hfcl_octree_mesh_collide_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_mesh, size_t n,
                                   const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out, double* distance_lower_bound,
                                   hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out) {
  return listed_collide_host<OctMeshHost>("hfcl_octree_mesh_collide_batch", lib, octree, shape, tf_octree, tf_mesh, n, swapped, req, out,
                                          distance_lower_bound, contacts, max_contacts_total, n_contacts_out);
}

int hfcl_octree_mesh_distance_pair_supported(int32_t t) { return t == HFCL_BV_OBBRSS ? 1 : 0; }

int hfcl_octree_mesh_distance_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                           const double* d_tf_mesh, size_t n, const uint8_t* d_swapped, const hfcl_distance_request* req,
                                           hfcl_result* d_out, uint32_t* d_n_visited, void* stream) {
  return listed_distance_device<OctMeshDist>("hfcl_octree_mesh_distance_batch_device", lib, d_octree, d_shape, d_tf_octree, d_tf_mesh, n, d_swapped, req,
                                             d_out, d_n_visited, (hipStream_t)stream);
}

int hfcl_octree_mesh_distance_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_mesh,
                                    size_t n, const uint8_t* swapped, const hfcl_distance_request* req, hfcl_result* out, uint32_t* n_visited) {
  return listed_distance_host<OctMeshDist>("hfcl_octree_mesh_distance_batch", lib, octree, shape, tf_octree, tf_mesh, n, swapped, req, out, n_visited);
}

}  // extern "C"
