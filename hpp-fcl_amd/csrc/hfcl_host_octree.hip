// hfcl_host_octree.hip -- host side of the octrees (hppfcl_amd_octree.h; the kernels: hfcl_k_octree.hip, the arithmetic:
// hfcl_octree.hpp): the validator and the builder from points, the registration on a library, the upload of the tables, the request
// checks, and hfcl_octree_collide_batch* -- the entry points and the chunk driver of the listed-leaf pipeline (hfcl_host_listed.hpp)
// for OctHost, the kind defined here.  At the end hfcl_octree_distance_batch* (hppfcl_amd_octree_distance.h; the kernel:
// hfcl_k_octree_distance.hip): one launch per chunk, no workspace, no read-back; its host form is staged as the collide call's.
// Last hfcl_octree_mesh_collide_batch* (hppfcl_amd_octree_mesh.h; the kernels: hfcl_k_octree_mesh.hip): the same driver for OctMeshHost, on a
// workspace of its own, behind a check of the meshes' BVH depths.  And hfcl_octree_mesh_distance_batch* (hppfcl_amd_octree_mesh_distance.h; the
// kernel: hfcl_k_octree_mesh_distance.hip): the request check of the octree distance() call, the mesh checks of the mesh collide() call, one
// launch per chunk.
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

size_t oct_chunk(const hfcl_lib* lib) { return lib->opt.octree_chunk ? lib->opt.octree_chunk : LISTED_AUTO_CHUNK; }

struct OctHost {
  using Args = hfcl::OctArgs;
  static constexpr const char* limit_who = "hfcl_octree_collide_batch";
  static constexpr const char* noun = "octree";
  static constexpr const char* a_noun = "an octree";
  static auto& ws(hfcl_lib* lib) { return lib->oct.ws; }
  static size_t n_containers(const hfcl_lib* lib) { return lib->oct.h_trees.size(); }
  static int upload(hfcl_lib* lib) {
    const int rc = upload_octrees(lib);
    return rc ? rc : ensure_local_boxes(lib);
  }
  static void fill(hfcl_lib* lib, Args& a) {
    a.local_boxes = lib->d_local_boxes;
    a.n_trees = uint32_t(lib->oct.h_trees.size());
    a.trees = lib->oct.d_trees;
    a.nodes = lib->oct.d_nodes;
  }
  static void ids(Args& a, const uint32_t* p) { a.octree = p; }
  static constexpr auto chunk = oct_chunk;
  static uint64_t item_cap(const hfcl_lib* lib) { return lib->opt.octree_items ? lib->opt.octree_items : LISTED_ITEM_SOFT_CAP; }
  static constexpr auto request = oct_request;
  static constexpr auto supported = hfcl_octree_pair_supported;
  static constexpr auto count = launch_oct_count;
  static constexpr auto solve = launch_oct_solve;
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

// ---- distance() (hppfcl_amd_octree_distance.h) ------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// what both forms check before any work
int octd_request(const char* who, const hfcl_distance_request* req, QParams<double>& q) {
  const int rc = setup_distance<double>(req, q);  // a null request, tolerances, epa_max_iterations > 64, variants
  if (rc) return rc;
  if (req->q.gjk_initial_guess != HFCL_GUESS_DEFAULT) {
    set_error(std::string(who) + ": gjk_initial_guess must be DefaultGuess (a cached guess chains from leaf to leaf inside a query, a bounding-volume guess changes the leaf set-up: not done)");
    return HFCL_ERR_LIMIT;
  }
  return HFCL_OK;
}

// one entry of last_kernel_breakdown() around the launches of a call
struct Timed {
  hfcl_lib* lib = nullptr;
  hipStream_t st;
  Timed(hfcl_lib* l, const char* name, hipStream_t s) : st(s) {
    for (auto& t : l->timers) t.used = false;
    if (!l->kernel_timing) return;
    lib = l;
    (void)hipEventRecord(timer_slot(lib, 0, name)->e0, st);
  }
  ~Timed() {
    if (lib) (void)hipEventRecord(lib->timers[0].e1, st);
  }
  Timed(const Timed&) = delete;
};

// The call on device pointers: queries [0, n) in chunks, one launch each; nothing is read back
int octd_run(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tft, const double* d_tfs, size_t n,
             const uint8_t* d_swapped, const QParams<double>& q, hfcl_result* d_out, uint32_t* d_visited, hipStream_t st) {
  auto& oc = lib->oct;
  const int rc = upload_octrees(lib);
  if (rc) return rc;
  hfcl::OctDistArgs a;
  a.shapes = lib->d_shapes64;
  a.verts = lib->d_verts64;
  a.n_shapes = uint32_t(lib->n_shapes);
  a.n_trees = uint32_t(oc.h_trees.size());
  a.trees = oc.d_trees;
  a.nodes = oc.d_nodes;
  a.q = q;
  const size_t chunk = std::min(oct_chunk(lib), n);
  Timed t(lib, "k_oct_distance", st);
  for (size_t q0 = 0; q0 < n; q0 += chunk) {
    const size_t m = std::min(chunk, n - q0);
    a.octree = d_octree + q0;
    a.shape = d_shape + q0;
    a.tf_t = d_tft + 12 * q0;
    a.tf_s = d_tfs + 12 * q0;
    a.swapped = d_swapped ? d_swapped + q0 : nullptr;
    a.out = d_out + q0;
    a.n_visited = d_visited ? d_visited + q0 : nullptr;
    a.m = uint32_t(m);
    launch_oct_distance(st, a, 1 << 20);  // (a workgroup per four queries: the hardware hands the long walks out as they come)
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

}  // namespace

extern "C" {

int hfcl_octree_distance_pair_supported(int32_t t) { return hfcl::oct_kind_supported(t) ? 1 : 0; }

int hfcl_octree_distance_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                      const double* d_tf_shape, size_t n, const uint8_t* d_swapped, const hfcl_distance_request* req,
                                      hfcl_result* d_out, uint32_t* d_n_visited, void* stream) {
  if (int rc = no_device()) return rc;
  if (!lib) {
    set_error("hfcl_octree_distance_batch_device: null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  if (int rc = octd_request("hfcl_octree_distance_batch_device", req, q)) return rc;
  if (n == 0) return HFCL_OK;
  if (int rc = listed_check_arrays("hfcl_octree_distance_batch_device", d_octree, d_shape, d_tf_octree, d_tf_shape, d_out, n)) return rc;
  HIP_TRY(hipSetDevice(lib->device));
  return octd_run(lib, d_octree, d_shape, d_tf_octree, d_tf_shape, n, d_swapped, q, d_out, d_n_visited, (hipStream_t)stream);
}

int hfcl_octree_distance_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_shape,
                               size_t n, const uint8_t* swapped, const hfcl_distance_request* req, hfcl_result* out, uint32_t* n_visited) {
  const char* who = "hfcl_octree_distance_batch";
  if (int rc = no_device()) return rc;
  if (!lib) {
    set_error("hfcl_octree_distance_batch: null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  if (int rc = octd_request(who, req, q)) return rc;
  if (n == 0) return HFCL_OK;
  if (int rc = listed_check_arrays(who, octree, shape, tf_octree, tf_shape, out, n)) return rc;
  if (int rc = listed_check_queries(who, lib, octree, lib->oct.h_trees.size(), shape, n, OctHost::noun, OctHost::a_noun, "Distance",
                                    hfcl_octree_distance_pair_supported))
    return rc;
  HIP_TRY(hipSetDevice(lib->device));
  auto& w = lib->oct.ws;
  if (!w.st) HIP_TRY(w.st.create());
  // staged in pieces of the chunk option: the staging buffers are the collide call's, the visited counts go through its count buffer
  const size_t chunk = std::min(oct_chunk(lib), n);
  HIP_TRY(w.d_counts.grow(chunk));
  const int rc = listed_staged(who, w, chunk, octree, shape, tf_octree, tf_shape, n, swapped, out, n_visited, w.d_counts.get(), [&](size_t, size_t m) {
    return octd_run(lib, w.s_id, w.s_shape, w.s_tf_a, w.s_tf_s, m, swapped ? w.s_swapped.get() : nullptr, q, w.s_out,
                    n_visited ? w.d_counts.get() : nullptr, w.st);
  });
  hipStreamSynchronize(w.st);
  return rc;
}

}  // extern "C"

// ---- collide() against meshes (hppfcl_amd_octree_mesh.h; the kernels: hfcl_k_octree_mesh.hip) ---------------------------------------
namespace {

// the levels of every registered mesh's BVH, computed once per mesh
void octm_depths(hfcl_lib* lib) {
  auto& depth = lib->oct.mesh_depth;
  for (size_t k = depth.size(); k < lib->h_meshes.size(); ++k) {
    const hfcl_bvh_node* nodes = lib->h_bvh_nodes.data() + lib->h_meshes[k].node_off;
    depth.push_back(hfcl::octm_bvh_depth(lib->h_meshes[k].n_nodes, [&](uint32_t i) { return nodes[i].first_child; }));
  }
}
int octm_too_deep(const char* who, size_t mesh, uint32_t depth) {
  set_error(std::string(who) + ": the BVH of mesh " + std::to_string(mesh) + " has " + (depth == 0xFFFFFFFFu ? std::string("unbounded") : std::to_string(depth)) +
            " levels (limit " + std::to_string(HFCL_OCTREE_MESH_MAX_BVH_DEPTH) + ")");
  return HFCL_ERR_LIMIT;
}

struct OctMeshHost {
  using Args = hfcl::OctMeshArgs;
  static constexpr const char* limit_who = "hfcl_octree_mesh_collide_batch";
  static constexpr const char* noun = "octree";
  static constexpr const char* a_noun = "an octree";
  static auto& ws(hfcl_lib* lib) { return lib->oct.ws_mesh; }
  static size_t n_containers(const hfcl_lib* lib) { return lib->oct.h_trees.size(); }
  static int upload(hfcl_lib* lib) {
    const int rc = upload_octrees(lib);
    return rc ? rc : upload_bvh(lib);
  }
  static void fill(hfcl_lib* lib, Args& a) {
    a.n_trees = uint32_t(lib->oct.h_trees.size());
    a.trees = lib->oct.d_trees;
    a.nodes = lib->oct.d_nodes;
    a.n_meshes = uint32_t(lib->h_meshes.size());
    a.mnodes = lib->d_nodes64;
    a.mverts = lib->d_bverts64;
    a.mtris = lib->d_btris;
    a.meshes = lib->d_meshes;
  }
  static void ids(Args& a, const uint32_t* p) { a.octree = p; }
  static constexpr auto chunk = oct_chunk;
  static uint64_t item_cap(const hfcl_lib* lib) { return lib->opt.octree_items ? lib->opt.octree_items : LISTED_ITEM_SOFT_CAP; }
  static constexpr auto request = oct_request;
  static constexpr auto supported = hfcl_octree_mesh_pair_supported;
  static constexpr auto count = launch_octm_count;
  static constexpr auto solve = launch_octm_solve;
};

}  // namespace

extern "C" {

int hfcl_octree_mesh_pair_supported(int32_t t) { return t == HFCL_BV_OBBRSS ? 1 : 0; }

int hfcl_octree_mesh_collide_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                          const double* d_tf_mesh, size_t n, const uint8_t* d_swapped, const hfcl_collision_request* req,
                                          hfcl_result* d_out, double* d_distance_lower_bound, hfcl_contact* d_contacts, size_t max_contacts_total,
                                          size_t* n_contacts_out, void* stream) {
  const char* who = "hfcl_octree_mesh_collide_batch_device";
  if (lib && req && n && no_device() == HFCL_OK) {  // the ids are not visible here: no registered mesh may be deeper than the walk's stack
    QParams<double> q;
    bool skip_all = false;
    if (int rc = oct_request(who, req, q, skip_all)) return rc;
    octm_depths(lib);
    for (size_t k = 0; k < lib->oct.mesh_depth.size(); ++k)
      if (lib->oct.mesh_depth[k] > HFCL_OCTREE_MESH_MAX_BVH_DEPTH) return octm_too_deep(who, k, lib->oct.mesh_depth[k]);
  }
  return listed_collide_device<OctMeshHost>(who, lib, d_octree, d_shape, d_tf_octree, d_tf_mesh, n, d_swapped, req, d_out, d_distance_lower_bound,
                                            d_contacts, max_contacts_total, n_contacts_out, (hipStream_t)stream);
}

int hfcl_octree_mesh_collide_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_mesh, size_t n,
                                   const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out, double* distance_lower_bound,
                                   hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out) {
  const char* who = "hfcl_octree_mesh_collide_batch";
  if (lib && req && n && shape && no_device() == HFCL_OK) {  // a mesh named by the batch that is deeper than the walk's stack: nothing is written
    QParams<double> q;
    bool skip_all = false;
    if (int rc = oct_request(who, req, q, skip_all)) return rc;
    octm_depths(lib);
    for (size_t i = 0; i < n; ++i) {
      if (shape[i] >= lib->n_shapes || lib->h_shapes[shape[i]].type != HFCL_BV_OBBRSS) continue;  // (refused below, in the order of every host form)
      const size_t k = lib->h_shapes[shape[i]].bvh_index;
      if (k < lib->oct.mesh_depth.size() && lib->oct.mesh_depth[k] > HFCL_OCTREE_MESH_MAX_BVH_DEPTH) return octm_too_deep(who, k, lib->oct.mesh_depth[k]);
    }
  }
  if (lib && shape && n && no_device() == HFCL_OK)  // a mesh row that names no registered mesh
    for (size_t i = 0; i < n; ++i)
      if (shape[i] < lib->n_shapes && lib->h_shapes[shape[i]].type == HFCL_BV_OBBRSS && size_t(lib->h_shapes[shape[i]].bvh_index) >= lib->h_meshes.size()) {
        set_error(std::string(who) + ": bvh_index outside the registered meshes at query " + std::to_string(i));
        return HFCL_ERR_INVALID_ARGUMENT;
      }
  return listed_collide_host<OctMeshHost>(who, lib, octree, shape, tf_octree, tf_mesh, n, swapped, req, out, distance_lower_bound, contacts,
                                          max_contacts_total, n_contacts_out);
}

}  // extern "C"

// ---- distance() against meshes (hppfcl_amd_octree_mesh_distance.h; the kernel: hfcl_k_octree_mesh_distance.hip) ---------------------
namespace {

// The call on device pointers: queries [0, n) in chunks, one launch each; nothing is read back
int octmd_run(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tft, const double* d_tfm, size_t n,
              const uint8_t* d_swapped, const QParams<double>& q, hfcl_result* d_out, uint32_t* d_visited, hipStream_t st) {
  auto& oc = lib->oct;
  if (int rc = upload_octrees(lib)) return rc;
  if (int rc = upload_bvh(lib)) return rc;
  hfcl::OctMeshDistArgs a;
  a.shapes = lib->d_shapes64;
  a.n_shapes = uint32_t(lib->n_shapes);
  a.n_trees = uint32_t(oc.h_trees.size());
  a.n_meshes = uint32_t(lib->h_meshes.size());
  a.trees = oc.d_trees;
  a.nodes = oc.d_nodes;
  a.mnodes = lib->d_nodes64;
  a.mverts = lib->d_bverts64;
  a.mtris = lib->d_btris;
  a.meshes = lib->d_meshes;
  a.q = q;
  const size_t chunk = std::min(oct_chunk(lib), n);
  Timed t(lib, "k_octm_distance", st);
  for (size_t q0 = 0; q0 < n; q0 += chunk) {
    const size_t m = std::min(chunk, n - q0);
    a.octree = d_octree + q0;
    a.shape = d_shape + q0;
    a.tf_t = d_tft + 12 * q0;
    a.tf_m = d_tfm + 12 * q0;
    a.swapped = d_swapped ? d_swapped + q0 : nullptr;
    a.out = d_out + q0;
    a.n_visited = d_visited ? d_visited + q0 : nullptr;
    a.m = uint32_t(m);
    launch_octm_distance(st, a, 1 << 20);  // (a workgroup per four queries: the hardware hands the long walks out as they come)
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

}  // namespace

extern "C" {

int hfcl_octree_mesh_distance_pair_supported(int32_t t) { return t == HFCL_BV_OBBRSS ? 1 : 0; }

int hfcl_octree_mesh_distance_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                           const double* d_tf_mesh, size_t n, const uint8_t* d_swapped, const hfcl_distance_request* req,
                                           hfcl_result* d_out, uint32_t* d_n_visited, void* stream) {
  const char* who = "hfcl_octree_mesh_distance_batch_device";
  if (int rc = no_device()) return rc;
  if (!lib) {
    set_error(std::string(who) + ": null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  if (int rc = octd_request(who, req, q)) return rc;
  if (n == 0) return HFCL_OK;
  if (int rc = listed_check_arrays(who, d_octree, d_shape, d_tf_octree, d_tf_mesh, d_out, n)) return rc;
  octm_depths(lib);  // the ids are not visible here: no registered mesh may be deeper than the walk's stack
  for (size_t k = 0; k < lib->oct.mesh_depth.size(); ++k)
    if (lib->oct.mesh_depth[k] > HFCL_OCTREE_MESH_MAX_BVH_DEPTH) return octm_too_deep(who, k, lib->oct.mesh_depth[k]);
  HIP_TRY(hipSetDevice(lib->device));
  return octmd_run(lib, d_octree, d_shape, d_tf_octree, d_tf_mesh, n, d_swapped, q, d_out, d_n_visited, (hipStream_t)stream);
}

int hfcl_octree_mesh_distance_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_mesh,
                                    size_t n, const uint8_t* swapped, const hfcl_distance_request* req, hfcl_result* out, uint32_t* n_visited) {
  const char* who = "hfcl_octree_mesh_distance_batch";
  if (int rc = no_device()) return rc;
  if (!lib) {
    set_error(std::string(who) + ": null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  if (int rc = octd_request(who, req, q)) return rc;
  if (n == 0) return HFCL_OK;
  if (int rc = listed_check_arrays(who, octree, shape, tf_octree, tf_mesh, out, n)) return rc;
  octm_depths(lib);
  for (size_t i = 0; i < n; ++i) {  // a mesh named by the batch that is deeper than the walk's stack, or a mesh row that names no registered mesh
    if (shape[i] >= lib->n_shapes || lib->h_shapes[shape[i]].type != HFCL_BV_OBBRSS) continue;  // (refused below, in the order of every host form)
    const size_t k = lib->h_shapes[shape[i]].bvh_index;
    if (k < lib->oct.mesh_depth.size() && lib->oct.mesh_depth[k] > HFCL_OCTREE_MESH_MAX_BVH_DEPTH) return octm_too_deep(who, k, lib->oct.mesh_depth[k]);
  }
  for (size_t i = 0; i < n; ++i)
    if (shape[i] < lib->n_shapes && lib->h_shapes[shape[i]].type == HFCL_BV_OBBRSS && size_t(lib->h_shapes[shape[i]].bvh_index) >= lib->h_meshes.size()) {
      set_error(std::string(who) + ": bvh_index outside the registered meshes at query " + std::to_string(i));
      return HFCL_ERR_INVALID_ARGUMENT;
    }
  if (int rc = listed_check_queries(who, lib, octree, lib->oct.h_trees.size(), shape, n, OctHost::noun, OctHost::a_noun, "Distance",
                                    hfcl_octree_mesh_distance_pair_supported))
    return rc;
  HIP_TRY(hipSetDevice(lib->device));
  auto& w = lib->oct.ws_mesh;
  if (!w.st) HIP_TRY(w.st.create());
  // staged in pieces of the chunk option: the staging buffers are the mesh collide call's, the visited counts go through its count buffer
  const size_t chunk = std::min(oct_chunk(lib), n);
  HIP_TRY(w.d_counts.grow(chunk));
  const int rc = listed_staged(who, w, chunk, octree, shape, tf_octree, tf_mesh, n, swapped, out, n_visited, w.d_counts.get(), [&](size_t, size_t m) {
    return octmd_run(lib, w.s_id, w.s_shape, w.s_tf_a, w.s_tf_s, m, swapped ? w.s_swapped.get() : nullptr, q, w.s_out,
                     n_visited ? w.d_counts.get() : nullptr, w.st);
  });
  hipStreamSynchronize(w.st);
  return rc;
}

}  // extern "C"
