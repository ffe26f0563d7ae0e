// hfcl_host_octree.hip -- host side of the octrees (hppfcl_amd_octree.h; the kernels: hfcl_k_octree.hip, the arithmetic:
// hfcl_octree.hpp): the validator and the builder from points, the registration on a library, and hfcl_octree_collide_batch* -- the
// device form in chunks of queries (count, scan, list, solve, fold), the host form a chunked copy / compute / copy around it.  The
// chunking and workspace rules are those of hfcl_host_hfield.hip.  At the end hfcl_octree_distance_batch* (hppfcl_amd_octree_distance.h;
// the kernel: hfcl_k_octree_distance.hip): one launch per chunk, no workspace, no read-back.
#include "hfcl_host.hpp"
#include "hfcl_octree_distance.hpp"

#include <cmath>

namespace {

constexpr size_t OCT_AUTO_CHUNK = 65536;          // queries per chunk when the option is 0
constexpr uint64_t OCT_ITEM_SOFT_CAP = 1u << 20;  // a chunk is cut down (to one query at the least) while it lists more items than this (option octree_items)
// (HF_ITEM_HARD_CAP, hfcl_host.hpp: ... and a single query that lists more is refused)

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

size_t oct_chunk(const hfcl_lib* lib) { return lib->opt.octree_chunk ? lib->opt.octree_chunk : OCT_AUTO_CHUNK; }
uint64_t oct_item_cap(const hfcl_lib* lib) { return lib->opt.octree_items ? lib->opt.octree_items : OCT_ITEM_SOFT_CAP; }

// The call on device pointers: queries [0, n) in chunks; pair0: the index of query 0 in the caller's batch; first: this is the first
// part of that batch (the running contact count starts at 0)
int oct_run(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tft, const double* d_tfs, size_t n,
            const uint8_t* d_swapped, const hfcl_collision_request* req, const QParams<double>& q, bool skip_all, hfcl_result* d_out, double* d_dlb,
            hfcl_contact* d_contacts, size_t contacts_cap, bool want_contacts, uint32_t pair0, bool first, hipStream_t st) {
  auto& oc = lib->oct;
  int rc = upload_octrees(lib);
  if (rc) return rc;
  rc = ensure_local_boxes(lib);
  if (rc) return rc;
  if (!oc.h_words) HIP_TRY(oc.h_words.alloc(2));
  HIP_TRY(oc.d_running.grow(1));
  if (first) HIP_TRY(hipMemsetAsync(oc.d_running, 0, sizeof(uint64_t), st));
  const size_t chunk = std::min(oct_chunk(lib), n);
  HIP_TRY(oc.d_counts.grow(chunk));
  HIP_TRY(oc.d_ccounts.grow(chunk));
  HIP_TRY(oc.d_offsets.grow(chunk + 1));
  HIP_TRY(oc.d_coffsets.grow(chunk + 1));
  HIP_TRY(oc.d_box_total.grow(chunk));
  for (auto& t : lib->timers) t.used = false;
  const bool timed = lib->kernel_timing;
  hipEvent_t e0[OCT_TIMED_KERNELS], e1[OCT_TIMED_KERNELS];
  const char* names[OCT_TIMED_KERNELS];
  if (timed)
    for (int k = 0; k < OCT_TIMED_KERNELS; ++k) {
      KernelTime* t = timer_slot(lib, size_t(k), "");
      e0[k] = t->e0;
      e1[k] = t->e1;
    }
  hfcl::OctArgs a;
  a.shapes = lib->d_shapes64;
  a.verts = lib->d_verts64;
  a.local_boxes = lib->d_local_boxes;
  a.n_shapes = uint32_t(lib->n_shapes);
  a.n_trees = uint32_t(oc.h_trees.size());
  a.trees = oc.d_trees;
  a.nodes = oc.d_nodes;
  a.q = q;
  a.bd2 = req->break_distance * req->break_distance;
  a.num_max_contacts = req->num_max_contacts;
  a.skip_all = skip_all ? 1 : 0;
  a.counts = oc.d_counts;
  a.offsets = oc.d_offsets;
  a.box_total = oc.d_box_total;
  a.ccounts = oc.d_ccounts;
  a.coffsets = oc.d_coffsets;
  a.running = oc.d_running;
  a.contacts = d_contacts;
  a.contacts_cap = d_contacts ? contacts_cap : 0;
  for (size_t q0 = 0; q0 < n;) {  // (every pass takes at least one query)
    size_t m = std::min(chunk, n - q0);
    a.octree = d_octree + q0;
    a.shape = d_shape + q0;
    a.tf_t = d_tft + 12 * q0;
    a.tf_s = d_tfs + 12 * q0;
    a.swapped = d_swapped ? d_swapped + q0 : nullptr;
    a.out = d_out + q0;
    a.dlb = d_dlb ? d_dlb + q0 : nullptr;
    a.pair0 = pair0 + uint32_t(q0);
    a.m = uint32_t(m);
    a.items = oc.d_items;
    a.leaves = oc.d_leaves;
    a.n_items = 0;
    launch_oct_count(st, a);
    // the one read-back of a chunk: its item count (the item workspace is sized by it); a chunk that lists too much is cut at a query
    uint64_t total = 0;
    for (;;) {  // (m at least halves per pass)
      HIP_TRY(hipMemcpyAsync(oc.h_words, oc.d_offsets.get() + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      total = oc.h_words[0];
      if (total <= oct_item_cap(lib) || m == 1) break;
      m = m / 2;
    }
    if (total > HF_ITEM_HARD_CAP) {
      set_error("hfcl_octree_collide_batch: one query lists " + std::to_string(total) + " leaves (limit 2^26)");
      return HFCL_ERR_LIMIT;
    }
    if (total > oc.d_items.capacity()) {
      const size_t want = size_t(total + total / 4 + 1024);
      HIP_TRY(oc.d_items.grow(want));
      HIP_TRY(oc.d_leaves.grow(want));
    }
    a.m = uint32_t(m);
    a.items = oc.d_items;
    a.leaves = oc.d_leaves;
    a.n_items = total;
    launch_oct_solve(st, a, lib->n_cus * 16, want_contacts, names, timed ? e0 : nullptr, timed ? e1 : nullptr);
    if (timed)
      for (int k = 0; k < OCT_TIMED_KERNELS; ++k) lib->timers[size_t(k)].name = names[k];
    q0 += m;
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

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
  if (int rc = hf_no_device()) return rc;
  if (!lib || !req) {
    set_error("hfcl_octree_collide_batch_device: null library / request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  bool skip_all = false;
  if (int rc = oct_request("hfcl_octree_collide_batch_device", req, q, skip_all)) return rc;
  if (n_contacts_out) *n_contacts_out = 0;
  if (n == 0) return HFCL_OK;
  if (!d_octree || !d_shape || !d_tf_octree || !d_tf_shape || !d_out) {
    set_error("hfcl_octree_collide_batch_device: null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 queries per call)");
    return HFCL_ERR_LIMIT;
  }
  HIP_TRY(hipSetDevice(lib->device));
  hipStream_t st = (hipStream_t)stream;
  const bool want_contacts = d_contacts || n_contacts_out;
  const int rc = oct_run(lib, d_octree, d_shape, d_tf_octree, d_tf_shape, n, d_swapped, req, q, skip_all, d_out, d_distance_lower_bound, d_contacts,
                         max_contacts_total, want_contacts, 0u, true, st);
  if (rc) return rc;
  if (n_contacts_out) {
    HIP_TRY(hipMemcpyAsync(lib->oct.h_words.get() + 1, lib->oct.d_running, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_contacts_out = size_t(lib->oct.h_words[1]);
  }
  return HFCL_OK;
}

int hfcl_octree_collide_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_shape, size_t n,
                              const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out, double* distance_lower_bound,
                              hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out) {
  if (int rc = hf_no_device()) return rc;
  if (!lib || !req) {
    set_error("hfcl_octree_collide_batch: null library / request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  bool skip_all = false;
  if (int rc = oct_request("hfcl_octree_collide_batch", req, q, skip_all)) return rc;
  if (n_contacts_out) *n_contacts_out = 0;
  if (n == 0) return HFCL_OK;
  if (!octree || !shape || !tf_octree || !tf_shape || !out) {
    set_error("hfcl_octree_collide_batch: null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 queries per call)");
    return HFCL_ERR_LIMIT;
  }
  auto& oc = lib->oct;
  for (size_t i = 0; i < n; ++i) {
    if (octree[i] >= oc.h_trees.size() || shape[i] >= lib->n_shapes) {
      set_error("hfcl_octree_collide_batch: octree / shape id outside the library at query " + std::to_string(i));
      return HFCL_ERR_INVALID_ARGUMENT;
    }
    if (!hfcl_octree_pair_supported(lib->h_shapes[shape[i]].type)) {
      set_error("Collision function between an octree and node type " + std::to_string(lib->h_shapes[shape[i]].type) + " is not yet supported.");
      return HFCL_ERR_UNSUPPORTED_PAIR;
    }
  }
  HIP_TRY(hipSetDevice(lib->device));
  if (!oc.st) HIP_TRY(oc.st.create());
  hipStream_t st = oc.st;
  const size_t chunk = std::min(oct_chunk(lib), n);
  const bool want_contacts = contacts || n_contacts_out;
  // the contact list of the whole call stays on the device until the last chunk has run: at most what the queries can produce
  // (a query adds at most num_max_contacts contacts, and no more than the 2^26 leaves it may list)
  const size_t ccap = contacts ? std::min(max_contacts_total, n * size_t(std::min<uint64_t>(req->num_max_contacts, HF_ITEM_HARD_CAP))) : 0;
  HIP_TRY(oc.s_octree.grow(chunk));
  HIP_TRY(oc.s_shape.grow(chunk));
  HIP_TRY(oc.s_tft.grow(12 * chunk));
  HIP_TRY(oc.s_tfs.grow(12 * chunk));
  HIP_TRY(oc.s_swapped.grow(chunk));
  HIP_TRY(oc.s_out.grow(chunk));
  HIP_TRY(oc.s_dlb.grow(chunk));
  if (ccap) HIP_TRY(oc.s_contacts.grow(ccap));
  int rc = HFCL_OK;
  for (size_t q0 = 0; q0 < n && !rc; q0 += chunk) {
    const size_t m = std::min(chunk, n - q0);
    bool ok = hipMemcpyAsync(oc.s_octree, octree + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(oc.s_shape, shape + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(oc.s_tft, tf_octree + 12 * q0, m * 12 * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(oc.s_tfs, tf_shape + 12 * q0, m * 12 * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && (!swapped || hipMemcpyAsync(oc.s_swapped, swapped + q0, m, hipMemcpyHostToDevice, st) == hipSuccess);
    if (!ok) {
      set_error("hfcl_octree_collide_batch: HIP copy failed");
      rc = HFCL_ERR_HIP;
      break;
    }
    rc = oct_run(lib, oc.s_octree, oc.s_shape, oc.s_tft, oc.s_tfs, m, swapped ? oc.s_swapped.get() : nullptr, req, q, skip_all, oc.s_out,
                 distance_lower_bound ? oc.s_dlb.get() : nullptr, ccap ? oc.s_contacts.get() : nullptr, ccap, want_contacts, uint32_t(q0), q0 == 0, st);
    if (rc) break;
    ok = hipMemcpyAsync(out + q0, oc.s_out, m * sizeof(hfcl_result), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && (!distance_lower_bound || hipMemcpyAsync(distance_lower_bound + q0, oc.s_dlb, m * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess);
    ok = ok && hipStreamSynchronize(st) == hipSuccess;  // (the staging buffers are the next chunk's)
    if (!ok) {
      set_error("hfcl_octree_collide_batch: HIP copy failed");
      rc = HFCL_ERR_HIP;
    }
  }
  if (!rc && want_contacts) {
    bool ok = hipMemcpyAsync(oc.h_words.get() + 1, oc.d_running, sizeof(uint64_t), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if (ok) {
      const size_t total = size_t(oc.h_words[1]);
      if (n_contacts_out) *n_contacts_out = total;
      const size_t stored = std::min(total, ccap);
      if (stored) ok = hipMemcpy(contacts, oc.s_contacts, stored * sizeof(hfcl_contact), hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) {
      set_error("hfcl_octree_collide_batch: HIP copy failed");
      rc = HFCL_ERR_HIP;
    }
  }
  hipStreamSynchronize(st);
  return rc;
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
  if (int rc = hf_no_device()) return rc;
  if (!lib) {
    set_error("hfcl_octree_distance_batch_device: null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  if (int rc = octd_request("hfcl_octree_distance_batch_device", req, q)) return rc;
  if (n == 0) return HFCL_OK;
  if (!d_octree || !d_shape || !d_tf_octree || !d_tf_shape || !d_out) {
    set_error("hfcl_octree_distance_batch_device: null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 queries per call)");
    return HFCL_ERR_LIMIT;
  }
  HIP_TRY(hipSetDevice(lib->device));
  return octd_run(lib, d_octree, d_shape, d_tf_octree, d_tf_shape, n, d_swapped, q, d_out, d_n_visited, (hipStream_t)stream);
}

int hfcl_octree_distance_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_shape,
                               size_t n, const uint8_t* swapped, const hfcl_distance_request* req, hfcl_result* out, uint32_t* n_visited) {
  if (int rc = hf_no_device()) return rc;
  if (!lib) {
    set_error("hfcl_octree_distance_batch: null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  if (int rc = octd_request("hfcl_octree_distance_batch", req, q)) return rc;
  if (n == 0) return HFCL_OK;
  if (!octree || !shape || !tf_octree || !tf_shape || !out) {
    set_error("hfcl_octree_distance_batch: null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 queries per call)");
    return HFCL_ERR_LIMIT;
  }
  auto& oc = lib->oct;
  for (size_t i = 0; i < n; ++i) {
    if (octree[i] >= oc.h_trees.size() || shape[i] >= lib->n_shapes) {
      set_error("hfcl_octree_distance_batch: octree / shape id outside the library at query " + std::to_string(i));
      return HFCL_ERR_INVALID_ARGUMENT;
    }
    if (!hfcl_octree_distance_pair_supported(lib->h_shapes[shape[i]].type)) {
      set_error("Distance function between an octree and node type " + std::to_string(lib->h_shapes[shape[i]].type) + " is not yet supported.");
      return HFCL_ERR_UNSUPPORTED_PAIR;
    }
  }
  HIP_TRY(hipSetDevice(lib->device));
  if (!oc.st) HIP_TRY(oc.st.create());
  hipStream_t st = oc.st;
  // staged in pieces of the chunk option: the staging buffers are the collide call's, the visited counts go through its count buffer
  const size_t chunk = std::min(oct_chunk(lib), n);
  HIP_TRY(oc.s_octree.grow(chunk));
  HIP_TRY(oc.s_shape.grow(chunk));
  HIP_TRY(oc.s_tft.grow(12 * chunk));
  HIP_TRY(oc.s_tfs.grow(12 * chunk));
  HIP_TRY(oc.s_swapped.grow(chunk));
  HIP_TRY(oc.s_out.grow(chunk));
  HIP_TRY(oc.d_counts.grow(chunk));
  int rc = HFCL_OK;
  for (size_t q0 = 0; q0 < n && !rc; q0 += chunk) {
    const size_t m = std::min(chunk, n - q0);
    bool ok = hipMemcpyAsync(oc.s_octree, octree + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(oc.s_shape, shape + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(oc.s_tft, tf_octree + 12 * q0, m * 12 * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(oc.s_tfs, tf_shape + 12 * q0, m * 12 * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && (!swapped || hipMemcpyAsync(oc.s_swapped, swapped + q0, m, hipMemcpyHostToDevice, st) == hipSuccess);
    if (!ok) {
      set_error("hfcl_octree_distance_batch: HIP copy failed");
      rc = HFCL_ERR_HIP;
      break;
    }
    rc = octd_run(lib, oc.s_octree, oc.s_shape, oc.s_tft, oc.s_tfs, m, swapped ? oc.s_swapped.get() : nullptr, q, oc.s_out,
                  n_visited ? oc.d_counts.get() : nullptr, st);
    if (rc) break;
    ok = hipMemcpyAsync(out + q0, oc.s_out, m * sizeof(hfcl_result), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && (!n_visited || hipMemcpyAsync(n_visited + q0, oc.d_counts, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess);
    ok = ok && hipStreamSynchronize(st) == hipSuccess;  // (the staging buffers are the next chunk's)
    if (!ok) {
      set_error("hfcl_octree_distance_batch: HIP copy failed");
      rc = HFCL_ERR_HIP;
    }
  }
  hipStreamSynchronize(st);
  return rc;
}

}  // extern "C"
