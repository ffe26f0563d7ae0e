// hfcl_host_hfield.hip -- host side of the height fields (hppfcl_amd_hfield.h; the kernels: hfcl_k_hfield.hip, the arithmetic:
// hfcl_hfield.hpp): the tree builder, the registration on a library, and hfcl_hfield_collide_batch* -- the device form in chunks of
// queries (count, scan, list, solve, fold), the host form a chunked copy / compute / copy around it.
#include "hfcl_host.hpp"

#include <cmath>

namespace {

constexpr size_t HF_AUTO_CHUNK = 65536;         // queries per chunk when the option is 0
constexpr uint64_t HF_ITEM_SOFT_CAP = 1u << 20;  // a chunk is cut down (to one query at the least) while it lists more items than this (option hfield_items)
// (HF_ITEM_HARD_CAP, hfcl_host.hpp: ... and a single query that lists more is refused)

int hf_build(double x_dim, double y_dim, const double* heights, size_t ny, size_t nx, double min_height, hfcl_hfield_node* nodes_out,
             size_t* n_nodes_out, double* xg_out, double* yg_out, std::vector<double>* clamped_out) {
  if (!heights || nx < 2 || ny < 2) {
    set_error("hfcl_hfield_build: null heights, or fewer than 2 samples along a side");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (nx > HFCL_HFIELD_MAX_SIDE || ny > HFCL_HFIELD_MAX_SIDE) {
    set_error("hfcl_hfield_build: a side above 32768 samples");
    return HFCL_ERR_LIMIT;
  }
  if (!std::isfinite(x_dim) || !std::isfinite(y_dim) || !std::isfinite(min_height)) {
    set_error("hfcl_hfield_build: non-finite dimension or min_height");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  std::vector<double> h(nx * ny);
  for (size_t i = 0; i < nx * ny; ++i) {
    if (!std::isfinite(heights[i])) {
      set_error("hfcl_hfield_build: non-finite height at sample " + std::to_string(i));
      return HFCL_ERR_INVALID_ARGUMENT;
    }
    h[i] = std::max(heights[i], min_height);  // heights.cwiseMax(min_height)
  }
  for (size_t y = 0; y + 1 < ny; ++y)
    for (size_t x = 0; x + 1 < nx; ++x) {
      const double* c = h.data() + y * nx + x;
      if (c[0] == min_height && c[1] == min_height && c[nx] == min_height && c[nx + 1] == min_height) {
        set_error("hfcl_hfield_build: the four heights of cell (" + std::to_string(y) + ", " + std::to_string(x) +
                  ") all equal min_height (the reference asserts max_height > min_height)");
        return HFCL_ERR_INVALID_ARGUMENT;
      }
    }
  const size_t n_nodes = 2 * (nx - 1) * (ny - 1) - 1;
  if (n_nodes_out) *n_nodes_out = n_nodes;
  std::vector<double> xg(nx), yg(ny);
  for (size_t i = 0; i < nx; ++i) xg[i] = hfcl::hf_linspaced(i, nx, -0.5 * x_dim, 0.5 * x_dim);
  for (size_t i = 0; i < ny; ++i) yg[i] = hfcl::hf_linspaced(i, ny, 0.5 * y_dim, -0.5 * y_dim);
  if (xg_out) std::copy(xg.begin(), xg.end(), xg_out);
  if (yg_out) std::copy(yg.begin(), yg.end(), yg_out);
  if (nodes_out) {
    hfcl::HfBuilder b;
    b.h = h.data();
    b.nx = nx;
    b.min_height = min_height;
    b.xg = xg.data();
    b.yg = yg.data();
    b.nodes = nodes_out;
    b.num = 1;
    b.ncols = nx;
    b.nrows = ny;
    b.rec(0, 0, int(nx - 1), 0, int(ny - 1));
    if (size_t(b.num) != n_nodes) {
      set_error("hfcl_hfield_build: internal error (node count)");
      return HFCL_ERR_INVALID_ARGUMENT;
    }
  }
  if (clamped_out) clamped_out->swap(h);
  return HFCL_OK;
}

int upload_hfields(hfcl_lib* lib) {
  auto& hf = lib->hf;
  if (!hf.dirty) return HFCL_OK;
  HIP_TRY(hipDeviceSynchronize());  // nothing of this library may still be reading the old tables
  if (hf.h_fields.empty()) {        // (hfcl_lib_clear_hfields: the device buffers stay for the next registration)
    hf.dirty = false;
    return HFCL_OK;
  }
  HIP_TRY(hf.d_fields.grow(hf.h_fields.size()));
  HIP_TRY(hf.d_nodes.grow(hf.h_nodes.size()));
  HIP_TRY(hf.d_heights.grow(hf.h_heights.size()));
  HIP_TRY(hf.d_xgrid.grow(hf.h_xgrid.size()));
  HIP_TRY(hf.d_ygrid.grow(hf.h_ygrid.size()));
  HIP_TRY(hipMemcpy(hf.d_fields, hf.h_fields.data(), hf.h_fields.size() * sizeof(hfcl::DHfield), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(hf.d_nodes, hf.h_nodes.data(), hf.h_nodes.size() * sizeof(hfcl_hfield_node), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(hf.d_heights, hf.h_heights.data(), hf.h_heights.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(hf.d_xgrid, hf.h_xgrid.data(), hf.h_xgrid.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(hf.d_ygrid, hf.h_ygrid.data(), hf.h_ygrid.size() * sizeof(double), hipMemcpyHostToDevice));
  hf.dirty = false;
  return HFCL_OK;
}

}  // namespace

// (hf_request, hf_chunk, hf_run, hf_no_device: declared in hfcl_host.hpp -- the scene unit's terrain calls run their chunks through them)
// what every form checks before any work
int hf_request(const char* who, const hfcl_collision_request* req, QParams<double>& q, bool& skip_all) {
  const int rc = setup_collide<double>(req, q, skip_all);  // num_max_contacts == 0, epa_max_iterations > 64, tolerances, variants
  if (rc) return rc;
  if (req->q.gjk_initial_guess != HFCL_GUESS_DEFAULT) {
    set_error(std::string(who) + ": gjk_initial_guess must be DefaultGuess (a cached guess chains from leaf to leaf inside a query: not done)");
    return HFCL_ERR_LIMIT;
  }
  if (req->distance_upper_bound != Lim<double>::max()) {
    set_error(std::string(who) + ": distance_upper_bound must be its default (a finite bound turns leaf distances into early-stopped bounds: not done)");
    return HFCL_ERR_LIMIT;
  }
  q = hfcl::hf_leaf_params(q);
  q.gjk.distance_upper_bound = Lim<double>::max();
  return HFCL_OK;
}

size_t hf_chunk(const hfcl_lib* lib) { return lib->opt.hfield_chunk ? lib->opt.hfield_chunk : HF_AUTO_CHUNK; }
static uint64_t hf_item_cap(const hfcl_lib* lib) { return lib->opt.hfield_items ? lib->opt.hfield_items : HF_ITEM_SOFT_CAP; }

// The call on device pointers: queries [0, n) in chunks; pair0: the index of query 0 in the caller's batch; first: this is the first
// part of that batch (the running contact count starts at 0)
int hf_run(hfcl_lib* lib, const uint32_t* d_hfield, const uint32_t* d_shape, const double* d_tfh, const double* d_tfs, size_t n,
           const uint8_t* d_swapped, const hfcl_collision_request* req, const QParams<double>& q, bool skip_all, hfcl_result* d_out, double* d_dlb,
           hfcl_contact* d_contacts, size_t contacts_cap, bool want_contacts, uint32_t pair0, bool first, hipStream_t st) {
  auto& hf = lib->hf;
  int rc = upload_hfields(lib);
  if (rc) return rc;
  if (!hf.h_words) HIP_TRY(hf.h_words.alloc(2));
  HIP_TRY(hf.d_running.grow(1));
  if (first) HIP_TRY(hipMemsetAsync(hf.d_running, 0, sizeof(uint64_t), st));
  const size_t chunk = std::min(hf_chunk(lib), n);
  HIP_TRY(hf.d_counts.grow(chunk));
  HIP_TRY(hf.d_ccounts.grow(chunk));
  HIP_TRY(hf.d_offsets.grow(chunk + 1));
  HIP_TRY(hf.d_coffsets.grow(chunk + 1));
  HIP_TRY(hf.d_box_total.grow(chunk));
  for (auto& t : lib->timers) t.used = false;
  const bool timed = lib->kernel_timing;
  hipEvent_t e0[HF_TIMED_KERNELS], e1[HF_TIMED_KERNELS];
  const char* names[HF_TIMED_KERNELS];
  if (timed)
    for (int k = 0; k < HF_TIMED_KERNELS; ++k) {
      KernelTime* t = timer_slot(lib, size_t(k), "");
      e0[k] = t->e0;
      e1[k] = t->e1;
    }
  hfcl::HfArgs a;
  a.shapes = lib->d_shapes64;
  a.verts = lib->d_verts64;
  a.n_shapes = uint32_t(lib->n_shapes);
  a.n_fields = uint32_t(hf.h_fields.size());
  a.fields = hf.d_fields;
  a.nodes = hf.d_nodes;
  a.heights = hf.d_heights;
  a.xgrid = hf.d_xgrid;
  a.ygrid = hf.d_ygrid;
  a.q = q;
  a.bd2 = req->break_distance * req->break_distance;
  a.num_max_contacts = req->num_max_contacts;
  a.skip_all = skip_all ? 1 : 0;
  a.counts = hf.d_counts;
  a.offsets = hf.d_offsets;
  a.box_total = hf.d_box_total;
  a.ccounts = hf.d_ccounts;
  a.coffsets = hf.d_coffsets;
  a.running = hf.d_running;
  a.contacts = d_contacts;
  a.contacts_cap = d_contacts ? contacts_cap : 0;
  for (size_t q0 = 0; q0 < n;) {  // (every pass takes at least one query)
    size_t m = std::min(chunk, n - q0);
    a.hfield = d_hfield + q0;
    a.shape = d_shape + q0;
    a.tf_h = d_tfh + 12 * q0;
    a.tf_s = d_tfs + 12 * q0;
    a.swapped = d_swapped ? d_swapped + q0 : nullptr;
    a.out = d_out + q0;
    a.dlb = d_dlb ? d_dlb + q0 : nullptr;
    a.pair0 = pair0 + uint32_t(q0);
    a.m = uint32_t(m);
    a.items = hf.d_items;
    a.leaves = hf.d_leaves;
    a.n_items = 0;
    launch_hf_count(st, a);
    // the one read-back of a chunk: its item count (the item workspace is sized by it); a chunk that lists too much is cut at a query
    uint64_t total = 0;
    for (;;) {  // (m at least halves per pass)
      HIP_TRY(hipMemcpyAsync(hf.h_words, hf.d_offsets.get() + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      total = hf.h_words[0];
      if (total <= hf_item_cap(lib) || m == 1) break;
      m = m / 2;
    }
    if (total > HF_ITEM_HARD_CAP) {
      set_error("hfcl_hfield_collide_batch: one query lists " + std::to_string(total) + " leaves (limit 2^26)");
      return HFCL_ERR_LIMIT;
    }
    if (total > hf.d_items.capacity()) {
      const size_t want = size_t(total + total / 4 + 1024);
      HIP_TRY(hf.d_items.grow(want));
      HIP_TRY(hf.d_leaves.grow(want));
    }
    a.m = uint32_t(m);
    a.items = hf.d_items;
    a.leaves = hf.d_leaves;
    a.n_items = total;
    launch_hf_solve(st, a, lib->n_cus * 16, want_contacts, names, timed ? e0 : nullptr, timed ? e1 : nullptr);
    if (timed)
      for (int k = 0; k < HF_TIMED_KERNELS; ++k) lib->timers[size_t(k)].name = names[k];
    q0 += m;
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

int hf_no_device() {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) {
    set_error("no HIP device available (hipGetDeviceCount): the engine has no CPU fallback");
    return HFCL_ERR_NO_DEVICE;
  }
  return HFCL_OK;
}

extern "C" {

int hfcl_hfield_build(double x_dim, double y_dim, const double* heights, size_t ny, size_t nx, double min_height, hfcl_hfield_node* nodes_out,
                      size_t* n_nodes_out, double* x_grid_out, double* y_grid_out) {
  return hf_build(x_dim, y_dim, heights, ny, nx, min_height, nodes_out, n_nodes_out, x_grid_out, y_grid_out, nullptr);
}

int hfcl_lib_add_hfield(hfcl_lib* lib, double x_dim, double y_dim, const double* heights, size_t ny, size_t nx, double min_height) {
  if (!lib) {
    set_error("hfcl_lib_add_hfield: null library");
    return -1;
  }
  size_t n_nodes = 0;
  if (hf_build(x_dim, y_dim, heights, ny, nx, min_height, nullptr, &n_nodes, nullptr, nullptr, nullptr) != HFCL_OK) return -1;
  if (n_nodes > 0x7FFFFFF0u) {
    set_error("hfcl_lib_add_hfield: height field too large (node ids are 32-bit)");
    return -1;
  }
  auto& hf = lib->hf;
  std::vector<hfcl_hfield_node> nodes(n_nodes);
  std::vector<double> xg(nx), yg(ny), clamped;
  if (hf_build(x_dim, y_dim, heights, ny, nx, min_height, nodes.data(), &n_nodes, xg.data(), yg.data(), &clamped) != HFCL_OK) return -1;
  hfcl::DHfield d;
  d.node_off = hf.h_nodes.size();
  d.height_off = hf.h_heights.size();
  d.xg_off = hf.h_xgrid.size();
  d.yg_off = hf.h_ygrid.size();
  d.n_nodes = uint32_t(n_nodes);
  d.nx = uint32_t(nx);
  d.ny = uint32_t(ny);
  d.pad = 0;
  d.min_height = min_height;
  d.max_height = nodes[0].max_height;
  hf.h_nodes.insert(hf.h_nodes.end(), nodes.begin(), nodes.end());
  hf.h_heights.insert(hf.h_heights.end(), clamped.begin(), clamped.end());
  hf.h_xgrid.insert(hf.h_xgrid.end(), xg.begin(), xg.end());
  hf.h_ygrid.insert(hf.h_ygrid.end(), yg.begin(), yg.end());
  hf.h_fields.push_back(d);
  hf.dirty = true;
  return int(hf.h_fields.size() - 1);
}

int hfcl_lib_clear_hfields(hfcl_lib* lib) {
  if (!lib) {
    set_error("hfcl_lib_clear_hfields: null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  auto& hf = lib->hf;
  hf.h_fields.clear();
  hf.h_nodes.clear();
  hf.h_heights.clear();
  hf.h_xgrid.clear();
  hf.h_ygrid.clear();
  hf.dirty = true;
  return HFCL_OK;
}

size_t hfcl_lib_hfield_count(const hfcl_lib* lib) { return lib ? lib->hf.h_fields.size() : 0; }

int hfcl_hfield_local_aabb(const hfcl_lib* lib, int hfield, double* out6) {
  if (!lib || !out6 || hfield < 0 || size_t(hfield) >= lib->hf.h_fields.size()) {
    set_error("hfcl_hfield_local_aabb: null argument, or not a height field of this library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  const hfcl::DHfield& d = lib->hf.h_fields[size_t(hfield)];
  const double* xg = lib->hf.h_xgrid.data() + d.xg_off;
  const double* yg = lib->hf.h_ygrid.data() + d.yg_off;
  const double a[3] = {xg[0], yg[0], d.min_height}, b[3] = {xg[d.nx - 1], yg[d.ny - 1], d.max_height};
  for (int k = 0; k < 3; ++k) {  // AABB(A, B)
    out6[k] = std::min(a[k], b[k]);
    out6[3 + k] = std::max(a[k], b[k]);
  }
  return HFCL_OK;
}

int hfcl_hfield_pair_supported(int32_t t) { return hfcl::hf_kind_supported(t) ? 1 : 0; }

int hfcl_hfield_collide_batch_device(hfcl_lib* lib, const uint32_t* d_hfield, const uint32_t* d_shape, const double* d_tf_hfield,
                                     const double* d_tf_shape, size_t n, const uint8_t* d_swapped, const hfcl_collision_request* req,
                                     hfcl_result* d_out, double* d_distance_lower_bound, hfcl_contact* d_contacts, size_t max_contacts_total,
                                     size_t* n_contacts_out, void* stream) {
  if (int rc = hf_no_device()) return rc;
  if (!lib || !req) {
    set_error("hfcl_hfield_collide_batch_device: null library / request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  bool skip_all = false;
  if (int rc = hf_request("hfcl_hfield_collide_batch_device", req, q, skip_all)) return rc;
  if (n_contacts_out) *n_contacts_out = 0;
  if (n == 0) return HFCL_OK;
  if (!d_hfield || !d_shape || !d_tf_hfield || !d_tf_shape || !d_out) {
    set_error("hfcl_hfield_collide_batch_device: null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 queries per call)");
    return HFCL_ERR_LIMIT;
  }
  HIP_TRY(hipSetDevice(lib->device));
  hipStream_t st = (hipStream_t)stream;
  const bool want_contacts = d_contacts || n_contacts_out;
  const int rc = hf_run(lib, d_hfield, d_shape, d_tf_hfield, d_tf_shape, n, d_swapped, req, q, skip_all, d_out, d_distance_lower_bound, d_contacts,
                        max_contacts_total, want_contacts, 0u, true, st);
  if (rc) return rc;
  if (n_contacts_out) {
    HIP_TRY(hipMemcpyAsync(lib->hf.h_words.get() + 1, lib->hf.d_running, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_contacts_out = size_t(lib->hf.h_words[1]);
  }
  return HFCL_OK;
}

int hfcl_hfield_collide_batch(hfcl_lib* lib, const uint32_t* hfield, const uint32_t* shape, const double* tf_hfield, const double* tf_shape, size_t n,
                              const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out, double* distance_lower_bound,
                              hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out) {
  if (int rc = hf_no_device()) return rc;
  if (!lib || !req) {
    set_error("hfcl_hfield_collide_batch: null library / request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  bool skip_all = false;
  if (int rc = hf_request("hfcl_hfield_collide_batch", req, q, skip_all)) return rc;
  if (n_contacts_out) *n_contacts_out = 0;
  if (n == 0) return HFCL_OK;
  if (!hfield || !shape || !tf_hfield || !tf_shape || !out) {
    set_error("hfcl_hfield_collide_batch: null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 queries per call)");
    return HFCL_ERR_LIMIT;
  }
  auto& hf = lib->hf;
  for (size_t i = 0; i < n; ++i) {
    if (hfield[i] >= hf.h_fields.size() || shape[i] >= lib->n_shapes) {
      set_error("hfcl_hfield_collide_batch: height field / shape id outside the library at query " + std::to_string(i));
      return HFCL_ERR_INVALID_ARGUMENT;
    }
    if (!hfcl_hfield_pair_supported(lib->h_shapes[shape[i]].type)) {
      set_error("Collision function between a height field and node type " + std::to_string(lib->h_shapes[shape[i]].type) + " is not yet supported.");
      return HFCL_ERR_UNSUPPORTED_PAIR;
    }
  }
  HIP_TRY(hipSetDevice(lib->device));
  if (!hf.st) HIP_TRY(hf.st.create());
  hipStream_t st = hf.st;
  const size_t chunk = std::min(hf_chunk(lib), n);
  const bool want_contacts = contacts || n_contacts_out;
  // the contact list of the whole call stays on the device until the last chunk has run: at most what the queries can produce
  // (a query adds at most num_max_contacts contacts, and no more than the 2^26 leaves it may list)
  const size_t ccap = contacts ? std::min(max_contacts_total, n * size_t(std::min<uint64_t>(req->num_max_contacts, HF_ITEM_HARD_CAP))) : 0;
  HIP_TRY(hf.s_hfield.grow(chunk));
  HIP_TRY(hf.s_shape.grow(chunk));
  HIP_TRY(hf.s_tfh.grow(12 * chunk));
  HIP_TRY(hf.s_tfs.grow(12 * chunk));
  HIP_TRY(hf.s_swapped.grow(chunk));
  HIP_TRY(hf.s_out.grow(chunk));
  HIP_TRY(hf.s_dlb.grow(chunk));
  if (ccap) HIP_TRY(hf.s_contacts.grow(ccap));
  int rc = HFCL_OK;
  for (size_t q0 = 0; q0 < n && !rc; q0 += chunk) {
    const size_t m = std::min(chunk, n - q0);
    bool ok = hipMemcpyAsync(hf.s_hfield, hfield + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(hf.s_shape, shape + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(hf.s_tfh, tf_hfield + 12 * q0, m * 12 * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(hf.s_tfs, tf_shape + 12 * q0, m * 12 * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && (!swapped || hipMemcpyAsync(hf.s_swapped, swapped + q0, m, hipMemcpyHostToDevice, st) == hipSuccess);
    if (!ok) {
      set_error("hfcl_hfield_collide_batch: HIP copy failed");
      rc = HFCL_ERR_HIP;
      break;
    }
    rc = hf_run(lib, hf.s_hfield, hf.s_shape, hf.s_tfh, hf.s_tfs, m, swapped ? hf.s_swapped.get() : nullptr, req, q, skip_all, hf.s_out,
                distance_lower_bound ? hf.s_dlb.get() : nullptr, ccap ? hf.s_contacts.get() : nullptr, ccap, want_contacts, uint32_t(q0), q0 == 0, st);
    if (rc) break;
    ok = hipMemcpyAsync(out + q0, hf.s_out, m * sizeof(hfcl_result), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && (!distance_lower_bound || hipMemcpyAsync(distance_lower_bound + q0, hf.s_dlb, m * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess);
    ok = ok && hipStreamSynchronize(st) == hipSuccess;  // (the staging buffers are the next chunk's)
    if (!ok) {
      set_error("hfcl_hfield_collide_batch: HIP copy failed");
      rc = HFCL_ERR_HIP;
    }
  }
  if (!rc && want_contacts) {
    bool ok = hipMemcpyAsync(hf.h_words.get() + 1, hf.d_running, sizeof(uint64_t), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if (ok) {
      const size_t total = size_t(hf.h_words[1]);
      if (n_contacts_out) *n_contacts_out = total;
      const size_t stored = std::min(total, ccap);
      if (stored) ok = hipMemcpy(contacts, hf.s_contacts, stored * sizeof(hfcl_contact), hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) {
      set_error("hfcl_hfield_collide_batch: HIP copy failed");
      rc = HFCL_ERR_HIP;
    }
  }
  hipStreamSynchronize(st);
  return rc;
}

}  // extern "C"
