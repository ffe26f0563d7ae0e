// hfcl_host_hfield.hip -- host side of the height fields (hppfcl_amd_hfield.h; the kernels: hfcl_k_hfield.hip, the arithmetic:
// hfcl_hfield.hpp): the tree builder, the registration on a library, the upload of the tables, the request checks, and
// hfcl_hfield_collide_batch* -- the entry points and the chunk driver of the listed-leaf pipeline (hfcl_host_listed.hpp) for HfHost,
// the kind defined here.  hf_run is that driver for the terrain calls of the scene unit too.
#include "hfcl_host_listed.hpp"

#include <cmath>

namespace {

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

// (hf_request, hf_chunk, hf_run: declared in hfcl_host.hpp -- the scene unit's terrain calls run their chunks through them)
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

size_t hf_chunk(const hfcl_lib* lib) { return lib->opt.hfield_chunk ? lib->opt.hfield_chunk : LISTED_AUTO_CHUNK; }

namespace {
struct HfHost {
  using Args = hfcl::HfArgs;
  static constexpr const char* limit_who = "hfcl_hfield_collide_batch";
  static constexpr const char* noun = "height field";
  static constexpr const char* a_noun = "a height field";
  static auto& ws(hfcl_lib* lib) { return lib->hf.ws; }
  static size_t n_containers(const hfcl_lib* lib) { return lib->hf.h_fields.size(); }
  static constexpr auto upload = upload_hfields;
  static void fill(hfcl_lib* lib, Args& a) {
    auto& hf = lib->hf;
    a.n_fields = uint32_t(hf.h_fields.size());
    a.fields = hf.d_fields;
    a.nodes = hf.d_nodes;
    a.heights = hf.d_heights;
    a.xgrid = hf.d_xgrid;
    a.ygrid = hf.d_ygrid;
  }
  static void ids(Args& a, const uint32_t* p) { a.hfield = p; }
  static constexpr auto chunk = hf_chunk;
  static uint64_t item_cap(const hfcl_lib* lib) { return lib->opt.hfield_items ? lib->opt.hfield_items : LISTED_ITEM_SOFT_CAP; }
  static constexpr auto request = hf_request;
  static constexpr auto supported = hfcl_hfield_pair_supported;
  static constexpr auto check = listed_no_check;
  static constexpr auto count = launch_hf_count;
  static constexpr auto solve = launch_hf_solve;
};
}  // namespace

int hf_run(hfcl_lib* lib, const uint32_t* d_hfield, const uint32_t* d_shape, const double* d_tfh, const double* d_tfs, size_t n,
           const uint8_t* d_swapped, const hfcl_collision_request* req, const QParams<double>& q, bool skip_all, hfcl_result* d_out, double* d_dlb,
           hfcl_contact* d_contacts, size_t contacts_cap, bool want_contacts, uint32_t pair0, bool first, hipStream_t st) {
  return listed_run<HfHost>(lib, d_hfield, d_shape, d_tfh, d_tfs, n, d_swapped, req, q, skip_all, d_out, d_dlb, d_contacts, contacts_cap, want_contacts,
                            pair0, first, st);
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
  return listed_collide_device<HfHost>("hfcl_hfield_collide_batch_device", lib, d_hfield, d_shape, d_tf_hfield, d_tf_shape, n, d_swapped, req, d_out,
                                       d_distance_lower_bound, d_contacts, max_contacts_total, n_contacts_out, (hipStream_t)stream);
}

int hfcl_hfield_collide_batch(hfcl_lib* lib, const uint32_t* hfield, const uint32_t* shape, const double* tf_hfield, const double* tf_shape, size_t n,
                              const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out, double* distance_lower_bound,
                              hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out) {
  return listed_collide_host<HfHost>("hfcl_hfield_collide_batch", lib, hfield, shape, tf_hfield, tf_shape, n, swapped, req, out, distance_lower_bound,
                                     contacts, max_contacts_total, n_contacts_out);
}

}  // extern "C"
