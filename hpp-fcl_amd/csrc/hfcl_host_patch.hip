// hfcl_host_patch.hip -- host side of the contact patches (hfcl_contact_patch_batch*; the kernels: hfcl_k_patch.hip, the arithmetic:
// hfcl_patch.hpp).  The library object and what this unit calls of hfcl_host.hip: hfcl_host.hpp.
#include "hfcl_host.hpp"

extern "C" {

// ---- contact patches (hfcl_k_patch.hip) ------------------------------------------------------------------------------
void hfcl_contact_patch_request_init(hfcl_patch_request* r) {
  if (!r) return;
  r->max_num_patch = 1;
  r->num_samples_curved_shapes = 12;
  r->patch_tolerance = 1e-3;
}

int hfcl_patch_supported(int32_t t1, int32_t t2) {
  auto known = [](int32_t t) {
    return t == HFCL_GEOM_BOX || t == HFCL_GEOM_SPHERE || t == HFCL_GEOM_CAPSULE || t == HFCL_GEOM_CONE || t == HFCL_GEOM_CYLINDER ||
           t == HFCL_GEOM_CONVEX || t == HFCL_GEOM_PLANE || t == HFCL_GEOM_HALFSPACE || t == HFCL_GEOM_TRIANGLE ||
           t == HFCL_GEOM_ELLIPSOID || t == HFCL_BV_OBBRSS;
  };
  return known(t1) && known(t2);
}

}  // extern "C"

// the request with the reference's setter clamps (collision_data.h:782-808)
static void patch_request_values(const hfcl_patch_request* r, uint32_t& ns, double& tol) {
  ns = r->num_samples_curved_shapes < 3u ? 3u : r->num_samples_curved_shapes;
  tol = r->patch_tolerance < 0 ? 1e-12 : r->patch_tolerance;
}
static uint32_t patch_shape_bound(const hfcl_shape& s, uint32_t ns) { return patch_set_bound(s.type, s.num_points, ns); }
static uint32_t patch_table_bound(const hfcl_shape* shapes, size_t n_shapes, uint32_t ns) {
  uint32_t m = 1;
  for (size_t k = 0; k < n_shapes; ++k) m = std::max(m, patch_shape_bound(shapes[k], ns));
  return 2 * m;
}
static uint32_t patch_lib_bound(const hfcl_lib* lib, uint32_t ns) { return patch_table_bound(lib->h_shapes.data(), lib->h_shapes.size(), ns); }

// workspace: slots of the polygons of one record each; at most 64k slots, no more than 256 MiB unless 256 slots need it
static int ensure_patch_ws(hfcl_lib* lib, size_t n, uint32_t cap, uint32_t cloud_cap, uint32_t vis_cap, PatchArgs& a) {
  size_t slot = 3 * size_t(cap) * 16 + size_t(cloud_cap) * 16 + size_t(cloud_cap / 2 + 1) * 16 + 8 * size_t(vis_cap) + vis_cap;
  slot = (slot + 255) & ~size_t(255);
  size_t nslots = std::max<size_t>(256, std::min<size_t>(65536, (size_t(256) << 20) / slot));
  nslots = std::min(nslots, std::max<size_t>(n, 1));
  const size_t bytes = nslots * slot;
  HIP_TRY(lib->d_patch_ws.grow(bytes));
  HIP_TRY(lib->d_patch_lists.grow(2 * n));
  HIP_TRY(lib->d_patch_counts.grow(2));
  a.ws = (char*)lib->d_patch_ws.get();
  a.slot_bytes = slot;
  a.nslots = uint32_t(nslots);
  a.cap = cap;
  a.cloud_cap = cloud_cap;
  a.vis_cap = vis_cap;
  a.lists = lib->d_patch_lists;
  a.counts = lib->d_patch_counts;
  return HFCL_OK;
}

static int patch_run(hfcl_lib* lib, const uint32_t* d_s1, const uint32_t* d_s2, const double* d_tf1, const double* d_tf2,
                     const hfcl_result* d_rec, const hfcl_guess* d_guess, size_t n, const hfcl_patch_request* req, uint32_t pcap,
                     hfcl_contact_patch* d_out, double* d_pts, hipStream_t st, uint32_t plim) {
  uint32_t ns;
  double tol;
  patch_request_values(req, ns, tol);
  if (lib->graph_dirty) {
    const int rcg = upload_graph(lib);
    if (rcg) return rcg;
  }
  uint32_t cloud_cap = 8, vis_cap = 0;
  for (size_t k = 0; k < lib->h_shapes.size(); ++k) {
    const hfcl_shape& s = lib->h_shapes[k];
    if (s.type != HFCL_GEOM_CONVEX) continue;
    cloud_cap = std::max(cloud_cap, s.num_points);
    if (s.num_points > 32u && lib->h_graphs.count(uint32_t(k))) vis_cap = std::max(vis_cap, s.num_points);
  }
  PatchArgs a;
  a.s1 = d_s1; a.s2 = d_s2; a.tf1 = d_tf1; a.tf2 = d_tf2; a.rec = d_rec; a.guess = d_guess;
  a.n = uint32_t(n);
  a.n_shapes = uint32_t(lib->n_shapes);
  a.shapes = lib->d_shapes64;
  a.verts = lib->d_verts64;
  a.graph_base = lib->d_graph_base;
  a.graph_off = lib->d_graph_off;
  a.graph_ent = reinterpret_cast<const uint32_t*>(lib->d_graph_ent64);
  a.max_num_patch = req->max_num_patch;
  a.num_samples = ns;
  a.tol = tol;
  a.pcap = pcap;
  a.plim = plim;
  a.out = d_out;
  a.out_pts = d_pts;
  int rc = ensure_patch_ws(lib, n, patch_lib_bound(lib, ns), cloud_cap, vis_cap, a);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(a.counts, 0, 2 * sizeof(uint32_t), st));
  for (auto& t : lib->timers) t.used = false;
  const char* names[3];
  hipEvent_t e0[3], e1[3];
  bool timed = lib->kernel_timing;
  if (timed) {
    for (int k = 0; k < 3; ++k) {
      KernelTime* t = timer_slot(lib, size_t(k), "");
      e0[k] = t->e0;
      e1[k] = t->e1;
    }
  }
  launch_patch(st, a, lib->n_cus * 16, names, timed ? e0 : nullptr, timed ? e1 : nullptr);
  if (timed)
    for (int k = 0; k < 3; ++k) lib->timers[size_t(k)].name = names[k];
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

extern "C" {

int hfcl_contact_patch_max_points(const hfcl_lib* lib, const hfcl_patch_request* req, uint32_t* cap) {
  if (!lib || !req || !cap) {
    set_error("hfcl_contact_patch_max_points: null argument");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  uint32_t ns;
  double tol;
  patch_request_values(req, ns, tol);
  *cap = patch_lib_bound(lib, ns);
  return HFCL_OK;
}

int hfcl_contact_patch_max_points_shapes(const hfcl_shape* shapes, size_t n_shapes, const hfcl_patch_request* req, uint32_t* cap) {
  if ((!shapes && n_shapes) || !req || !cap) {
    set_error("hfcl_contact_patch_max_points_shapes: null argument");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  uint32_t ns;
  double tol;
  patch_request_values(req, ns, tol);
  *cap = patch_table_bound(shapes, n_shapes, ns);
  return HFCL_OK;
}

int hfcl_contact_patch_batch_device(hfcl_lib* lib, const uint32_t* d_shape1, const uint32_t* d_shape2, const double* d_tf1,
                                    const double* d_tf2, const hfcl_result* d_records, const hfcl_guess* d_guesses, size_t n,
                                    const hfcl_patch_request* req, uint32_t points_capacity, hfcl_contact_patch* d_out,
                                    double* d_out_points, void* stream) {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) {
    set_error("no HIP device available (hipGetDeviceCount): the engine has no CPU fallback");
    return HFCL_ERR_NO_DEVICE;
  }
  if (!lib || !req) {
    set_error("hfcl_contact_patch_batch_device: null library / request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return HFCL_OK;
  if (!d_shape1 || !d_shape2 || !d_tf1 || !d_tf2 || !d_records || !d_out || !d_out_points) {
    set_error("hfcl_contact_patch_batch_device: null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 pairs per call)");
    return HFCL_ERR_LIMIT;
  }
  uint32_t ns;
  double tol;
  patch_request_values(req, ns, tol);
  const uint32_t need = patch_lib_bound(lib, ns);
  if (points_capacity < need) {
    set_error("hfcl_contact_patch_batch_device: points_capacity " + std::to_string(points_capacity) + " is below the library's bound " +
              std::to_string(need) + " (hfcl_contact_patch_max_points)");
    return HFCL_ERR_LIMIT;
  }
  HIP_TRY(hipSetDevice(lib->device));
  return patch_run(lib, d_shape1, d_shape2, d_tf1, d_tf2, d_records, d_guesses, n, req, points_capacity, d_out, d_out_points,
                   (hipStream_t)stream, points_capacity);
}

int hfcl_contact_patch_batch(hfcl_lib* lib, const uint32_t* shape1, const uint32_t* shape2, const double* tf1, const double* tf2,
                             const hfcl_result* records, const hfcl_guess* guesses, size_t n, const hfcl_patch_request* req,
                             uint32_t points_capacity, hfcl_contact_patch* out, double* out_points) {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) {
    set_error("no HIP device available (hipGetDeviceCount): the engine has no CPU fallback");
    return HFCL_ERR_NO_DEVICE;
  }
  if (!lib || !req) {
    set_error("hfcl_contact_patch_batch: null library / request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return HFCL_OK;
  if (!shape1 || !shape2 || !tf1 || !tf2 || !records || !out || !out_points) {
    set_error("hfcl_contact_patch_batch: null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 pairs per call)");
    return HFCL_ERR_LIMIT;
  }
  uint32_t ns;
  double tol;
  patch_request_values(req, ns, tol);
  uint32_t need = 0;
  for (size_t i = 0; i < n; ++i) {
    if (shape1[i] >= lib->n_shapes || shape2[i] >= lib->n_shapes) {
      set_error("hfcl_contact_patch_batch: shape id outside the library at record " + std::to_string(i));
      return HFCL_ERR_INVALID_ARGUMENT;
    }
    const hfcl_shape& a = lib->h_shapes[shape1[i]];
    const hfcl_shape& b = lib->h_shapes[shape2[i]];
    if (!hfcl_patch_supported(a.type, b.type)) {
      set_error("Contact patch computation between node types " + std::to_string(a.type) + " and " + std::to_string(b.type) +
                " is not yet supported.");
      return HFCL_ERR_UNSUPPORTED_PAIR;
    }
    need = std::max(need, patch_shape_bound(a, ns) + patch_shape_bound(b, ns));
  }
  if (points_capacity < need) {
    set_error("hfcl_contact_patch_batch: points_capacity " + std::to_string(points_capacity) + " is below the batch's need " +
              std::to_string(need));
    return HFCL_ERR_LIMIT;
  }
  HIP_TRY(hipSetDevice(lib->device));
  if (!lib->patch_st) HIP_TRY(lib->patch_st.create());
  hipStream_t st = lib->patch_st;
  // the workspace slots are sized by the library's bound: records go through a device copy of that width
  const uint32_t dcap = std::max(points_capacity, patch_lib_bound(lib, ns));
  const size_t b_ids = n * sizeof(uint32_t), b_tf = n * 12 * sizeof(double), b_rec = n * sizeof(hfcl_result);
  const size_t b_g = guesses ? n * sizeof(hfcl_guess) : 0, b_out = n * sizeof(hfcl_contact_patch);
  const size_t b_pts = n * size_t(dcap) * 2 * sizeof(double);
  const size_t total = 2 * b_ids + 2 * b_tf + b_rec + b_g + b_out + b_pts + 8 * 256;
  DevBuf<char> block;  // (freed on the way out, after the stream has been waited for)
  HIP_TRY(block.grow(total));
  char* const d = block;
  size_t off = 0;
  auto carve = [&](size_t b) {
    char* p = d + off;
    off += (b + 255) & ~size_t(255);
    return p;
  };
  uint32_t* d_s1 = (uint32_t*)carve(b_ids);
  uint32_t* d_s2 = (uint32_t*)carve(b_ids);
  double* d_tf1 = (double*)carve(b_tf);
  double* d_tf2 = (double*)carve(b_tf);
  hfcl_result* d_rec = (hfcl_result*)carve(b_rec);
  hfcl_guess* d_g = guesses ? (hfcl_guess*)carve(b_g) : nullptr;
  hfcl_contact_patch* d_out = (hfcl_contact_patch*)carve(b_out);
  double* d_pts = (double*)carve(b_pts);
  int rc = HFCL_OK;
  bool ok = hipMemcpyAsync(d_s1, shape1, b_ids, hipMemcpyHostToDevice, st) == hipSuccess;
  ok = ok && hipMemcpyAsync(d_s2, shape2, b_ids, hipMemcpyHostToDevice, st) == hipSuccess;
  ok = ok && hipMemcpyAsync(d_tf1, tf1, b_tf, hipMemcpyHostToDevice, st) == hipSuccess;
  ok = ok && hipMemcpyAsync(d_tf2, tf2, b_tf, hipMemcpyHostToDevice, st) == hipSuccess;
  ok = ok && hipMemcpyAsync(d_rec, records, b_rec, hipMemcpyHostToDevice, st) == hipSuccess;
  ok = ok && (!guesses || hipMemcpyAsync(d_g, guesses, b_g, hipMemcpyHostToDevice, st) == hipSuccess);
  // rows are copied back whole: the points past a record's num_points are zeros, not whatever the allocation held
  ok = ok && hipMemsetAsync(d_pts, 0, b_pts, st) == hipSuccess;
  if (!ok) rc = HFCL_ERR_HIP;
  if (!rc) rc = patch_run(lib, d_s1, d_s2, d_tf1, d_tf2, d_rec, d_g, n, req, dcap, d_out, d_pts, st, points_capacity);
  if (!rc) {
    ok = hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, st) == hipSuccess;
    // rows of dcap points on the device, of points_capacity in the caller's buffer
    ok = ok && hipMemcpy2DAsync(out_points, size_t(points_capacity) * 2 * sizeof(double), d_pts, size_t(dcap) * 2 * sizeof(double),
                                size_t(points_capacity) * 2 * sizeof(double), n, hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) rc = HFCL_ERR_HIP;
  }
  if (rc == HFCL_ERR_HIP) set_error("hfcl_contact_patch_batch: HIP copy / launch failed");
  hipStreamSynchronize(st);
  return rc;
}

}  // extern "C"