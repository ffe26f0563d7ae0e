// hfcl_host.hip -- host side: library object, options, uploads, request set-up, host pipeline and their part of the C-ABI implementation of
// include/hppfcl_amd.h (one device-resident batch, the dispatcher run_batch: hfcl_host_batch.hip; contact patches: hfcl_host_patch.hip; scene
// queries and the cull: hfcl_host_scene.hip; the library object itself and what the four units share: hfcl_host.hpp; the host pipeline's chunk
// plan: hfcl_plan.hpp; the kernels live in hfcl_k_gjk.hip / hfcl_k_epa.hip / hfcl_k_bvh.hip / hfcl_k_bvhc.hip / hfcl_k_bvhs.hip, see hfcl_launch.hpp).
// No CPU fallback anywhere in these files: every compute entry point needs a HIP device and fails loudly without one.
//
// Kernel map (pair buckets follow the reference's dispatch table,
// include/hpp/fcl/internal/shape_shape_func.h:185-211 and src/collision_func_matrix.cpp:279-733):
//   k_classify       pair -> bucket lists (block-aggregated atomics), one pass over the shape ids
//   k_closed<T>      closed forms (sphere / capsule / cylinder / box-sphere pairs, every Plane / Halfspace
//                    row), one pair per lane
//   k_gjk_prim<T>    GJK for Box/Capsule/Cone/Cylinder/Ellipsoid/Sphere pairs, one pair per lane
//   k_gjk_cvx<W,M>   GJK with hulls of <= 32 vertices: one pair per W-lane group, hull vertices in the
//                    group's registers, support = per-lane dots + DPP-butterfly arg-max (fp32 / fp64
//                    entry points with their own register budgets)
//   k_gjk_large<T>   GJK when a hull has more than 32 vertices: 16-lane groups scan the vertices from memory
//   k_epa<T,WE,CAP,TIER>  EPA on the pairs GJK left in `Collision`: one polytope per WE-lane group in LDS;
//                    tier 1 = 8 polytopes per wave in small blocks, tier 2 = full capacity (continues the
//                    polytopes tier 1 saved when they outgrew their block; every pair with a large hull)
//   k_epa_stream<T,WE,CAP>  tier 1 for fp32: same blocks, but a lane group whose polytope is done starts the
//                    wave's next item instead of waiting for the slowest of the 8
//   k_bvh_collide<T> / k_bvh_distance<T>   BVHModel<OBBRSS> x BVHModel<OBBRSS>: one mesh pair per lane,
//                    explicit DFS stack in LDS (reference order), OBB SAT / RSS bounds, triangle-triangle leaves;
//                    a walk past its step budget is continued by a wave, 64 stack entries per trip
//                    (k_bvh_coop<T> / k_bvh_distance_coop<T>)
//   k_bvh_collide<T,SOLID> + k_shape_obb<T> + k_bvh_shape_coop<T> + k_bvh_shape_finish<T> (collide, first contact) and
//   k_bvh_shape_distance_lane<T> + k_shape_obbrss<T> + k_bvh_shape_distance_coop<T> (distance)
//                    BVHModel<OBBRSS> x convex solid or Plane/Halfspace the same way: one query per lane, per-lane GJK
//                    leaves, the leaves that need EPA from a queue
//   k_bvh_shape<T> / k_bvh_shape_distance<T>   ... one query per 16-lane group, sequential traversal, leaves =
//                    TriangleP-vs-solid GJK + EPA in LDS: requests that keep walking after a contact
//   k_unsupported<T> flags the pairs of a bucket the engine cannot evaluate (never computed elsewhere)
#include "hfcl_host.hpp"
#include "hfcl_plan.hpp"

// =======================================================================================
// Host side: library object + C ABI
// =======================================================================================
static thread_local std::string g_last_error;
void set_error(const std::string& s) { g_last_error = s; }
void hfcl_internal_set_error(const char* msg) { g_last_error = msg ? msg : ""; }  // hfcl_multi.hip: a worker thread's message handed to the caller's

static void free_retired_graphs(hfcl_lib* lib);

// bucket population i of the last batch (both halves of a split batch)
static uint32_t total_count(const hfcl_lib* lib, int i) {
  if (lib->last_host) return one_count(lib->acc_counts, i);
  uint32_t c = lib->h_counts ? one_count(lib->h_counts, i) : 0u;
  if (lib->last_split && lib->helper && lib->helper->h_counts) c += one_count(lib->helper->h_counts, i);
  return c;
}

static int ensure_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    set_error("no HIP device available (hipGetDeviceCount): the engine has no CPU fallback");
    return HFCL_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n) {
    set_error("device index out of range");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(device));
  return HFCL_OK;
}

extern "C" {

int hfcl_abi_version(void) { return HFCL_ABI_VERSION; }
int hfcl_has_ab_forms(void) { return HFCL_KEEP_AB_FORMS ? 1 : 0; }
int hfcl_pair_supported(int32_t t1, int32_t t2, int for_distance) {
  if (t1 < 0 || t1 > 255 || t2 < 0 || t2 > 255) return 0;
  // 21 is NODE_TYPE HF_OBBRSS to a caller (no row here: height fields have hfcl_hfield_pair_supported); inside, the kernels' class of large hulls
  if (t1 == K_CONVEX_LARGE || t2 == K_CONVEX_LARGE) return 0;
  return bucket_of(t1, t2, for_distance != 0) != B_UNSUPPORTED;
}
int hfcl_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
const char* hfcl_last_error(void) { return g_last_error.c_str(); }

static void query_defaults(hfcl_query_request* q) {
  q->gjk_initial_guess = HFCL_GUESS_DEFAULT;
  q->gjk_variant = HFCL_GJK_DEFAULT;
  q->gjk_convergence_criterion = HFCL_CRIT_DEFAULT;
  q->gjk_convergence_criterion_type = HFCL_CRIT_RELATIVE;
  q->gjk_max_iterations = 128;
  q->epa_max_iterations = 64;
  q->gjk_tolerance = 1e-6;
  q->epa_tolerance = 1e-6;
  q->collision_distance_threshold = 1e-12;
  q->cached_gjk_guess[0] = 1.0;
  q->cached_gjk_guess[1] = 0.0;
  q->cached_gjk_guess[2] = 0.0;
  q->cached_support_func_guess[0] = 0;
  q->cached_support_func_guess[1] = 0;
}
void hfcl_collision_request_init(hfcl_collision_request* r) {
  memset(r, 0, sizeof(*r));
  query_defaults(&r->q);
  r->num_max_contacts = 1;
  r->enable_contact = 1;
  r->security_margin = 0.0;
  r->break_distance = 1e-3;
  r->distance_upper_bound = 1.7976931348623157e+308;
}
void hfcl_distance_request_init(hfcl_distance_request* r) {
  memset(r, 0, sizeof(*r));
  query_defaults(&r->q);
  r->enable_nearest_points = 1;
  r->enable_signed_distance = 1;
  r->rel_err = 0.0;
  r->abs_err = 0.0;
}

static bool validate_shapes(const char* who, const hfcl_shape* shapes, size_t n_shapes, const double* vertices, size_t n_vertices) {
  if (!shapes || n_shapes == 0) {
    set_error(std::string(who) + ": empty shape table");
    return false;
  }
  for (size_t i = 0; i < n_shapes; ++i) {
    const hfcl_shape& s = shapes[i];
    const bool ok_kind = s.type == HFCL_GEOM_BOX || s.type == HFCL_GEOM_SPHERE || s.type == HFCL_GEOM_CAPSULE ||
                         s.type == HFCL_GEOM_ELLIPSOID || s.type == HFCL_GEOM_CONVEX || s.type == HFCL_BV_OBBRSS ||
                         s.type == HFCL_GEOM_TRIANGLE || s.type == HFCL_GEOM_CONE || s.type == HFCL_GEOM_CYLINDER ||
                         s.type == HFCL_GEOM_PLANE || s.type == HFCL_GEOM_HALFSPACE;
    if (!ok_kind) {
      set_error(std::string(who) + ": unsupported shape type " + std::to_string(s.type));
      return false;
    }
    if (s.type == HFCL_GEOM_CONVEX) {
      if (s.num_points == 0 || s.num_points > (uint32_t)HULL_LARGE_MAX) {
        set_error(std::string(who) + ": convex shapes must have 1.." + std::to_string(HULL_LARGE_MAX) + " vertices; got " +
                  std::to_string(s.num_points));
        return false;
      }
      if (size_t(s.vertex_offset) + s.num_points > n_vertices) {
        set_error(std::string(who) + ": convex vertex range out of bounds");
        return false;
      }
    }
    if (s.type == HFCL_GEOM_TRIANGLE && size_t(s.vertex_offset) + 3 > n_vertices) {  // its corners are 3 vertices of the array
      set_error(std::string(who) + ": TriangleP vertex range out of bounds");
      return false;
    }
    if ((s.type == HFCL_GEOM_CONVEX || s.type == HFCL_GEOM_TRIANGLE) && !vertices) {
      set_error(std::string(who) + ": shapes with vertices but no vertex array");
      return false;
    }
  }
  return true;
}

// (Re)build the device shape tables of `lib` from a shape / vertex table: both precisions, the kind bytes of k_classify
// and the set of buckets a pair of these kinds can fall into.
static bool upload_shapes(hfcl_lib* lib, const hfcl_shape* shapes, size_t n_shapes, const double* vertices, size_t n_vertices) {
  lib->n_shapes = n_shapes;
  lib->h_shapes.assign(shapes, shapes + n_shapes);
  lib->h_verts.assign(vertices, vertices + (vertices ? 3 * n_vertices : 0));
  lib->h_graphs.clear();  // shape ids / vertex ranges may have changed: adjacency is registered again by the caller
  lib->graph_dirty = true;
  lib->local_boxes_dirty = true;
  std::vector<DShape<double>> s64(n_shapes);
  std::vector<DShape<float>> s32(n_shapes);
  std::vector<uint8_t> kinds(n_shapes);
  for (size_t i = 0; i < n_shapes; ++i) {
    const hfcl_shape& s = shapes[i];
    s64[i].kind = s.type;
    s64[i].num_points = s.num_points;
    s64[i].vertex_offset = s.vertex_offset;
    s64[i].bvh_index = s.bvh_index;
    s64[i].p0 = s.params[0];
    s64[i].p1 = s.params[1];
    s64[i].p2 = s.params[2];
    s64[i].p3 = s.params[3];
    s64[i].ssr = s.swept_sphere_radius;
    s32[i].kind = s.type;
    s32[i].num_points = s.num_points;
    s32[i].vertex_offset = s.vertex_offset;
    s32[i].bvh_index = s.bvh_index;
    s32[i].p0 = float(s.params[0]);
    s32[i].p1 = float(s.params[1]);
    s32[i].p2 = float(s.params[2]);
    s32[i].p3 = float(s.params[3]);
    s32[i].ssr = float(s.swept_sphere_radius);
    if (s.type == HFCL_GEOM_CONVEX && s.num_points > 0 && vertices &&
        size_t(s.vertex_offset) + s.num_points <= n_vertices) {  // centre of aabb_local, for BoundingVolumeGuess
      double mn[3], mx[3];
      const double* v = vertices + 3 * size_t(s.vertex_offset);
      for (int k = 0; k < 3; ++k) mn[k] = mx[k] = v[k];
      for (uint32_t j = 1; j < s.num_points; ++j)
        for (int k = 0; k < 3; ++k) {
          mn[k] = std::min(mn[k], v[3 * size_t(j) + k]);
          mx[k] = std::max(mx[k], v[3 * size_t(j) + k]);
        }
      s64[i].p0 = (mn[0] + mx[0]) * 0.5; s64[i].p1 = (mn[1] + mx[1]) * 0.5; s64[i].p2 = (mn[2] + mx[2]) * 0.5;
      s32[i].p0 = float(s64[i].p0); s32[i].p1 = float(s64[i].p1); s32[i].p2 = float(s64[i].p2);
    }
    kinds[i] = uint8_t(s.type == HFCL_GEOM_CONVEX && s.num_points > (uint32_t)HULL_MAX ? K_CONVEX_LARGE : s.type);
  }
  {
    bool present[256] = {false};
    for (size_t i = 0; i < n_shapes; ++i) present[kinds[i]] = true;
    uint32_t mask = 1u << B_UNSUPPORTED;  // shape ids out of range can always occur
    for (int a = 0; a < 256; ++a)
      if (present[a])
        for (int b = 0; b < 256; ++b)
          if (present[b]) mask |= 1u << bucket_of(a, b);
    lib->possible_buckets = mask;
    lib->has_curved = present[K_ELLIPSOID] || present[K_CONE] || present[K_CYLINDER];
    lib->has_flats = present[K_PLANE] || present[K_HALFSPACE];
    lib->has_capsules = present[K_CAPSULE];
  }
  lib->h_kinds = kinds;
  std::vector<float> v32(3 * n_vertices + 3);
  for (size_t i = 0; i < 3 * n_vertices; ++i) v32[i] = float(vertices[i]);
  hfcl_lib::Tables& t = lib->own;
  reset_all(t.shapes64, t.shapes32, t.kinds, t.verts64, t.verts32);
  bool ok = true;
  ok = ok && t.shapes64.grow(n_shapes) == hipSuccess;
  ok = ok && t.shapes32.grow(n_shapes) == hipSuccess;
  ok = ok && t.kinds.grow(n_shapes) == hipSuccess;
  ok = ok && t.verts64.grow(3 * n_vertices + 3) == hipSuccess;
  ok = ok && t.verts32.grow(3 * n_vertices + 3) == hipSuccess;
  if (ok) {
    ok = ok && hipMemcpy(t.shapes64, s64.data(), n_shapes * sizeof(DShape<double>), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(t.shapes32, s32.data(), n_shapes * sizeof(DShape<float>), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(t.kinds, kinds.data(), n_shapes, hipMemcpyHostToDevice) == hipSuccess;
    if (n_vertices) {
      ok = ok && hipMemcpy(t.verts64, vertices, 3 * n_vertices * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
      ok = ok && hipMemcpy(t.verts32, v32.data(), 3 * n_vertices * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    }
  }
  share_tables(lib, lib);  // the library's own view of them
  return ok;
}

// ---------------------------------------------------------------------------------------
// Tuning options (include/hppfcl_amd.h: hfcl_lib_set_option).  One table: the keys, and what each sets.  Every option is a field of
// the library read when a batch is set up, so an option holds from the next call on; none changes a record (tests/test_options_gpu.py
// holds every value against the default form byte for byte; a new key needs a row in tests/options_table.py), they choose between forms
// of the same computation and size their budgets.  The one exception -- the last bits of `distance` in fp64 mesh x mesh collide() under
// bvh_coop = 0 / bvh_walk_rounds = 0 / bvh_force_wide = 1, every decision the same bytes -- and the triangle named inside a 0-ulp tie
// class of distance() under pool_rerun = 0, bvhd_pool = 0, shape_dist_pool = 0, bvh_shape_lane = 0 are in the header and in
// INTEGRATION.md section 4.  A value outside an option's range is refused, never clamped (apply_option).
// ---------------------------------------------------------------------------------------
static const char* const* option_keys() {
  static const char* const keys[] = {
      "closed_staged", "split", "epa_cc_staged", "epa_records_aside", "epa_general_staged", "shape_finish_tiers", "shape_finish_aside",
      "epa_general_staged_min", "epa64_two_streams", "epa_cc_staged_min", "pipe_chunk", "bvh_filter", "bvh_shape_lane", "shape_coop",
      "bvh_cut_ticks", "shape_cut_ticks", "bvh_coop", "bvhd_budget", "bvhd_pool", "shape_dist_pool", "pool_rerun", "bvh_walk_early_coop",
      "bvh_walk_rounds", "bvh_walk_order", "mesh_beside", "mesh_prio", "shape_walk", "shape_walk_sort", "shape_walk_budget", "shape_walk_min", "gjk_beside_max", "epa_direct_max", "bvh_walk_k", "bvh_walk_budget", "shape_dist_leaf_min", "shape_dist_starve", "bvhd_leaf_min", "bvhd_starve",
      "bvhd_part_min", "shape_dist_budget", "bvh_budget0_coop", "shape_budget0", "shape_budget", "shape_leaf_cost", "shape_levels",
      "climb_min", "bvh_budget", "bvh_budget0", "bvh_levels", "cvx_w", "epa_resume_slots", "bvh_task_slots", "bvh_force_wide",
      "pipe_trace", "scene_chunk", "scene_cull_chunk", "scene_pairs_small_max", "scene_pairs_sorted", "scene_pairs_sorted_axis", "scene_env_span", "scene_nearest_env_prune", "epa_pool_share", "epa_pool_min_refills", "hfield_chunk", "hfield_items", "octree_chunk", "octree_items", nullptr};
  return keys;
}
// One unsigned decimal number, the whole string: digits only -- no sign, no blank, nothing behind it -- and lo <= value <= hi.
static bool parse_uint(const char* p, const char* end, unsigned long long lo, unsigned long long hi, unsigned long long* out) {
  if (p == end || end - p > 20) return false;
  unsigned long long x = 0;
  for (; p != end; ++p) {
    if (*p < '0' || *p > '9') return false;
    const unsigned long long d = (unsigned long long)(*p - '0');
    if (x > (~0ull - d) / 10) return false;  // (past 2^64 - 1)
    x = x * 10 + d;
  }
  if (x < lo || x > hi) return false;
  *out = x;
  return true;
}
// "4,16,16": one to `cap` comma-separated unsigned values, each in lo .. hi, into out[0 ...]; returns how many there are, 0 when any
// element is not a number in range, when one is empty or when there are too many (out is then not to be used)
static int parse_list(const char* v, uint32_t* out, int cap, uint32_t lo, uint32_t hi) {
  int k = 0;
  for (const char* p = v;; ++k) {
    const char* e = p;
    while (*e && *e != ',') ++e;
    unsigned long long x;
    if (k >= cap || !parse_uint(p, e, lo, hi, &x)) return 0;
    out[k] = uint32_t(x);
    if (!*e) return k + 1;
    p = e + 1;
  }
}
// The value is parsed and checked against the option's range first; the library is written only when all of it is valid, so a refused
// call changes nothing (include/hppfcl_amd.h).  No value is clamped: what is outside an option's range is refused.
static int apply_option(hfcl_lib* lib, const std::string& key, const char* v) {
  constexpr unsigned long long U32 = 0xFFFFFFFFull, SIZE = 1ull << 40;
  hfcl_options& o = lib->opt;
  unsigned long long x = 0;
  bool on = false;
  auto num = [&](unsigned long long lo, unsigned long long hi) { return parse_uint(v, v + strlen(v), lo, hi, &x); };
  auto flag = [&]() {
    const bool ok = num(0, 1);
    on = x != 0;
    return ok;
  };
  auto set_flag = [&](bool& field) {
    if (!flag()) return int(HFCL_ERR_INVALID_ARGUMENT);
    field = on;
    return int(HFCL_OK);
  };
  auto set_u32 = [&](uint32_t& field, unsigned long long lo, unsigned long long hi) {
    if (!num(lo, hi)) return int(HFCL_ERR_INVALID_ARGUMENT);
    field = uint32_t(x);
    return int(HFCL_OK);
  };
  auto set_size = [&](size_t& field, unsigned long long hi) {
    if (!num(0, hi)) return int(HFCL_ERR_INVALID_ARGUMENT);
    field = size_t(x);
    return int(HFCL_OK);
  };
  if (key == "closed_staged") return set_flag(o.closed_staged);
  if (key == "split") {
    if (!num(0, 2)) return HFCL_ERR_INVALID_ARGUMENT;
    o.split = int(x);
    return HFCL_OK;
  }
  if (key == "epa_cc_staged") return set_flag(o.epa_cc_staged);
  if (key == "epa_records_aside") return set_flag(o.records_aside);
  if (key == "epa_general_staged") {
    if (!flag() || (on && !HFCL_KEEP_AB_FORMS)) return HFCL_ERR_INVALID_ARGUMENT;  // (not in the product build: hfcl_dev.hpp)
    o.epa_general_staged = on;
    return HFCL_OK;
  }
  if (key == "shape_finish_tiers") return set_flag(o.shape_finish_tiers);
  if (key == "shape_finish_aside") return set_flag(o.shape_finish_aside);
  if (key == "epa_general_staged_min") return set_size(o.epa_general_staged_min, SIZE);
  if (key == "epa64_two_streams") return set_flag(o.epa64_two_streams);
  if (key == "epa_cc_staged_min") return set_size(o.epa_cc_staged_min, SIZE);
  if (key == "pipe_chunk") return set_size(o.pipe_chunk, SIZE);
  if (key == "bvh_filter") {
    if (!flag() || (on && !HFCL_KEEP_AB_FORMS)) return HFCL_ERR_INVALID_ARGUMENT;
    o.bvh_filter = on;
    return HFCL_OK;
  }
  if (key == "bvh_shape_lane") return set_flag(o.bvh_shape_lane);
  if (key == "shape_coop") return set_flag(o.shape_coop);
  if (key == "bvh_cut_ticks") return set_u32(o.bvh_cut_ticks, 0, U32);
  if (key == "shape_cut_ticks") return set_u32(o.shape_cut_ticks, 0, U32);
  if (key == "bvh_coop") return set_flag(o.bvh_coop);
  if (key == "bvhd_budget") return set_u32(o.bvhd_budget, 0, U32);
  if (key == "bvhd_pool") return set_u32(o.bvhd_pool, 0, 1);
  if (key == "shape_dist_pool") return set_u32(o.shape_dist_pool, 0, 1);
  if (key == "pool_rerun") return set_u32(o.pool_rerun, 0, 2);
  if (key == "bvh_walk_early_coop") return set_flag(o.walk_early_coop);
  if (key == "bvh_walk_order") return set_flag(o.walk_order);
  if (key == "mesh_beside") {
    if (!num(0, 4) || x == 3) return HFCL_ERR_INVALID_ARGUMENT;
    o.mesh_beside = uint32_t(x);
    return HFCL_OK;
  }
  if (key == "shape_walk") return set_flag(o.shape_walk);
  if (key == "mesh_prio") return set_flag(o.mesh_prio);
  if (key == "shape_walk_sort") return set_flag(o.shape_walk_sort);
  if (key == "shape_walk_budget") return set_u32(o.shape_walk_budget, 0, U32);
  if (key == "shape_walk_min") return set_u32(o.shape_walk_min, 0, U32);
  if (key == "gjk_beside_max") return set_u32(o.gjk_beside_max, 0, U32);
  if (key == "epa_direct_max") return set_u32(o.epa_direct_max, 0, U32);
  if (key == "epa_pool_share") return set_u32(o.epa_pool_share, 0, 50);
  if (key == "epa_pool_min_refills") return set_u32(o.epa_pool_min_refills, 0, U32);
  if (key == "bvh_walk_rounds") {
    if (!num(0, WALK_ROUNDS)) return HFCL_ERR_INVALID_ARGUMENT;
    o.walk_rounds = uint32_t(x);
    o.walk_auto = false;
    return HFCL_OK;
  }
  if (key == "bvh_walk_k") {  // "6,16": per round
    uint32_t k[WALK_ROUNDS];
    const int n = parse_list(v, k, WALK_ROUNDS, 1u, uint32_t(WALK_K));
    if (!n) return HFCL_ERR_INVALID_ARGUMENT;
    std::copy(k, k + n, o.walk_k);
    o.walk_auto = false;
    return HFCL_OK;
  }
  if (key == "bvh_walk_budget") {  // rounds 1 ...: box tests (round 0 takes bvh_budget0_coop's)
    uint32_t b[WALK_ROUNDS - 1];
    const int n = parse_list(v, b, WALK_ROUNDS - 1, 0u, 0xFFFFFFFFu);
    if (!n) return HFCL_ERR_INVALID_ARGUMENT;
    std::copy(b, b + n, o.walk_budget + 1);
    return HFCL_OK;
  }
  if (key == "shape_dist_leaf_min") return set_u32(o.shape_dist_leaf_min, 1, U32);
  if (key == "shape_dist_starve") return set_u32(o.shape_dist_starve, 1, U32);  // (>= 1: a window of triangles alone must always run)
  if (key == "bvhd_leaf_min") return set_u32(o.bvhd_pool_leaf_min, 1, U32);
  if (key == "bvhd_starve") return set_u32(o.bvhd_pool_starve, 1, U32);
  if (key == "bvhd_part_min") return set_u32(o.bvhd_pool_part_min, 0, U32);
  if (key == "shape_dist_budget") return set_u32(o.shape_dist_budget, 0, U32);
  if (key == "bvh_budget0_coop") return set_u32(o.bvh_budget0_coop, 1, U32);
  if (key == "shape_budget0") {
    if (!num(0, U32)) return HFCL_ERR_INVALID_ARGUMENT;
    o.shape_budget0 = o.shape_budget0_coop = uint32_t(x);
    return HFCL_OK;
  }
  if (key == "shape_budget") return set_u32(o.shape_budget, 0, U32);
  if (key == "shape_leaf_cost") return set_u32(o.shape_leaf_cost, 1, U32);
  if (key == "shape_levels") return set_u32(o.shape_levels, 1, BVH_MAX_LEVELS);
  if (key == "climb_min") return set_u32(o.climb_min, 0, U32);
  if (key == "bvh_budget") {
    if (!num(0, U32)) return HFCL_ERR_INVALID_ARGUMENT;
    o.bvh_budget = o.bvh_budget0 = uint32_t(x);
    o.bvh_auto = false;
    return HFCL_OK;
  }
  if (key == "bvh_budget0") {
    if (!num(0, U32)) return HFCL_ERR_INVALID_ARGUMENT;
    o.bvh_budget0 = uint32_t(x);
    o.bvh_auto = false;
    return HFCL_OK;
  }
  if (key == "bvh_levels") {
    if (!num(1, BVH_MAX_LEVELS)) return HFCL_ERR_INVALID_ARGUMENT;
    o.bvh_levels = uint32_t(x);
    o.bvh_auto = false;
    return HFCL_OK;
  }
  if (key == "cvx_w") {
    if (!num(0, 64) || (x != 0 && (x < 2 || (x & (x - 1)) != 0))) return HFCL_ERR_INVALID_ARGUMENT;  // 0, 2, 4, 8, 16, 32, 64
    o.cvx_w = int(x);
    return HFCL_OK;
  }
  if (key == "epa_resume_slots") return set_size(o.epa_resume_slots, SIZE);
  if (key == "bvh_task_slots") return set_size(o.bvh_task_slots, 1ull << 16);  // (the table is slots x queries entries)
  if (key == "bvh_force_wide") return set_flag(o.bvh_force_wide);
  if (key == "pipe_trace") return set_flag(o.pipe_trace);
  if (key == "scene_chunk") return set_size(o.scene_chunk, 0xFFFFFFF0ull);
  if (key == "scene_cull_chunk") return set_size(o.scene_cull_chunk, 1ull << 31);  // (one workgroup scans a chunk's counts: 2^23 of them at most)
  if (key == "scene_pairs_small_max") return set_u32(o.scene_pairs_small_max, 0, PAIRS_SMALL_MAX);  // (a lane per column)
  if (key == "scene_pairs_sorted") return set_flag(o.scene_pairs_sorted);
  if (key == "scene_pairs_sorted_axis") return set_u32(o.scene_pairs_sorted_axis, 0, 3);  // (3: automatic, per configuration)
  if (key == "scene_env_span") return set_u32(o.scene_env_span, 0, U32);
  if (key == "scene_nearest_env_prune") return set_flag(o.scene_nearest_env_prune);
  if (key == "hfield_chunk") return set_size(o.hfield_chunk, 0xFFFFFFF0ull);
  if (key == "hfield_items") return set_size(o.hfield_items, 1ull << 26);  // (the item workspace of one query's limit)
  if (key == "octree_chunk") return set_size(o.octree_chunk, 0xFFFFFFF0ull);
  if (key == "octree_items") return set_size(o.octree_items, 1ull << 26);  // (the item workspace of one query's limit)
  return HFCL_ERR_INVALID_ARGUMENT;
}

hfcl_lib* hfcl_lib_create(const hfcl_shape* shapes, size_t n_shapes, const double* vertices, size_t n_vertices,
                          int device) {
  if (ensure_device(device) != HFCL_OK) return nullptr;
  if (!validate_shapes("hfcl_lib_create", shapes, n_shapes, vertices, n_vertices)) return nullptr;
  hfcl_lib* lib = new hfcl_lib();
  lib->device = device;
  bool ok = upload_shapes(lib, shapes, n_shapes, vertices, n_vertices);
  ok = ok && lib->d_counts.grow(N_COUNTER_WORDS) == hipSuccess;
  ok = ok && lib->h_counts.alloc(N_COUNTERS) == hipSuccess;
  if (ok) memset(lib->h_counts, 0, N_COUNTERS * sizeof(uint32_t));
  if (!ok) {
    set_error("hfcl_lib_create: HIP allocation/copy failed");
    hfcl_lib_destroy(lib);
    return nullptr;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) lib->n_cus = prop.multiProcessorCount;
  // one slot per lane group of the largest full-capacity EPA grid (run_batch caps grids at n_cus * 16 blocks)
  if (lib->d_epa_v0.grow(size_t(lib->n_cus) * 16 * (64 / EPA_WE2) * EPA_MAX_VERTS * sizeof(Quad<double>)) != hipSuccess) {
    set_error("hfcl_lib_create: HIP allocation failed");
    hfcl_lib_destroy(lib);
    return nullptr;
  }
  // Tuning options: hfcl_lib_set_option is the interface; the environment (HFCL_<KEY>) is read ONCE, here, as a fallback for
  // processes that cannot call it (A/B runs of an unchanged binary).
  for (const char* const* k = option_keys(); *k; ++k) {
    std::string name = "HFCL_";
    for (const char* c = *k; *c; ++c) name.push_back(char(toupper(static_cast<unsigned char>(*c))));
    if (const char* v = getenv(name.c_str()))
      if (apply_option(lib, *k, v) != HFCL_OK) fprintf(stderr, "[hfcl] %s=%s in the environment is not a value of option %s: ignored\n", name.c_str(), v, *k);
  }
  return lib;
}

// (every buffer, stream and event of the library is a handle that frees itself: hfcl_own.hpp)
void hfcl_lib_destroy(hfcl_lib* lib) {
  if (!lib) return;
  hipSetDevice(lib->device);
  hipDeviceSynchronize();
  if (lib->helper) hfcl_lib_destroy(lib->helper);
  delete lib;
}
// Replace the shape table of a library in place: registered BVH models, workspaces, staging buffers and streams stay
// (a caller that keeps adding geometries -- the hpp::fcl shim -- does not pay a full rebuild with every new shape).
int hfcl_lib_set_shapes(hfcl_lib* lib, const hfcl_shape* shapes, size_t n_shapes, const double* vertices, size_t n_vertices) {
  if (!lib) {
    set_error("null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (!validate_shapes("hfcl_lib_set_shapes", shapes, n_shapes, vertices, n_vertices)) return HFCL_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(lib->device));
  HIP_TRY(hipDeviceSynchronize());  // nothing of this library may still be reading the old tables
  free_retired_graphs(lib);
  if (!upload_shapes(lib, shapes, n_shapes, vertices, n_vertices)) {
    set_error("hfcl_lib_set_shapes: HIP allocation/copy failed");
    return HFCL_ERR_HIP;
  }
  if (lib->helper) share_tables(lib->helper, lib);  // the second half of split batches reads the same tables
  ++lib->shapes_epoch;  // (the scenes of this library hold shape ids of the old table)
  return HFCL_OK;
}

// Vertex adjacency of a convex shape (ConvexBase::neighbors, shape/geometric_shapes.h; Convex<PolygonT>::fillNeighbors,
// shape/details/convex.hxx:231-280): offsets[num_points + 1] into neighbors[], vertex indices relative to the shape's first
// vertex.  Hulls of at least HFCL_CLIMB_MIN vertices that have one answer support queries by hill-climbing
// (getShapeSupportLog) instead of scanning all vertices; without one (or below the threshold) nothing changes.
int hfcl_lib_set_convex_neighbors(hfcl_lib* lib, uint32_t shape_id, const uint32_t* offsets, const uint32_t* neighbors) {
  if (!lib || !offsets || !neighbors) {
    set_error("hfcl_lib_set_convex_neighbors: null argument");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (shape_id >= lib->n_shapes || lib->h_shapes[shape_id].type != HFCL_GEOM_CONVEX) {
    set_error("hfcl_lib_set_convex_neighbors: not a convex shape of this library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  const uint32_t n = lib->h_shapes[shape_id].num_points;
  if (offsets[0] != 0) {
    set_error("hfcl_lib_set_convex_neighbors: offsets[0] must be 0");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) {
      set_error("hfcl_lib_set_convex_neighbors: offsets must not decrease");
      return HFCL_ERR_INVALID_ARGUMENT;
    }
  if (offsets[n] == 0) {
    set_error("hfcl_lib_set_convex_neighbors: empty adjacency");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  for (uint32_t k = 0; k < offsets[n]; ++k)
    if (neighbors[k] >= n) {
      set_error("hfcl_lib_set_convex_neighbors: neighbour index outside the shape's vertices");
      return HFCL_ERR_INVALID_ARGUMENT;
    }
  hfcl_lib::HostGraph& g = lib->h_graphs[shape_id];
  g.off.assign(offsets, offsets + n + 1);
  g.ids.assign(neighbors, neighbors + offsets[n]);
  lib->graph_dirty = true;
  return HFCL_OK;
}
size_t hfcl_lib_num_shapes(const hfcl_lib* lib) { return lib ? lib->n_shapes : 0; }
int hfcl_lib_device(const hfcl_lib* lib) { return lib ? lib->device : -1; }
uint32_t hfcl_lib_climb_min(const hfcl_lib* lib) { return lib ? lib->opt.climb_min : 0u; }

int hfcl_lib_add_bvh(hfcl_lib* lib, const hfcl_bvh_node* nodes, size_t n_nodes, const double* vertices,
                     size_t n_vertices, const uint32_t* triangles, size_t n_tris) {
  if (!lib || !nodes || !vertices || !triangles || n_tris == 0) {
    set_error("hfcl_lib_add_bvh: null/empty input");
    return -1;
  }
  if (n_nodes != 2 * n_tris - 1) {  // BVH_model.cpp:821-825
    set_error("hfcl_lib_add_bvh: a BVHModel with T triangles has exactly 2T-1 nodes");
    return -1;
  }
  if (n_nodes > 0x7FFFFFF0u || n_vertices > 0xFFFFFFF0u) {
    set_error("hfcl_lib_add_bvh: model too large (node / vertex ids are 32-bit)");
    return -1;
  }
  for (size_t i = 0; i < n_nodes; ++i) {
    const int fc = nodes[i].first_child;
    if (fc == 0 || (fc > 0 && size_t(fc) + 1 > n_nodes - 1) || (fc < 0 && size_t(-(fc + 1)) >= n_tris)) {
      set_error("hfcl_lib_add_bvh: malformed node array (first_child out of range)");
      return -1;
    }
  }
  for (size_t i = 0; i < 3 * n_tris; ++i)
    if (triangles[i] >= n_vertices) {
      set_error("hfcl_lib_add_bvh: triangle vertex index out of range");
      return -1;
    }
  DMesh m;
  m.node_off = uint32_t(lib->h_bvh_nodes.size());
  m.vert_off = uint32_t(lib->h_bvh_verts.size() / 3);
  m.tri_off = uint32_t(lib->h_bvh_tris.size() / 3);
  m.n_nodes = uint32_t(n_nodes);
  lib->h_bvh_nodes.insert(lib->h_bvh_nodes.end(), nodes, nodes + n_nodes);
  lib->h_bvh_verts.insert(lib->h_bvh_verts.end(), vertices, vertices + 3 * n_vertices);
  lib->h_bvh_tris.insert(lib->h_bvh_tris.end(), triangles, triangles + 3 * n_tris);
  lib->h_meshes.push_back(m);
  lib->h_mesh_nverts.push_back(uint32_t(n_vertices));
  lib->local_boxes_dirty = true;
  {  // depth of the tree (the traversal stacks are sized from it) -- iterative: degenerate models are as deep as they are big
    std::vector<std::pair<uint32_t, uint32_t>> todo;
    todo.emplace_back(0u, 1u);
    uint32_t depth = 1;
    while (!todo.empty()) {
      const auto [i, d] = todo.back();
      todo.pop_back();
      depth = std::max(depth, d);
      const int fc = nodes[i].first_child;
      if (fc > 0) {
        todo.emplace_back(uint32_t(fc), d + 1);
        todo.emplace_back(uint32_t(fc) + 1u, d + 1);
      }
    }
    lib->bvh_max_depth = std::max(lib->bvh_max_depth, depth);
    lib->bvh_max_nodes = std::max<size_t>(lib->bvh_max_nodes, n_nodes);
  }
  lib->bvh_dirty = true;
  return int(lib->h_meshes.size() - 1);
}

}  // extern "C"

template <typename T>
static DNode<T> pack_node(const hfcl_bvh_node& n) {
  DNode<T> d;
  d.first_child = n.first_child;
  d.pad_ = 0;
  const double* a = n.obb_axes;  // column-major
  d.axes.r0 = mk<T>(T(a[0]), T(a[3]), T(a[6]));
  d.axes.r1 = mk<T>(T(a[1]), T(a[4]), T(a[7]));
  d.axes.r2 = mk<T>(T(a[2]), T(a[5]), T(a[8]));
  d.To = mk<T>(T(n.obb_To[0]), T(n.obb_To[1]), T(n.obb_To[2]));
  d.extent = mk<T>(T(n.obb_extent[0]), T(n.obb_extent[1]), T(n.obb_extent[2]));
  return d;
}

// Device image of the registered vertex adjacencies: per shape [14 warm-start vertices][num_points + 1 offsets] in
// d_graph_off, the neighbours with their coordinates inline in d_graph_ent32/64 (one fetch per hop instead of two).
// The warm-start vertices are the support vertices along the 14 directions of ConvexBase::buildSupportWarmStart
// (src/shape/geometric_shapes.cpp: the six axis directions and the eight cube diagonals).
static void free_retired_graphs(hfcl_lib* lib) { lib->graph_retired.clear(); }  // (the caller has waited for the device)
// No device-wide wait (round 4): the previous image is retired, not freed, the new one is copied on a non-blocking stream
// of its own and the host waits for that stream only -- freeing it and the null-stream hipMemcpy the first version used both
// stall every stream of the device, inside an entry point documented as asynchronous.
int upload_graph(hfcl_lib* lib) {
  if (!lib->graph_dirty) return HFCL_OK;
  HIP_TRY(hipSetDevice(lib->device));
  // (an application that re-registers neighbours between batches must not grow device memory without bound: after four retired
  // images the device is waited for once and they are freed)
  if (lib->graph_retired.size() >= 4) {
    HIP_TRY(hipDeviceSynchronize());
    free_retired_graphs(lib);
  }
  hfcl_lib::GraphImage& img = lib->own.graph;
  if (img.base) lib->graph_retired.push_back(std::move(img));  // (an image is whole or not there at all; moved from, it is empty)
  lib->graph_dirty = false;
  if (lib->h_graphs.empty()) {
    share_tables(lib, lib);
    if (lib->helper) share_tables(lib->helper, lib);
    return HFCL_OK;
  }
  std::vector<uint32_t> base(lib->n_shapes, HFCL_NO_GRAPH), off;
  std::vector<NbrEntry<float>> e32;
  std::vector<NbrEntry<double>> e64;
  static const double dirs[HFCL_WARM_STARTS][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1},
                                                   {1, 1, 1}, {-1, 1, 1}, {1, -1, 1}, {-1, -1, 1}, {1, 1, -1}, {-1, 1, -1}, {1, -1, -1}, {-1, -1, -1}};
  for (const auto& kv : lib->h_graphs) {
    const hfcl_shape& sh = lib->h_shapes[kv.first];
    const hfcl_lib::HostGraph& g = kv.second;
    const double* v = lib->h_verts.data() + 3 * size_t(sh.vertex_offset);
    for (int k = 0; k < HFCL_WARM_STARTS; ++k) {
      uint32_t bi = 0;
      double best = -1.7976931348623157e+308;
      for (uint32_t j = 0; j < sh.num_points; ++j) {
        if (g.off[j + 1] == g.off[j]) continue;  // not a hull vertex: no way on from there
        const double d = v[3 * size_t(j)] * dirs[k][0] + v[3 * size_t(j) + 1] * dirs[k][1] + v[3 * size_t(j) + 2] * dirs[k][2];
        if (d > best) {
          best = d;
          bi = j;
        }
      }
      off.push_back(bi);
    }
    base[kv.first] = uint32_t(off.size());
    const size_t e0 = e64.size();
    if (e0 + g.ids.size() > 0xFFFFFFF0u) {
      set_error("hfcl_lib_set_convex_neighbors: more than 2^32 adjacency entries in one library");
      return HFCL_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t o : g.off) off.push_back(uint32_t(e0) + o);
    for (uint32_t id : g.ids) {
      const double* p = v + 3 * size_t(id);
      NbrEntry<double> a;
      a.x = p[0]; a.y = p[1]; a.z = p[2]; a.id = id; a.pad_ = 0;
      NbrEntry<float> b;
      b.x = float(p[0]); b.y = float(p[1]); b.z = float(p[2]); b.id = id;
      e64.push_back(a);
      e32.push_back(b);
    }
  }
  bool ok = img.base.grow(base.size()) == hipSuccess;
  ok = ok && img.off.grow(off.size()) == hipSuccess;
  ok = ok && img.ent32.grow(e32.size() + 1) == hipSuccess;
  ok = ok && img.ent64.grow(e64.size() + 1) == hipSuccess;
  if (!lib->upload_stream) ok = ok && lib->upload_stream.create() == hipSuccess;
  hipStream_t us = lib->upload_stream;
  ok = ok && hipMemcpyAsync(img.base, base.data(), base.size() * sizeof(uint32_t), hipMemcpyHostToDevice, us) == hipSuccess;
  ok = ok && hipMemcpyAsync(img.off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, us) == hipSuccess;
  ok = ok && (e32.empty() || hipMemcpyAsync(img.ent32, e32.data(), e32.size() * sizeof(NbrEntry<float>), hipMemcpyHostToDevice, us) == hipSuccess);
  ok = ok && (e64.empty() || hipMemcpyAsync(img.ent64, e64.data(), e64.size() * sizeof(NbrEntry<double>), hipMemcpyHostToDevice, us) == hipSuccess);
  ok = ok && hipStreamSynchronize(us) == hipSuccess;  // the host vectors go out of scope; kernels launched after this see the image
  if (!ok) {  // nothing half-built stays behind: the next batch retries the upload from the host copies
    img = hfcl_lib::GraphImage();
    lib->graph_dirty = true;
    share_tables(lib, lib);
    if (lib->helper) share_tables(lib->helper, lib);
    set_error("vertex adjacency: HIP allocation/copy failed");
    return HFCL_ERR_HIP;
  }
  share_tables(lib, lib);
  if (lib->helper) share_tables(lib->helper, lib);
  return HFCL_OK;
}

int upload_bvh(hfcl_lib* lib) {
  if (!lib->bvh_dirty) return HFCL_OK;
  reset_all(lib->d_nodes64, lib->d_nodes32, lib->d_bverts64, lib->d_bverts32, lib->d_btris, lib->d_meshes, lib->d_rss64, lib->d_rss32,
            lib->d_fnodes, lib->d_dnodes64, lib->d_dnodes32);
  const size_t nn = lib->h_bvh_nodes.size(), nv = lib->h_bvh_verts.size(), nt = lib->h_bvh_tris.size();
  std::vector<DNode<double>> n64(nn);
  std::vector<DNode<float>> n32(nn);
  std::vector<DRss<double>> r64(nn);
  std::vector<DRss<float>> r32(nn);
  for (size_t i = 0; i < nn; ++i) {
    const hfcl_bvh_node& hn = lib->h_bvh_nodes[i];
    n64[i] = pack_node<double>(hn);
    n32[i] = pack_node<float>(hn);
    r64[i].Tr = mk<double>(hn.rss_Tr[0], hn.rss_Tr[1], hn.rss_Tr[2]);
    r64[i].l0 = hn.rss_length[0];
    r64[i].l1 = hn.rss_length[1];
    r64[i].r = hn.rss_radius;
    r32[i].Tr = mk<float>(float(hn.rss_Tr[0]), float(hn.rss_Tr[1]), float(hn.rss_Tr[2]));
    // fp32 image of the RSS must still contain the fp64 one: round the radius up a little
    r32[i].l0 = float(hn.rss_length[0]);
    r32[i].l1 = float(hn.rss_length[1]);
    r32[i].r = float(hn.rss_radius) * (1.0f + 4e-7f) + 1e-7f;
  }
  std::vector<float> v32(nv);
  for (size_t i = 0; i < nv; ++i) v32[i] = float(lib->h_bvh_verts[i]);
  {  // filter records: sizes compared through their rank among all nodes of the library (exact, hfcl_bvh.hpp)
    std::vector<uint32_t> rank(nn);
    obbf_size_ranks(lib->h_bvh_nodes.data(), nn, rank.data());
    std::vector<DNodeF> fn(nn);
    for (size_t i = 0; i < nn; ++i) fn[i] = pack_fnode(lib->h_bvh_nodes[i], rank[i]);
    HIP_TRY(lib->d_fnodes.grow(nn));
    HIP_TRY(hipMemcpy(lib->d_fnodes, fn.data(), nn * sizeof(DNodeF), hipMemcpyHostToDevice));
    // the distance() walk's records: axes + RSS + child link + the same ranks
    std::vector<DNodeD<double>> d64(nn);
    std::vector<DNodeD<float>> d32(nn);
    for (size_t i = 0; i < nn; ++i) {
      d64[i].axes = n64[i].axes; d64[i].Tr = r64[i].Tr; d64[i].l0 = r64[i].l0; d64[i].l1 = r64[i].l1; d64[i].r = r64[i].r;
      d64[i].first_child = n64[i].first_child; d64[i].rank = rank[i];
      d32[i].axes = n32[i].axes; d32[i].Tr = r32[i].Tr; d32[i].l0 = r32[i].l0; d32[i].l1 = r32[i].l1; d32[i].r = r32[i].r;
      d32[i].first_child = n32[i].first_child; d32[i].rank = rank[i];
    }
    HIP_TRY(lib->d_dnodes64.grow(nn));
    HIP_TRY(lib->d_dnodes32.grow(nn));
    HIP_TRY(hipMemcpy(lib->d_dnodes64, d64.data(), nn * sizeof(DNodeD<double>), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lib->d_dnodes32, d32.data(), nn * sizeof(DNodeD<float>), hipMemcpyHostToDevice));
  }
  HIP_TRY(lib->d_nodes64.grow(nn));
  HIP_TRY(lib->d_nodes32.grow(nn));
  HIP_TRY(lib->d_bverts64.grow(nv));
  HIP_TRY(lib->d_bverts32.grow(nv));
  HIP_TRY(lib->d_btris.grow(nt));
  HIP_TRY(lib->d_meshes.grow(lib->h_meshes.size()));
  HIP_TRY(hipMemcpy(lib->d_nodes64, n64.data(), nn * sizeof(DNode<double>), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(lib->d_nodes32, n32.data(), nn * sizeof(DNode<float>), hipMemcpyHostToDevice));
  HIP_TRY(lib->d_rss64.grow(nn));
  HIP_TRY(lib->d_rss32.grow(nn));
  HIP_TRY(hipMemcpy(lib->d_rss64, r64.data(), nn * sizeof(DRss<double>), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(lib->d_rss32, r32.data(), nn * sizeof(DRss<float>), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(lib->d_bverts64, lib->h_bvh_verts.data(), nv * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(lib->d_bverts32, v32.data(), nv * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(lib->d_btris, lib->h_bvh_tris.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(lib->d_meshes, lib->h_meshes.data(), lib->h_meshes.size() * sizeof(DMesh), hipMemcpyHostToDevice));
  lib->bvh_dirty = false;
  return HFCL_OK;
}

KernelTime* timer_slot(hfcl_lib* lib, size_t i, const char* name) {
  while (lib->timers.size() <= i) {
    KernelTime t;
    t.name = "";
    t.used = false;
    (void)t.e0.create(hipEventDefault);
    (void)t.e1.create(hipEventDefault);
    lib->timers.push_back(std::move(t));
  }
  lib->timers[i].name = name;
  lib->timers[i].used = true;
  return &lib->timers[i];
}

int no_device() {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) {
    set_error("no HIP device available (hipGetDeviceCount): the engine has no CPU fallback");
    return HFCL_ERR_NO_DEVICE;
  }
  return HFCL_OK;
}

template <typename T>
static void fill_qparams(QParams<T>& q, const hfcl_query_request& r) {
  q.gjk.tolerance = T(r.gjk_tolerance);
  q.gjk.max_iterations = r.gjk_max_iterations;
  q.gjk.variant = r.gjk_variant;
  q.gjk.crit = r.gjk_convergence_criterion;
  q.gjk.crit_type = r.gjk_convergence_criterion_type;
  q.epa_tolerance = T(r.epa_tolerance);
  q.epa_max_iterations = int(r.epa_max_iterations);
  q.collision_distance_threshold = T(r.collision_distance_threshold);
  q.guess_mode = r.gjk_initial_guess;
  q.guess[0] = T(r.cached_gjk_guess[0]);
  q.guess[1] = T(r.cached_gjk_guess[1]);
  q.guess[2] = T(r.cached_gjk_guess[2]);
}

static int validate_query(const hfcl_query_request& q) {
  if (!(q.gjk_tolerance > 0) || !(q.epa_tolerance > 0)) {
    set_error("tolerance must be positive (gjk.cpp:62)");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (q.epa_max_iterations > (uint32_t)EPA_MAX_ITER) {
    set_error("epa_max_iterations > 64 exceeds the device polytope capacity");
    return HFCL_ERR_LIMIT;
  }
  if (q.gjk_variant < 0 || q.gjk_variant > 2 || q.gjk_convergence_criterion < 0 || q.gjk_convergence_criterion > 2 ||
      q.gjk_convergence_criterion_type < 0 || q.gjk_convergence_criterion_type > 1) {
    set_error("invalid GJK variant / convergence criterion");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (q.gjk_initial_guess < 0 || q.gjk_initial_guess > HFCL_GUESS_BOUNDING_VOLUME) {
    set_error("Wrong initial guess for GJK.");  // narrowphase.h:379-380
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return HFCL_OK;
}

template <typename T>
int setup_collide(const hfcl_collision_request* req, QParams<T>& q, bool& skip_all) {
  skip_all = false;
  if (!req) {
    set_error("null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (req->num_max_contacts == 0) {  // src/collision.cpp:82-85
    set_error("Invalid number of max contacts (current value is 0).");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  int rc = validate_query(req->q);
  if (rc) return rc;
  fill_qparams(q, req->q);
  q.mode = 1;
  q.compute_penetration = (req->enable_contact || req->security_margin < 0) ? 1 : 0;  // shape_shape_func.h:141-142
  q.security_margin = T(req->security_margin);
  // narrowphase.h:228-229
  double ub = req->distance_upper_bound > req->security_margin ? req->distance_upper_bound : req->security_margin;
  if (ub < 0) ub = 0;
  q.gjk.distance_upper_bound = (ub >= double(Lim<T>::max())) ? Lim<T>::max() : T(ub);
  if (req->security_margin == -__builtin_inf()) skip_all = true;  // src/collision.cpp:73-76
  return HFCL_OK;
}
template <typename T>
int setup_distance(const hfcl_distance_request* req, QParams<T>& q) {
  if (!req) {
    set_error("null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  int rc = validate_query(req->q);
  if (rc) return rc;
  fill_qparams(q, req->q);
  q.mode = 0;
  q.compute_penetration = req->enable_signed_distance ? 1 : 0;
  q.security_margin = T(0);
  q.gjk.distance_upper_bound = Lim<T>::max();  // narrowphase.h:175
  return HFCL_OK;
}

template int setup_collide<double>(const hfcl_collision_request*, QParams<double>&, bool&);  // (hfcl_host_scene.hip)
template int setup_collide<float>(const hfcl_collision_request*, QParams<float>&, bool&);
template int setup_distance<double>(const hfcl_distance_request*, QParams<double>&);
template int setup_distance<float>(const hfcl_distance_request*, QParams<float>&);

// full records -> compact records (hfcl_result_compact), for the multi-GPU exchange of results
template <typename R, typename C>
static int compact_results(hfcl_lib* lib, const R* d_records, size_t n, C* d_out, void* stream) {
  if (!lib) {
    set_error("null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return HFCL_OK;
  if (!d_records || !d_out) {
    set_error("hfcl_compact_results_device: null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 pairs per call)");
    return HFCL_ERR_LIMIT;
  }
  HIP_TRY(hipSetDevice(lib->device));
  launch_compact_records((hipStream_t)stream, d_records, d_out, uint32_t(n));
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}
extern "C" {

int hfcl_collide_batch_device(hfcl_lib* lib, const uint32_t* d_shape1, const uint32_t* d_shape2, const double* d_tf1,
                              const double* d_tf2, size_t n, const hfcl_collision_request* req, hfcl_result* d_out,
                              const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  if (!lib) {
    set_error("null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  bool skip;
  int rc = setup_collide<double>(req, q, skip);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (skip) {
    HIP_TRY(hipSetDevice(lib->device));
    if (n) launch_fill_skipped(st, d_out, uint32_t(n));
    return HFCL_OK;
  }
  IO<double> io{d_tf1, d_tf2, d_out, d_guess_in, d_guess_out};
  lib->bvh_params.num_max_contacts = req->num_max_contacts;
  lib->break_distance = req->break_distance;
  return run_batch<double>(lib, d_shape1, d_shape2, io, n, q, st);
}

int hfcl_distance_batch_device(hfcl_lib* lib, const uint32_t* d_shape1, const uint32_t* d_shape2, const double* d_tf1,
                               const double* d_tf2, size_t n, const hfcl_distance_request* req, hfcl_result* d_out,
                               const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  if (!lib) {
    set_error("null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  int rc = setup_distance<double>(req, q);
  if (rc) return rc;
  IO<double> io{d_tf1, d_tf2, d_out, d_guess_in, d_guess_out};
  return run_batch<double>(lib, d_shape1, d_shape2, io, n, q, (hipStream_t)stream);
}

int hfcl_distance_batch_device_f32(hfcl_lib* lib, const uint32_t* d_shape1, const uint32_t* d_shape2,
                                   const float* d_pose1, const float* d_pose2, size_t n,
                                   const hfcl_distance_request* req, hfcl_result_f32* d_out, void* stream) {
  if (!lib) {
    set_error("null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<float> q;
  int rc = setup_distance<float>(req, q);
  if (rc) return rc;
  IO<float> io{d_pose1, d_pose2, d_out, nullptr, nullptr};
  return run_batch<float>(lib, d_shape1, d_shape2, io, n, q, (hipStream_t)stream);
}

int hfcl_collide_batch_device_f32(hfcl_lib* lib, const uint32_t* d_shape1, const uint32_t* d_shape2,
                                  const float* d_pose1, const float* d_pose2, size_t n,
                                  const hfcl_collision_request* req, hfcl_result_f32* d_out, void* stream) {
  if (!lib) {
    set_error("null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<float> q;
  bool skip;
  int rc = setup_collide<float>(req, q, skip);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (skip) {
    HIP_TRY(hipSetDevice(lib->device));
    if (n) launch_fill_skipped(st, d_out, uint32_t(n));
    return HFCL_OK;
  }
  IO<float> io{d_pose1, d_pose2, d_out, nullptr, nullptr};
  lib->bvh_params.num_max_contacts = req->num_max_contacts;
  lib->break_distance = req->break_distance;
  return run_batch<float>(lib, d_shape1, d_shape2, io, n, q, st);
}

int hfcl_compact_results_device(hfcl_lib* lib, const hfcl_result* d_records, size_t n, hfcl_result_compact* d_out, void* stream) {
  return compact_results(lib, d_records, n, d_out, stream);
}
int hfcl_compact_results_device_f32(hfcl_lib* lib, const hfcl_result_f32* d_records, size_t n, hfcl_result_compact_f32* d_out,
                                    void* stream) {
  return compact_results(lib, d_records, n, d_out, stream);
}

static int ensure_staging(hfcl_lib* lib, size_t n, bool gin, bool gout, bool compact) {
  if (!lib->s_cmp) {  // the streams, the slots' events and counter blocks: made into locals and committed together
    Stream st[4];
    Event ev[hfcl_lib::PIPE_SLOTS][3];
    PinnedBuf<uint32_t> hc[hfcl_lib::PIPE_SLOTS][2];
    for (Stream& x : st) HIP_TRY(x.create());
    for (int k = 0; k < hfcl_lib::PIPE_SLOTS; ++k) {
      for (Event& e : ev[k]) HIP_TRY(e.create());
      for (PinnedBuf<uint32_t>& h : hc[k]) HIP_TRY(h.alloc(N_COUNTERS));
    }
    for (int k = 0; k < hfcl_lib::PIPE_SLOTS; ++k) {
      hfcl_lib::Staging& sg = lib->stage[k];
      sg.ev_in = std::move(ev[k][0]);
      sg.ev_done = std::move(ev[k][1]);
      sg.ev_in2 = std::move(ev[k][2]);
      sg.h_counts = std::move(hc[k][0]);
      sg.h_counts2 = std::move(hc[k][1]);
    }
    lib->s_h2d = std::move(st[0]);
    lib->s_h2d2 = std::move(st[1]);
    lib->s_d2h = std::move(st[3]);
    lib->s_cmp = std::move(st[2]);
  }
  if (n > lib->st_capacity) {
    lib->st_capacity = 0;
    const size_t cap = n + n / 8 + 256;
    for (auto& sg : lib->stage) {
      reset_all(sg.d_s1, sg.d_s2, sg.d_tf1, sg.d_tf2, sg.d_out, sg.d_gin, sg.d_gout, sg.d_qt1, sg.d_qt2);
      HIP_TRY(sg.d_s1.grow(cap));
      HIP_TRY(sg.d_s2.grow(cap));
      HIP_TRY(sg.d_tf1.grow(cap * 12));
      HIP_TRY(sg.d_tf2.grow(cap * 12));
      HIP_TRY(sg.d_out.grow(cap));
    }
    lib->st_capacity = cap;
  }
  for (auto& sg : lib->stage) {
    if (gin) HIP_TRY(sg.d_gin.grow(lib->st_capacity));
    if (gout) HIP_TRY(sg.d_gout.grow(lib->st_capacity));
    if (compact) {
      HIP_TRY(sg.d_qt1.grow(lib->st_capacity * 7));
      HIP_TRY(sg.d_qt2.grow(lib->st_capacity * 7));
    }
  }
  return HFCL_OK;
}

// what a host batch reports after its records are back: pairs without an evaluator, requests the reference rejects
int host_batch_checks(hfcl_lib* lib, const hfcl_collision_request* creq, const hfcl_distance_request* dreq) {
  const bool skipped = creq && creq->security_margin == -__builtin_inf();
  if (!skipped && total_count(lib, B_UNSUPPORTED) > 0) {
    set_error("Collision/distance function between some node types of the batch is not yet supported (" +
              std::to_string(total_count(lib, B_UNSUPPORTED)) + " pairs; their records carry status bit 31)");
    return HFCL_ERR_UNSUPPORTED_PAIR;
  }
  {
    // a TriangleP built inside the reference (top-level TriangleP overloads, mesh x shape leaves) never had
    // computeLocalAABB() called: BoundingVolumeGuess throws there (narrowphase.h:366-373)
    const hfcl_query_request& qq = creq ? creq->q : dreq->q;
    if (!skipped && qq.gjk_initial_guess == HFCL_GUESS_BOUNDING_VOLUME &&
        (total_count(lib, B_TRI) > 0 || total_count(lib, B_BVHSHAPE) > 0)) {
      set_error("computeLocalAABB must have been called on the shapes before using GJKInitialGuess::BoundingVolumeGuess.");
      return HFCL_ERR_INVALID_ARGUMENT;
    }
  }
  if (!skipped && creq && creq->security_margin < 0 && total_count(lib, B_BVHSHAPE) > 0) {
    set_error("Negative security margin are not handled yet for BVHModel");  // collision_func_matrix.cpp:109-112
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (!skipped && (total_count(lib, B_BVH) > 0 || total_count(lib, B_BVHSHAPE) > 0) && lib->h_meshes.empty()) {
    set_error("BVH shapes in the batch but no BVHModel registered (hfcl_lib_add_bvh)");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return HFCL_OK;
}

// A small batch from a library of many shape kinds pays a launch for every bucket the LIBRARY can reach (up to a dozen
// dependent launches, ~5 us each) although its pairs fall into one or two: the host has the ids, so it classifies them
// itself and, for the lifetime of this object, only the kernels of buckets that hold a pair are launched (a single
// box x box pair: 5 launches instead of 12).
struct SmallBatchBuckets {
  hfcl_lib* lib;
  uint32_t library_buckets;
  SmallBatchBuckets(hfcl_lib* l, const uint32_t* s1, const uint32_t* s2, size_t n, bool distance_mode) : lib(l), library_buckets(l->possible_buckets) {
    if (n > 1024 || lib->h_kinds.size() != lib->n_shapes) return;
    uint32_t mask = 0;
    for (size_t i = 0; i < n; ++i)
      mask |= 1u << ((s1[i] < lib->n_shapes && s2[i] < lib->n_shapes) ? bucket_of(lib->h_kinds[s1[i]], lib->h_kinds[s2[i]], distance_mode)
                                                                       : int(B_UNSUPPORTED));
    lib->possible_buckets = mask & (library_buckets | (1u << B_UNSUPPORTED));
    if (lib->helper) lib->helper->possible_buckets = lib->possible_buckets;
  }
  ~SmallBatchBuckets() {
    lib->possible_buckets = library_buckets;
    if (lib->helper) lib->helper->possible_buckets = library_buckets;
  }
};

// Host batch of at most hfcl_lib::SMALL_MAX pairs: the per-call cost is what counts (a hpp::fcl::collide() caller sends one
// pair).  Every input array is packed into one pinned block, which crosses the link as ONE copy; the kernels and the one
// copy back run on the same stream; the call waits for that stream.  (Five pageable copies, the event hand-overs between
// three streams and the copy back cost ~85 us of host time per call; profiles/r03_d.)
static int host_batch_small(hfcl_lib* lib, const uint32_t* s1, const uint32_t* s2, const double* tf1, const double* tf2, size_t n,
                            const hfcl_collision_request* creq, const hfcl_distance_request* dreq, hfcl_result* out,
                            const hfcl_guess* gin, hfcl_guess* gout, bool compact) {
  constexpr size_t C = hfcl_lib::SMALL_MAX;
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t pose_in = compact ? 7 : 12;
  // block layout for n pairs: [pose1][pose2][guess in][ids 1][ids 2] | [records][guess out] | [expanded poses 1][2] (device only)
  const size_t o_p1 = 0, o_p2 = o_p1 + n * pose_in * 8, o_gin = o_p2 + n * pose_in * 8, o_s1 = o_gin + (gin ? n * sizeof(hfcl_guess) : 0),
               o_s2 = o_s1 + up(n * 4), in_bytes = o_s2 + up(n * 4);
  const size_t o_out = up(in_bytes), o_gout = o_out + n * sizeof(hfcl_result), out_bytes = n * sizeof(hfcl_result) + (gout ? n * sizeof(hfcl_guess) : 0);
  const size_t o_tf1 = up(o_out + out_bytes), o_tf2 = o_tf1 + n * 96;
  if (!lib->d_pack) {
    const size_t cap = up(C * (2 * 96 + sizeof(hfcl_guess)) + 2 * up(C * 4)) + up(C * (sizeof(hfcl_result) + sizeof(hfcl_guess))) + 2 * C * 96 + 1024;
    HIP_TRY(lib->h_pack.alloc(cap));
    HIP_TRY(lib->h_pack_counts.alloc(2 * N_COUNTERS));
    HIP_TRY(lib->d_pack.grow(cap));
  }
  if (!lib->s_cmp) {  // (the pipeline's streams; this path uses the compute stream only)
    const int rc0 = ensure_staging(lib, 256, false, false, false);
    if (rc0) return rc0;
  }
  char* h = lib->h_pack;
  char* d = lib->d_pack;
  memcpy(h + o_p1, tf1, n * pose_in * 8);
  memcpy(h + o_p2, tf2, n * pose_in * 8);
  if (gin) memcpy(h + o_gin, gin, n * sizeof(hfcl_guess));
  memcpy(h + o_s1, s1, n * 4);
  memcpy(h + o_s2, s2, n * 4);
  hipStream_t st = lib->s_cmp;
  HIP_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
  const double *d_tf1 = reinterpret_cast<const double*>(d + o_p1), *d_tf2 = reinterpret_cast<const double*>(d + o_p2);
  if (compact) {
    launch_expand_poses(st, d_tf1, reinterpret_cast<double*>(d + o_tf1), uint32_t(n));
    launch_expand_poses(st, d_tf2, reinterpret_cast<double*>(d + o_tf2), uint32_t(n));
    d_tf1 = reinterpret_cast<const double*>(d + o_tf1);
    d_tf2 = reinterpret_cast<const double*>(d + o_tf2);
  }
  HostBatchScope scope(lib);
  if (lib->note_forms) lib->host_notes = "host_packed=1;";
  memset(lib->h_pack_counts, 0, 2 * N_COUNTERS * sizeof(uint32_t));
  lib->counts_dst = lib->h_pack_counts;
  if (lib->helper) lib->helper->counts_dst = lib->h_pack_counts + N_COUNTERS;  // (a batch this small is never split)
  int rc;
  {
    SmallBatchBuckets batch_buckets(lib, s1, s2, n, dreq != nullptr);
    const uint32_t* d_s1 = reinterpret_cast<const uint32_t*>(d + o_s1);
    const uint32_t* d_s2 = reinterpret_cast<const uint32_t*>(d + o_s2);
    const hfcl_guess* d_gin = gin ? reinterpret_cast<const hfcl_guess*>(d + o_gin) : nullptr;
    hfcl_guess* d_gout = gout ? reinterpret_cast<hfcl_guess*>(d + o_gout) : nullptr;
    if (creq)
      rc = hfcl_collide_batch_device(lib, d_s1, d_s2, d_tf1, d_tf2, n, creq, reinterpret_cast<hfcl_result*>(d + o_out), d_gin, d_gout, st);
    else
      rc = hfcl_distance_batch_device(lib, d_s1, d_s2, d_tf1, d_tf2, n, dreq, reinterpret_cast<hfcl_result*>(d + o_out), d_gin, d_gout, st);
  }
  hipError_t e = hipSuccess;
  if (rc == HFCL_OK) e = hipMemcpyAsync(h + o_out, d + o_out, out_bytes, hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);  // (also after a failed launch sequence: nothing of this call stays in flight)
  if (rc) return rc;
  if (e != hipSuccess || e2 != hipSuccess) {
    set_error(std::string("host batch (small): ") + hipGetErrorString(e != hipSuccess ? e : e2));
    return HFCL_ERR_HIP;
  }
  memcpy(out, h + o_out, n * sizeof(hfcl_result));
  if (gout) memcpy(gout, h + o_gout, n * sizeof(hfcl_guess));
  for (int i = 0; i < N_COUNTERS; ++i) lib->acc_counts[i] = lib->h_pack_counts[i] + (lib->last_split ? lib->h_pack_counts[N_COUNTERS + i] : 0u);
  lib->last_host = true;
  return host_batch_checks(lib, creq, dreq);
}

// Host-buffer entry point = the drop-in boundary a user of hpp::fcl::collide() / distance() gets.  The batch is cut into
// chunks that flow through a three-stage pipeline on three streams: H2D of chunk k+1 | kernels of chunk k | D2H of chunk
// k-1, over PIPE_SLOTS device buffer sets.  The caller's thread feeds the pipeline (copies in, launches); a helper thread
// drains it (waits for a chunk's kernels, adds up its bucket populations, copies the records out, releases the slot).  The
// copies go straight from / to the caller's (pageable) arrays: the runtime moves them at the link rate (tools/valu_peak.hip:
// 56 GB/s pageable vs 57 GB/s pinned, 37.6 GB/s per direction when both run), an extra staging memcpy would only add a
// 33 GB/s single-thread stage.  No device-wide synchronisation: other streams of the process are not disturbed.
// pipelined = false (contact lists: their pair ids are batch-wide) runs the batch as one chunk.
static int host_batch(hfcl_lib* lib, const uint32_t* s1, const uint32_t* s2, const double* tf1, const double* tf2,
                      size_t n, const hfcl_collision_request* creq, const hfcl_distance_request* dreq, hfcl_result* out,
                      const hfcl_guess* gin, hfcl_guess* gout, bool pipelined = true, bool compact = false, bool f32 = false) {
  // f32 (hfcl_*_batch_f32): tf1 / tf2 are 7-FLOAT poses and `out` hfcl_result_f32 records, both smaller than what the slots' buffers hold for the
  // fp64 formats, so the same staging serves; the chunks go through the fp32 device path.  No guesses in that format.
  if (!lib) {
    set_error("null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return HFCL_OK;
  if (!s1 || !s2 || !tf1 || !tf2 || !out) {
    set_error("null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(lib->device));
  if (pipelined && n <= hfcl_lib::SMALL_MAX && !lib->opt.pipe_chunk && !f32) return host_batch_small(lib, s1, s2, tf1, tf2, n, creq, dreq, out, gin, gout, compact);
  const std::vector<size_t> bounds = plan_chunks(n, lib->opt.pipe_chunk, pipelined, f32);  // chunk k = [bounds[k], bounds[k + 1]): hfcl_plan.hpp
  size_t max_chunk = 0;
  for (size_t k = 0; k + 1 < bounds.size(); ++k) max_chunk = std::max(max_chunk, bounds[k + 1] - bounds[k]);
  const size_t n_chunks = bounds.size() - 1;
  if (lib->note_forms) lib->host_notes = "host_chunks=" + std::to_string(n_chunks) + ";host_max_chunk=" + std::to_string(max_chunk) + ";host_trace=" + std::to_string(int(lib->opt.pipe_trace)) + ";";
  int rc = ensure_staging(lib, max_chunk, gin != nullptr, gout != nullptr, compact);
  if (rc) return rc;
  SmallBatchBuckets batch_buckets(lib, s1, s2, n, dreq != nullptr);
  constexpr int S = hfcl_lib::PIPE_SLOTS;
  HostBatchScope scope(lib);  // (before the threads: they are joined on every way out)

  // Host threads keep the streams busy.  A copy between pageable memory and the device holds its caller until the data
  // has moved (above a few MB; the first time a range of host memory is used it is also pinned, several times slower),
  // so every stream that copies has a thread of its own: two feeders (the arrays of object 1 and of object 2, on two
  // streams: one blocking copy at a time leaves the link idle between copies, 42 instead of 50 GB/s), the drainer
  // (records out, queued behind the chunk's kernels on the stream; bucket populations), and the caller's thread, which
  // launches the kernels of a chunk as soon as its inputs are on their way (profiles/r03_c).
  std::mutex mu;
  std::condition_variable cv;
  size_t copied[2] = {0, 0}, issued = 0, drained = 0;  // chunks whose inputs are queued / whose kernels are launched / whose records are back
  int side_rc = HFCL_OK;                       // first failure of the feeder or the drainer
  std::string side_err;
  bool abort_all = false;
  auto side_fail = [&](const char* who, hipError_t e) {
    std::lock_guard<std::mutex> lk(mu);
    if (side_rc == HFCL_OK) {
      side_rc = HFCL_ERR_HIP;
      side_err = std::string("host batch (") + who + "): " + hipGetErrorString(e);
    }
    abort_all = true;
    cv.notify_all();
  };

  // option pipe_trace: per-chunk time line of the three threads on stderr (ms since the call started)
  const bool trace = lib->opt.pipe_trace;
  const auto t_call = std::chrono::steady_clock::now();
  auto ms_now = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
  std::vector<double> tr(trace ? 6 * n_chunks : 0);
  // `copied[h]`: chunks whose arrays of object h + 1 (ids, poses; h = 0 also the guesses) are queued
  auto feed = [&](int h) {
    hipSetDevice(lib->device);
    hipStream_t st = h ? lib->s_h2d2 : lib->s_h2d;
    for (size_t k = 0; k < n_chunks; ++k) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return drained + S > k || abort_all; });  // the slot's previous chunk must be back on the host
        if (abort_all) return;
      }
      hfcl_lib::Staging& sg = lib->stage[k % S];
      const size_t lo = bounds[k], m = bounds[k + 1] - lo;
      if (trace && !h) tr[6 * k] = ms_now();
      const uint32_t* ids = h ? s2 : s1;
      const double* tf = h ? tf2 : tf1;
      hipError_t e = hipMemcpyAsync(h ? sg.d_s2 : sg.d_s1, ids + lo, m * sizeof(uint32_t), hipMemcpyHostToDevice, st);
      if (f32) {
        if (e == hipSuccess) e = hipMemcpyAsync(h ? sg.d_tf2 : sg.d_tf1, reinterpret_cast<const float*>(tf) + 7 * lo, m * 7 * sizeof(float), hipMemcpyHostToDevice, st);
      } else if (compact) {  // tf1 / tf2 are 7-double poses: expanded to Transform3f images by the first kernel of the chunk
        if (e == hipSuccess) e = hipMemcpyAsync(h ? sg.d_qt2 : sg.d_qt1, tf + 7 * lo, m * 7 * sizeof(double), hipMemcpyHostToDevice, st);
      } else {
        if (e == hipSuccess) e = hipMemcpyAsync(h ? sg.d_tf2 : sg.d_tf1, tf + 12 * lo, m * 12 * sizeof(double), hipMemcpyHostToDevice, st);
      }
      if (e == hipSuccess && gin && !h) e = hipMemcpyAsync(sg.d_gin, gin + lo, m * sizeof(hfcl_guess), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipEventRecord(h ? sg.ev_in2 : sg.ev_in, st);
      if (e != hipSuccess) {
        side_fail("feed", e);
        return;
      }
      if (trace && !h) tr[6 * k + 1] = ms_now();
      std::lock_guard<std::mutex> lk(mu);
      copied[h] = k + 1;
      cv.notify_all();
    }
  };
  auto drain = [&]() {
    hipSetDevice(lib->device);
    for (size_t k = 0; k < n_chunks; ++k) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return issued > k || abort_all; });
        if (abort_all && issued <= k) return;
      }
      hfcl_lib::Staging& sg = lib->stage[k % S];
      const size_t lo = bounds[k], m = bounds[k + 1] - lo;
      // the records' way back is queued behind the chunk's kernels on the third stream (no host round trip between the two)
      hipError_t e = trace ? hipEventSynchronize(sg.ev_done) : hipSuccess;
      if (trace) tr[6 * k + 4] = ms_now();
      if (e == hipSuccess) e = hipStreamWaitEvent(lib->s_d2h, sg.ev_done, 0);
      if (e == hipSuccess)
        e = f32 ? hipMemcpyAsync(reinterpret_cast<hfcl_result_f32*>(out) + lo, sg.d_out, m * sizeof(hfcl_result_f32), hipMemcpyDeviceToHost, lib->s_d2h)
                : hipMemcpyAsync(out + lo, sg.d_out, m * sizeof(hfcl_result), hipMemcpyDeviceToHost, lib->s_d2h);
      if (e == hipSuccess && gout) e = hipMemcpyAsync(gout + lo, sg.d_gout, m * sizeof(hfcl_guess), hipMemcpyDeviceToHost, lib->s_d2h);
      if (e == hipSuccess) e = hipStreamSynchronize(lib->s_d2h);  // (ev_done has passed: the counters are on the host too)
      if (e == hipSuccess)
        for (int i = 0; i < N_COUNTERS; ++i) lib->acc_counts[i] += sg.h_counts[i] + (sg.split ? sg.h_counts2[i] : 0u);
      if (e != hipSuccess) {
        side_fail("drain", e);
        return;
      }
      if (trace) tr[6 * k + 5] = ms_now();
      std::lock_guard<std::mutex> lk(mu);
      drained = k + 1;
      cv.notify_all();
    }
  };
  const bool threaded = n_chunks > 1;
  std::thread feeder, feeder2, drainer;
  if (threaded) {
    feeder = std::thread(feed, 0);
    feeder2 = std::thread(feed, 1);
    drainer = std::thread(drain);
  }

  auto fail = [&](int code) {  // stop the pipeline and leave
    {
      std::lock_guard<std::mutex> lk(mu);
      abort_all = true;
    }
    cv.notify_all();
    if (threaded) {
      feeder.join();
      feeder2.join();
      drainer.join();
    }
    hipStreamSynchronize(lib->s_h2d);
    hipStreamSynchronize(lib->s_h2d2);
    hipStreamSynchronize(lib->s_cmp);
    hipStreamSynchronize(lib->s_d2h);
    return code;
  };
#define PIPE_TRY(expr)                                                       \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));          \
      return fail(HFCL_ERR_HIP);                                             \
    }                                                                        \
  } while (0)

  if (!threaded) {
    feed(0);
    feed(1);
  }
  for (size_t k = 0; k < n_chunks; ++k) {
    hfcl_lib::Staging& sg = lib->stage[k % S];
    const size_t m = bounds[k + 1] - bounds[k];
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return (copied[0] > k && copied[1] > k) || abort_all; });
      if (side_rc) {
        lk.unlock();
        set_error(side_err);
        return fail(side_rc);
      }
    }
    if (trace) tr[6 * k + 2] = ms_now();
    PIPE_TRY(hipStreamWaitEvent(lib->s_cmp, sg.ev_in, 0));
    PIPE_TRY(hipStreamWaitEvent(lib->s_cmp, sg.ev_in2, 0));
    if (compact) {
      launch_expand_poses(lib->s_cmp, sg.d_qt1, sg.d_tf1, uint32_t(m));
      launch_expand_poses(lib->s_cmp, sg.d_qt2, sg.d_tf2, uint32_t(m));
    }
    memset(sg.h_counts, 0, N_COUNTERS * sizeof(uint32_t));  // (a skipped batch -- -inf margin -- copies no counters)
    memset(sg.h_counts2, 0, N_COUNTERS * sizeof(uint32_t));
    lib->counts_dst = sg.h_counts;
    if (batch_splits(lib, m)) {
      rc = ensure_helper(lib);
      if (rc) return fail(rc);
      lib->helper->counts_dst = sg.h_counts2;
    }
    if (f32 && creq)
      rc = hfcl_collide_batch_device_f32(lib, sg.d_s1, sg.d_s2, reinterpret_cast<const float*>(sg.d_tf1.get()), reinterpret_cast<const float*>(sg.d_tf2.get()), m, creq,
                                         reinterpret_cast<hfcl_result_f32*>(sg.d_out.get()), lib->s_cmp);
    else if (f32)
      rc = hfcl_distance_batch_device_f32(lib, sg.d_s1, sg.d_s2, reinterpret_cast<const float*>(sg.d_tf1.get()), reinterpret_cast<const float*>(sg.d_tf2.get()), m, dreq,
                                          reinterpret_cast<hfcl_result_f32*>(sg.d_out.get()), lib->s_cmp);
    else if (creq)
      rc = hfcl_collide_batch_device(lib, sg.d_s1, sg.d_s2, sg.d_tf1, sg.d_tf2, m, creq, sg.d_out, gin ? sg.d_gin : nullptr,
                                     gout ? sg.d_gout : nullptr, lib->s_cmp);
    else
      rc = hfcl_distance_batch_device(lib, sg.d_s1, sg.d_s2, sg.d_tf1, sg.d_tf2, m, dreq, sg.d_out, gin ? sg.d_gin : nullptr,
                                      gout ? sg.d_gout : nullptr, lib->s_cmp);
    if (rc) return fail(rc);
    sg.split = lib->last_split;
    PIPE_TRY(hipEventRecord(sg.ev_done, lib->s_cmp));
    if (trace) tr[6 * k + 3] = ms_now();
    {
      std::lock_guard<std::mutex> lk(mu);
      issued = k + 1;
    }
    cv.notify_all();
    if (!threaded) drain();
  }
#undef PIPE_TRY
  if (threaded) {
    feeder.join();
    feeder2.join();
    drainer.join();
  }
  if (trace) {
    fprintf(stderr, "[hfcl pipe] %zu pairs, %zu chunks, %.3f ms\n", n, n_chunks, ms_now());
    for (size_t k = 0; k < n_chunks; ++k)
      fprintf(stderr, "[hfcl pipe] chunk %2zu %7zu pairs: copy-in issued %.3f..%.3f  launches %.3f..%.3f  kernels done %.3f  records out %.3f\n", k,
              bounds[k + 1] - bounds[k], tr[6 * k], tr[6 * k + 1], tr[6 * k + 2], tr[6 * k + 3], tr[6 * k + 4], tr[6 * k + 5]);
  }
  lib->last_host = true;
  if (side_rc) {
    set_error(side_err);
    return side_rc;
  }
  return host_batch_checks(lib, creq, dreq);
}

int hfcl_collide_batch(hfcl_lib* lib, const uint32_t* shape1, const uint32_t* shape2, const double* tf1,
                       const double* tf2, size_t n, const hfcl_collision_request* req, hfcl_result* out,
                       const hfcl_guess* guess_in, hfcl_guess* guess_out) {
  if (!req) {
    set_error("null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return host_batch(lib, shape1, shape2, tf1, tf2, n, req, nullptr, out, guess_in, guess_out);
}
int hfcl_distance_batch(hfcl_lib* lib, const uint32_t* shape1, const uint32_t* shape2, const double* tf1,
                        const double* tf2, size_t n, const hfcl_distance_request* req, hfcl_result* out,
                        const hfcl_guess* guess_in, hfcl_guess* guess_out) {
  if (!req) {
    set_error("null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return host_batch(lib, shape1, shape2, tf1, tf2, n, nullptr, req, out, guess_in, guess_out);
}

int hfcl_collide_batch_f32(hfcl_lib* lib, const uint32_t* shape1, const uint32_t* shape2, const float* pose1, const float* pose2, size_t n,
                           const hfcl_collision_request* req, hfcl_result_f32* out) {
  if (!req) {
    set_error("null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return host_batch(lib, shape1, shape2, reinterpret_cast<const double*>(pose1), reinterpret_cast<const double*>(pose2), n, req, nullptr,
                    reinterpret_cast<hfcl_result*>(out), nullptr, nullptr, true, false, true);
}
int hfcl_distance_batch_f32(hfcl_lib* lib, const uint32_t* shape1, const uint32_t* shape2, const float* pose1, const float* pose2, size_t n,
                            const hfcl_distance_request* req, hfcl_result_f32* out) {
  if (!req) {
    set_error("null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return host_batch(lib, shape1, shape2, reinterpret_cast<const double*>(pose1), reinterpret_cast<const double*>(pose2), n, nullptr, req,
                    reinterpret_cast<hfcl_result*>(out), nullptr, nullptr, true, false, true);
}

int hfcl_collide_batch_qt(hfcl_lib* lib, const uint32_t* shape1, const uint32_t* shape2, const double* pose1,
                          const double* pose2, size_t n, const hfcl_collision_request* req, hfcl_result* out,
                          const hfcl_guess* guess_in, hfcl_guess* guess_out) {
  if (!req) {
    set_error("null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return host_batch(lib, shape1, shape2, pose1, pose2, n, req, nullptr, out, guess_in, guess_out, true, true);
}
int hfcl_distance_batch_qt(hfcl_lib* lib, const uint32_t* shape1, const uint32_t* shape2, const double* pose1,
                           const double* pose2, size_t n, const hfcl_distance_request* req, hfcl_result* out,
                           const hfcl_guess* guess_in, hfcl_guess* guess_out) {
  if (!req) {
    set_error("null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return host_batch(lib, shape1, shape2, pose1, pose2, n, nullptr, req, out, guess_in, guess_out, true, true);
}

int hfcl_collide_batch_contacts(hfcl_lib* lib, const uint32_t* shape1, const uint32_t* shape2, const double* tf1,
                                const double* tf2, size_t n, const hfcl_collision_request* req, hfcl_result* out,
                                hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out) {
  if (!lib || !req || !contacts || !n_contacts_out) {
    set_error("null argument");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(lib->device));
  HIP_TRY(lib->d_contacts.grow(max_contacts_total));
  HIP_TRY(lib->d_contacts_count.grow(1));
  HIP_TRY(hipMemset(lib->d_contacts_count, 0, sizeof(uint32_t)));
  lib->bvh_params.contacts = lib->d_contacts;
  lib->bvh_params.contacts_cap = uint32_t(max_contacts_total > 0xFFFFFFFFull ? 0xFFFFFFFFull : max_contacts_total);
  lib->bvh_params.contacts_count = lib->d_contacts_count;
  int rc = host_batch(lib, shape1, shape2, tf1, tf2, n, req, nullptr, out, nullptr, nullptr, /*pipelined=*/false);
  lib->bvh_params.contacts = nullptr;
  lib->bvh_params.contacts_cap = 0;
  lib->bvh_params.contacts_count = nullptr;
  if (rc) return rc;
  uint32_t cnt = 0;
  HIP_TRY(hipMemcpy(&cnt, lib->d_contacts_count, sizeof(uint32_t), hipMemcpyDeviceToHost));
  const size_t stored = cnt < max_contacts_total ? cnt : max_contacts_total;
  if (stored) HIP_TRY(hipMemcpy(contacts, lib->d_contacts, stored * sizeof(hfcl_contact), hipMemcpyDeviceToHost));
  *n_contacts_out = cnt;  // number produced (may exceed the capacity; the excess was dropped)
  return HFCL_OK;
}

double hfcl_last_kernel_ms(hfcl_lib* lib) {
  if (!lib) return 0.0;
  hipSetDevice(lib->device);
  double total = 0, best = -1;
  lib->dominant = "";
  for (auto& t : lib->timers) {
    if (!t.used) continue;
    if (hipEventSynchronize(t.e1) != hipSuccess) continue;
    float ms = 0;
    if (hipEventElapsedTime(&ms, t.e0, t.e1) != hipSuccess) continue;
    total += ms;
    if (ms > best) {
      best = ms;
      lib->dominant = t.name;
    }
  }
  return total;
}
const char* hfcl_last_kernel_name(hfcl_lib* lib) { return lib ? lib->dominant.c_str() : ""; }
void hfcl_lib_set_kernel_timing(hfcl_lib* lib, int on) {
  if (!lib) return;
  lib->kernel_timing = on != 0;
  if (!on)
    for (auto& t : lib->timers) t.used = false;
}

// breakdown: up to `cap` (name, ms) entries of the last call; returns the number written
int hfcl_last_kernel_breakdown(hfcl_lib* lib, const char** names, double* ms, int cap) {
  if (!lib) return 0;
  hipSetDevice(lib->device);
  int k = 0;
  for (auto& t : lib->timers) {
    if (!t.used || k >= cap) continue;
    float m = 0;
    if (hipEventSynchronize(t.e1) != hipSuccess) continue;
    if (hipEventElapsedTime(&m, t.e0, t.e1) != hipSuccess) continue;
    // split batch: the two halves ran the same launch sequence on two streams; report the mean as-run duration of a launch
    const size_t i = size_t(&t - lib->timers.data());
    if (lib->last_split && lib->helper && i < lib->helper->timers.size() && lib->helper->timers[i].used) {
      KernelTime& u = lib->helper->timers[i];
      float m2 = 0;
      if (hipEventSynchronize(u.e1) == hipSuccess && hipEventElapsedTime(&m2, u.e0, u.e1) == hipSuccess) m = 0.5f * (m + m2);
    }
    names[k] = t.name;
    ms[k] = m;
    ++k;
  }
  return k;
}

// parts = 2: batches of at least 128k pairs (libraries without meshes) run as two halves on two streams; 1: one stream
void hfcl_lib_set_split(hfcl_lib* lib, int parts) {
  if (lib) lib->opt.split = parts >= 2 ? 2 : (parts == 1 ? 1 : 0);
}
int hfcl_lib_get_split(const hfcl_lib* lib) { return lib ? lib->opt.split : 0; }
// (diagnostic, not part of the ABI: the counters of the last batch's walk rounds -- WalkArgs::ctr, 8 words per round -- of the mesh x mesh (solid = 0) or the
// mesh x solid walks, and BVH_CTR_TASKS / BVH_CTR_SUSPENDED of their split tables behind them: tools/dbg/walk_counters.py)
extern "C" int hfcl_debug_walk_counters(hfcl_lib* lib, int solid, uint32_t* out34) {
  if (!lib || !out34) return HFCL_ERR_INVALID_ARGUMENT;
  if (hipSetDevice(lib->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return HFCL_ERR_HIP;
  memset(out34, 0, 34 * sizeof(uint32_t));
  const uint32_t* src = solid ? lib->walk_ms.ctr : lib->walk_mm.ctr;
  if (src && hipMemcpy(out34, src, 8 * WALK_ROUNDS * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return HFCL_ERR_HIP;
  uint32_t ctr[BVH_CTR_WORDS] = {0};
  // (a mixed batch run beside walks its mesh x mesh pairs on the second set of tables; otherwise the kind walked last owns the first)
  const uint32_t* bsrc = (!solid && lib->split_beside.ctr) ? lib->split_beside.ctr : lib->split_main.ctr;
  if (bsrc && hipMemcpy(ctr, bsrc, sizeof(ctr), hipMemcpyDeviceToHost) != hipSuccess) return HFCL_ERR_HIP;
  out34[32] = ctr[BVH_CTR_TASKS];
  out34[33] = ctr[BVH_CTR_SUSPENDED];
  return HFCL_OK;
}
// (diagnostic, not part of the ABI: the owning handles alive in this process -- device buffers, pinned buffers, streams, events; hfcl_own.hpp.
// What a library, a scene or a multi-device set took is given back when it is destroyed: tests/test_gpu_ownership.py)
extern "C" void hfcl_debug_live_handles(int64_t* out4) {
  for (int k = 0; k < 4; ++k) out4[k] = g_hfcl_live[k].load(std::memory_order_relaxed);
}
// (diagnostic, not part of the ABI: what the host entry point and the dispatcher chose for the last call -- "name=value;" per decision, note_form;
// a split batch: the first half's.  Empty unless hfcl_debug_note_forms(lib, 1) was called before the batch.  Valid until the library's next call: tests/test_options_gpu.py takes the forms' witnesses from it)
extern "C" void hfcl_debug_note_forms(hfcl_lib* lib, int on) {
  if (lib) lib->note_forms = on != 0;
  if (lib && lib->helper) lib->helper->note_forms = on != 0;
}
extern "C" const char* hfcl_debug_last_forms(hfcl_lib* lib) {
  if (!lib) return "";
  lib->notes_out = lib->host_notes + lib->form_notes;
  return lib->notes_out.c_str();
}
// (diagnostic, not part of the ABI: the bytes of the library's options block, hfcl_options, so that a test can show that a refused
// hfcl_lib_set_option left every option as it was; returns the block's size, copies min(cap, size) bytes: tests/test_options_gpu.py)
extern "C" size_t hfcl_debug_options_block(const hfcl_lib* lib, void* out, size_t cap) {
  if (lib && out) memcpy(out, &lib->opt, std::min(cap, sizeof(hfcl_options)));
  return sizeof(hfcl_options);
}
// pairs per chunk of the host-buffer pipeline (0 = automatic: n/8 clamped to 32k .. 256k)
void hfcl_lib_set_host_chunk(hfcl_lib* lib, size_t pairs) {
  if (lib) lib->opt.pipe_chunk = pairs;
}
// Options by name (the list: option_keys above; INTEGRATION.md describes them).  Keys are case-insensitive, an "HFCL_" prefix -- the
// spelling of the environment fallback -- is accepted.  Holds from the next batch on; the caller does not call it while a batch of this
// library is being set up on another thread (the library has no lock of its own, like every other hfcl_lib_set_*).
int hfcl_lib_set_option(hfcl_lib* lib, const char* key, const char* value) {
  if (!lib || !key || !value) {
    set_error("hfcl_lib_set_option: null argument");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  std::string k;
  for (const char* c = key; *c; ++c) k.push_back(char(tolower(static_cast<unsigned char>(*c))));
  if (k.compare(0, 5, "hfcl_") == 0) k.erase(0, 5);
  const int rc = apply_option(lib, k, value);
  if (rc != HFCL_OK) {
    set_error("hfcl_lib_set_option: unknown option or value out of range: " + std::string(key) + "=" + value);
    return rc;
  }
  // buffers sized by an option are sized again by the next batch
  if (k == "epa_resume_slots") lib->epa_capacity = 0;
  if (k == "bvh_task_slots") lib->split_main.n = 0;
  return HFCL_OK;
}
// The option names, one per call: index 0, 1, ... until nullptr.
const char* hfcl_lib_option_key(int index) {
  if (index < 0) return nullptr;
  const char* const* k = option_keys();
  for (int i = 0; k[i]; ++i)
    if (i == index) return k[i];
  return nullptr;
}
int hfcl_lib_last_split_parts(const hfcl_lib* lib) { return (lib && lib->last_split) ? 2 : 1; }

// bucket populations of the last call (after a stream sync): closed, prim, cc, pc, cp, bvh, unsupported,
// epa queue, epa overflow queue
void hfcl_last_bucket_counts(hfcl_lib* lib, uint32_t* out12) {  // B_COUNT buckets + the two EPA queues
  if (lib) {  // the counters travel with an asynchronous copy at the end of the batch: wait for it
    hipSetDevice(lib->device);
    hipDeviceSynchronize();
  }
  for (int i = 0; i <= B_COUNT + 1; ++i) out12[i] = lib ? total_count(lib, i) : 0;
}

// Pairs of the last fp32 call whose fp32 run was inconsistent and which the batch solved again in fp64 (CTR_REDO; k_redo).  Waits for the
// device like hfcl_last_bucket_counts.
uint32_t hfcl_last_redo_count(hfcl_lib* lib) {
  if (!lib) return 0;
  hipSetDevice(lib->device);
  hipDeviceSynchronize();
  if (lib->last_host) return lib->acc_counts[CTR_REDO];
  uint32_t c = lib->h_counts ? lib->h_counts[CTR_REDO] : 0u;
  if (lib->last_split && lib->helper && lib->helper->h_counts) c += lib->helper->h_counts[CTR_REDO];
  return c;
}

// Walks of the last distance() batch that the pooled continuations walked again in the reference's order (BvhSpill::rerun_count): out4 = mesh x mesh
// walks continued by waves, of those re-run in order; the same two for mesh x solid.  Waits for the device like hfcl_last_bucket_counts.
void hfcl_last_ordered_reruns(hfcl_lib* lib, uint32_t* out4) {
  static const int idx[4] = {CTR_DIST_SUSP, CTR_DIST_RERUN, CTR_SHAPE_DIST_SUSP, CTR_SHAPE_DIST_RERUN};
  if (lib) {
    hipSetDevice(lib->device);
    hipDeviceSynchronize();
  }
  for (int k = 0; k < 4; ++k) {
    uint32_t c = 0;
    if (lib) {
      if (lib->last_host)
        c = lib->acc_counts[idx[k]];
      else {
        c = lib->h_counts ? lib->h_counts[idx[k]] : 0u;
        if (lib->last_split && lib->helper && lib->helper->h_counts) c += lib->helper->h_counts[idx[k]];
      }
    }
    out4[k] = c;
  }
}

// Convex x convex polytopes of the last fp32 call that outgrew k_epa_loop's block and were handed to k_epa_resume_cc (or, past the
// hand-over area, to the full-capacity tier): CTR_EPA_CC_OVER.  Waits for the device like hfcl_last_bucket_counts.
uint32_t hfcl_last_epa_handed_over(hfcl_lib* lib) {
  if (!lib) return 0;
  hipSetDevice(lib->device);
  hipDeviceSynchronize();
  if (lib->last_host) return lib->acc_counts[CTR_EPA_CC_OVER];
  uint32_t c = lib->h_counts ? lib->h_counts[CTR_EPA_CC_OVER] : 0u;
  if (lib->last_split && lib->helper && lib->helper->h_counts) c += lib->helper->h_counts[CTR_EPA_CC_OVER];
  return c;
}

}  // extern "C"
