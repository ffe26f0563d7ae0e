// TEST INFRASTRUCTURE: host build of the octree distance header (hpp-fcl_amd/csrc/hfcl_octree_distance.hpp) with g++, built by
// tests/test_octree_distance_cpu.py / tests/test_octree_distance_gpu.py into a temporary directory.  ohd_distance runs the queries one
// after the other through oct_distance_query, the function the kernel of hfcl_k_octree_distance.hip runs per lane group, on one lane
// (SerialGroup<1>).  Not a fallback: the product library neither links nor loads this file.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_octree_distance.hpp"

using namespace hfcl;

static DShape<double> dshape(const hfcl_shape& s) {
  DShape<double> d;
  d.kind = s.type;
  d.num_points = s.num_points;
  d.vertex_offset = s.vertex_offset;
  d.bvh_index = s.bvh_index;
  d.p0 = s.params[0]; d.p1 = s.params[1]; d.p2 = s.params[2]; d.p3 = s.params[3];
  d.ssr = s.swept_sphere_radius;
  return d;
}

struct HostSolid {
  DShape<double> s;
  const double* verts;
  V3<double> operator()(const V3<double>& d) const {
    SerialSupport<double> ss;
    return ss.one(s, verts + 3 * size_t(s.vertex_offset), d);
  }
};

// tree_table: 2 words a tree (node_off, n_nodes); tree_params: 4 doubles a tree (resolution, depth, occupancy_threshold,
// free_threshold), as oh_collide (tests/octree_harness).  n_visited (optional): leaves solved per query
extern "C" int ohd_distance(const hfcl_shape* shapes, uint32_t n_shapes, const double* verts, uint32_t n_trees, const uint64_t* tree_table,
                            const double* tree_params, const hfcl_octree_node* nodes, const uint32_t* octree, const uint32_t* shape,
                            const double* tft_rows, const double* tfs_rows, size_t n, const uint8_t* swapped, const hfcl_distance_request* req,
                            hfcl_result* out, uint32_t* n_visited) {
  QParams<double> q;  // setup_distance
  std::memset(&q, 0, sizeof(q));
  q.gjk.tolerance = req->q.gjk_tolerance;
  q.gjk.max_iterations = req->q.gjk_max_iterations;
  q.gjk.variant = req->q.gjk_variant;
  q.gjk.crit = req->q.gjk_convergence_criterion;
  q.gjk.crit_type = req->q.gjk_convergence_criterion_type;
  q.gjk.distance_upper_bound = Lim<double>::max();
  q.epa_tolerance = req->q.epa_tolerance;
  q.epa_max_iterations = int(req->q.epa_max_iterations);
  q.collision_distance_threshold = req->q.collision_distance_threshold;
  q.security_margin = 0;
  q.mode = 0;
  q.compute_penetration = req->enable_signed_distance ? 1 : 0;
  q.guess_mode = HFCL_GUESS_DEFAULT;
  q.guess[0] = 1; q.guess[1] = 0; q.guess[2] = 0;
  static thread_local EpaScratch<double, EPA_MAX_ITER> scratch;
  static thread_local OctDistStack<double> stack;
  for (size_t i = 0; i < n; ++i) {
    const bool sw = swapped && swapped[i];
    if (octree[i] >= n_trees || shape[i] >= n_shapes || !oct_kind_supported(shapes[shape[i]].type)) {
      oct_skipped_record(&out[i], nullptr, sw);
      if (n_visited) n_visited[i] = 0;
      continue;
    }
    DOctree tr;
    tr.node_off = tree_table[2 * size_t(octree[i])];
    tr.n_nodes = uint32_t(tree_table[2 * size_t(octree[i]) + 1]);
    const double* tp = tree_params + 4 * size_t(octree[i]);
    tr.resolution = tp[0];
    tr.depth = uint32_t(tp[1]);
    tr.root_half = oct_root_half(tr.depth, tr.resolution);
    tr.occupancy_threshold = tp[2];
    tr.free_threshold = tp[3];
    const DShape<double> s = dshape(shapes[shape[i]]);
    const Pose<double> tft = pose_from_abi<double>(tft_rows + 12 * i), tfs = pose_from_abi<double>(tfs_rows + 12 * i);
    HostSolid solid{s, verts};
    OctDistResult<double> r;
    bool overflow = false;
    oct_distance_query<double, SerialGroup<1>>(nodes + tr.node_off, tr, tft, s, verts, tfs, solid, q, &stack, &scratch, r, overflow);
    if (overflow) return 1;
    oct_dist_record(r, sw, &out[i]);
    if (n_visited) n_visited[i] = r.visited;
  }
  return 0;
}
