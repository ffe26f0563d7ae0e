// TEST INFRASTRUCTURE: host build of the octree x mesh distance header (hpp-fcl_amd/csrc/hfcl_octree_mesh_distance.hpp) with g++, built by
// tests/test_octree_mesh_distance_cpu.py / tests/test_octree_mesh_distance_gpu.py into a temporary directory.  omdh_distance runs the
// queries one after the other through octm_distance_query, the function the kernel of hfcl_k_octree_mesh_distance.hip runs per lane
// group, on one lane (SerialGroup<1>), and lists the pairs it solves in order.  Not a fallback: the product library neither links nor
// loads this file.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_octree_mesh_distance.hpp"

using namespace hfcl;

static DNode<double> pack(const hfcl_bvh_node& n) {
  DNode<double> d;
  d.first_child = n.first_child;
  d.pad_ = 0;
  const double* a = n.obb_axes;  // column-major
  d.axes.r0 = mk<double>(a[0], a[3], a[6]);
  d.axes.r1 = mk<double>(a[1], a[4], a[7]);
  d.axes.r2 = mk<double>(a[2], a[5], a[8]);
  d.To = mk<double>(n.obb_To[0], n.obb_To[1], n.obb_To[2]);
  d.extent = mk<double>(n.obb_extent[0], n.obb_extent[1], n.obb_extent[2]);
  return d;
}

// levels of a BVH (the root is level 1); 0xFFFFFFFF: the links revisit a node
extern "C" uint32_t omdh_bvh_depth(const hfcl_bvh_node* nodes, size_t n_nodes) {
  return octm_bvh_depth(n_nodes, [&](uint32_t i) { return nodes[i].first_child; });
}
extern "C" uint32_t omdh_depth_limit() { return uint32_t(OCTM_MESH_DEPTH); }

struct ListPairs {
  uint32_t query;
  uint32_t* out;
  size_t cap;
  size_t* n;
  void operator()(uint32_t node, uint32_t prim) const {
    if (out && *n < cap) {
      out[3 * *n] = query;
      out[3 * *n + 1] = node;
      out[3 * *n + 2] = prim;
    }
    ++*n;
  }
};

// tree_table: 2 words a tree (node_off, n_nodes); tree_params: 4 doubles a tree (resolution, depth, occupancy_threshold,
// free_threshold).  mesh_table: 4 words a mesh (node_off, vert_off, tri_off, n_nodes); mesh[i]: the mesh of query i.  n_visited
// (optional): pairs solved per query.  pairs_out (optional): the solved pairs of every query in order, 3 words a pair (query, node,
// triangle), at most pairs_cap; n_pairs_out: how many were solved.  Returns 1 when a walk's stack overflowed, 2 when a named mesh is
// deeper than the limit (nothing is written)
extern "C" int omdh_distance(uint32_t n_trees, const uint64_t* tree_table, const double* tree_params, const hfcl_octree_node* nodes, uint32_t n_meshes,
                             const uint32_t* mesh_table, const hfcl_bvh_node* mnodes_abi, size_t n_mnodes_total, const double* mverts,
                             const uint32_t* mtris, const uint32_t* octree, const uint32_t* mesh, const double* tft_rows, const double* tfm_rows,
                             size_t n, const uint8_t* swapped, const hfcl_distance_request* req, hfcl_result* out, uint32_t* n_visited,
                             uint32_t* pairs_out, size_t pairs_cap, size_t* n_pairs_out) {
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
  std::vector<DNode<double>> mnodes(n_mnodes_total);
  for (size_t k = 0; k < n_mnodes_total; ++k) mnodes[k] = pack(mnodes_abi[k]);
  for (size_t i = 0; i < n; ++i)
    if (octree[i] < n_trees && mesh[i] < n_meshes) {
      const uint32_t* mt = mesh_table + 4 * size_t(mesh[i]);
      if (omdh_bvh_depth(mnodes_abi + mt[0], mt[3]) > uint32_t(OCTM_MESH_DEPTH)) return 2;
    }
  static thread_local EpaScratch<double, EPA_MAX_ITER> scratch;
  static thread_local OctMeshDistStack<double> stack;
  size_t n_pairs = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool sw = swapped && swapped[i];
    if (octree[i] >= n_trees || mesh[i] >= n_meshes) {
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
    const uint32_t* mt = mesh_table + 4 * size_t(mesh[i]);
    const Pose<double> tft = pose_from_abi<double>(tft_rows + 12 * i), tfm = pose_from_abi<double>(tfm_rows + 12 * i);
    OctMeshDistResult<double> r;
    bool overflow = false;
    const ListPairs list{uint32_t(i), pairs_out, pairs_cap, &n_pairs};
    octm_distance_query<double, SerialGroup<1>>(nodes + tr.node_off, tr, tft, mnodes.data() + mt[0], mt[3], mverts + 3 * size_t(mt[1]),
                                                mtris + 3 * size_t(mt[2]), tfm, q, &stack, &scratch, r, overflow, list);
    if (overflow) return 1;
    octmd_record(r, sw, &out[i]);
    if (n_visited) n_visited[i] = r.visited;
  }
  if (n_pairs_out) *n_pairs_out = n_pairs;
  return 0;
}
