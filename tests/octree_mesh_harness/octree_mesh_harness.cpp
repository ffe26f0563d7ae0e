// TEST INFRASTRUCTURE: host build of the octree x mesh device header (hpp-fcl_amd/csrc/hfcl_octree_mesh.hpp) with g++, built by
// tests/test_octree_mesh_cpu.py / tests/test_octree_mesh_gpu.py into a temporary directory.  omh_collide runs the queries one after
// the other in the steps the kernels of hfcl_k_octree_mesh.hip take: the dual walk that lists the (leaf, triangle) pairs with their
// boxes, every listed item through the solver on one lane (SerialGroup<1>), the fold, the contacts.  Not a fallback: the product
// library neither links nor loads this file.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_octree_mesh.hpp"

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
extern "C" uint32_t omh_bvh_depth(const hfcl_bvh_node* nodes, size_t n_nodes) {
  return octm_bvh_depth(n_nodes, [&](uint32_t i) { return nodes[i].first_child; });
}
extern "C" uint32_t omh_depth_limit() { return uint32_t(OCTM_MESH_DEPTH); }

// tree_table: 2 words a tree (node_off, n_nodes); tree_params: 4 doubles a tree (resolution, depth, occupancy_threshold,
// free_threshold).  mesh_table: 4 words a mesh (node_off, vert_off, tri_off, n_nodes); mesh[i]: the mesh of query i.  items_out
// (optional): the listed items of every query, 3 words an item (query, node, triangle), at most items_cap; n_items_out: how many were
// listed.  Returns 1 when a walk's stack overflowed, 2 when a named mesh is deeper than the limit (nothing is written)
extern "C" int omh_collide(uint32_t n_trees, const uint64_t* tree_table, const double* tree_params, const hfcl_octree_node* nodes, uint32_t n_meshes,
                           const uint32_t* mesh_table, const hfcl_bvh_node* mnodes_abi, size_t n_mnodes_total, const double* mverts,
                           const uint32_t* mtris, const uint32_t* octree, const uint32_t* mesh, const double* tft_rows, const double* tfm_rows,
                           size_t n, const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out, double* dlb,
                           hfcl_contact* contacts, size_t contacts_cap, size_t* n_contacts, uint32_t* items_out, size_t items_cap,
                           size_t* n_items_out) {
  QParams<double> q;
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
  q.security_margin = req->security_margin;
  q.mode = 1;
  q.compute_penetration = (req->enable_contact || req->security_margin < 0) ? 1 : 0;
  q.guess_mode = HFCL_GUESS_DEFAULT;
  q.guess[0] = 1; q.guess[1] = 0; q.guess[2] = 0;
  const bool skip_all = req->security_margin == -__builtin_inf();
  const double bd2 = req->break_distance * req->break_distance;
  std::vector<DNode<double>> mnodes(n_mnodes_total);
  for (size_t k = 0; k < n_mnodes_total; ++k) mnodes[k] = pack(mnodes_abi[k]);
  for (size_t i = 0; i < n && !skip_all; ++i)
    if (octree[i] < n_trees && mesh[i] < n_meshes) {
      const uint32_t* mt = mesh_table + 4 * size_t(mesh[i]);
      if (omh_bvh_depth(mnodes_abi + mt[0], mt[3]) > uint32_t(OCTM_MESH_DEPTH)) return 2;
    }
  static thread_local EpaScratch<double, EPA_MAX_ITER> scratch;
  size_t nc_total = 0, ni_total = 0;
  std::vector<OctMeshItem<double>> items;
  std::vector<OctMeshLeafOut<double>> leaves;
  for (size_t i = 0; i < n; ++i) {
    const bool sw = swapped && swapped[i];
    if (skip_all || octree[i] >= n_trees || mesh[i] >= n_meshes) {
      oct_skipped_record(&out[i], dlb ? &dlb[i] : nullptr, sw);
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
    uint32_t st_node[OCT_STACK], st_next[OCT_STACK], st_m[OCTM_MESH_STACK];
    uint8_t st_mo[OCTM_MESH_STACK];
    double st_box[6 * OCT_STACK];
    bool overflow;
    items.clear();
    const double total = octm_walk(nodes + tr.node_off, tr, tft, mnodes.data() + mt[0], mt[3], tfm, q.security_margin, bd2, st_node, st_next, st_box, st_m,
                                   st_mo, 1,
                                   [&](uint32_t node, const V3<double>& lo, const V3<double>& hi, uint32_t prim, double box_min) {
                                     OctMeshItem<double> it;
                                     it.node = node;
                                     it.query = uint32_t(i);
                                     it.prim = prim;
                                     it.pad_ = 0;
                                     it.lo[0] = lo.x; it.lo[1] = lo.y; it.lo[2] = lo.z;
                                     it.hi[0] = hi.x; it.hi[1] = hi.y; it.hi[2] = hi.z;
                                     it.box_min = box_min;
                                     items.push_back(it);
                                   },
                                   overflow);
    if (overflow) return 1;
    leaves.resize(items.size());
    for (size_t k = 0; k < items.size(); ++k) {
      const OctMeshItem<double>& it = items[k];
      octm_leaf<double, SerialGroup<1>>(mk<double>(it.lo[0], it.lo[1], it.lo[2]), mk<double>(it.hi[0], it.hi[1], it.hi[2]), tft, mverts + 3 * size_t(mt[1]),
                                        mtris + 3 * (size_t(mt[2]) + it.prim), tfm, q, &scratch, leaves[k]);
      leaves[k].prim = it.prim;
      leaves[k].pad_ = 0;
      if (items_out && ni_total + k < items_cap) {
        items_out[3 * (ni_total + k)] = uint32_t(i);
        items_out[3 * (ni_total + k) + 1] = it.node;
        items_out[3 * (ni_total + k) + 2] = it.prim;
      }
    }
    ni_total += items.size();
    const size_t at = nc_total;
    nc_total += octm_fold(items.data(), leaves.data(), items.size(), total, q.security_margin, q.collision_distance_threshold, req->num_max_contacts,
                          sw,
                          [&](uint32_t k, uint32_t node, const OctMeshLeafOut<double>& lf) {
                            if (contacts && at + k < contacts_cap) octm_fill_contact(contacts[at + k], uint32_t(i), node, lf);
                          },
                          &out[i], dlb ? &dlb[i] : nullptr);
  }
  if (n_contacts) *n_contacts = nc_total;
  if (n_items_out) *n_items_out = ni_total;
  return 0;
}
