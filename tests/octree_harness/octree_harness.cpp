// TEST INFRASTRUCTURE: host build of the octree device header (hpp-fcl_amd/csrc/hfcl_octree.hpp) with g++, built by
// tests/test_octree_cpu.py / tests/test_octree_gpu.py into a temporary directory.  oh_collide runs the queries one after the other in
// the steps the kernels of hfcl_k_octree.hip take: the solid's OBB from its local box, the walk that lists the leaves with their boxes,
// every listed leaf through the per-pair solver on one lane (SerialGroup<1>), the fold, the contacts.  Not a fallback: the product
// library neither links nor loads this file.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_cull.hpp"
#include "../../hpp-fcl_amd/csrc/hfcl_octree.hpp"

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
// free_threshold).  items_out (optional): the listed leaves of every query, 2 words an item (query, node), at most items_cap;
// n_items_out: how many were listed
extern "C" int oh_collide(const hfcl_shape* shapes, uint32_t n_shapes, const double* verts, uint32_t n_trees, const uint64_t* tree_table,
                          const double* tree_params, const hfcl_octree_node* nodes, const uint32_t* octree, const uint32_t* shape,
                          const double* tft_rows, const double* tfs_rows, size_t n, const uint8_t* swapped, const hfcl_collision_request* req,
                          hfcl_result* out, double* dlb, hfcl_contact* contacts, size_t contacts_cap, size_t* n_contacts, uint32_t* items_out,
                          size_t items_cap, size_t* n_items_out) {
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
  static thread_local EpaScratch<double, EPA_MAX_ITER> scratch;
  size_t nc_total = 0, ni_total = 0;
  std::vector<OctItem<double>> items;
  std::vector<OctLeafOut<double>> leaves;
  for (size_t i = 0; i < n; ++i) {
    const bool sw = swapped && swapped[i];
    if (skip_all || octree[i] >= n_trees || shape[i] >= n_shapes || !oct_kind_supported(shapes[shape[i]].type)) {
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
    const DShape<double> s = dshape(shapes[shape[i]]);
    const Pose<double> tft = pose_from_abi<double>(tft_rows + 12 * i), tfs = pose_from_abi<double>(tfs_rows + 12 * i);
    const Box3 lb = shape_local_box(shapes[shape[i]], verts);
    const double lb6[6] = {lb.lo[0], lb.lo[1], lb.lo[2], lb.hi[0], lb.hi[1], lb.hi[2]};
    const OctQuery<double> oq = oct_make_query(tft, tfs, lb6);
    uint32_t st_node[OCT_STACK], st_next[OCT_STACK];
    double st_box[6 * OCT_STACK];
    bool overflow;
    items.clear();
    const double total = oct_walk(nodes + tr.node_off, tr, tft, oq, q.security_margin, bd2, st_node, st_next, st_box, 1,
                                  [&](uint32_t node, const V3<double>& lo, const V3<double>& hi, double box_min) {
                                    OctItem<double> it;
                                    it.node = node;
                                    it.query = uint32_t(i);
                                    it.lo[0] = lo.x; it.lo[1] = lo.y; it.lo[2] = lo.z;
                                    it.hi[0] = hi.x; it.hi[1] = hi.y; it.hi[2] = hi.z;
                                    it.box_min = box_min;
                                    items.push_back(it);
                                  },
                                  overflow);
    if (overflow) return 1;
    HostSolid solid{s, verts};
    leaves.resize(items.size());
    for (size_t k = 0; k < items.size(); ++k) {
      const OctItem<double>& it = items[k];
      oct_leaf<double, SerialGroup<1>>(mk<double>(it.lo[0], it.lo[1], it.lo[2]), mk<double>(it.hi[0], it.hi[1], it.hi[2]), tft, s, verts, tfs, solid, q,
                                       &scratch, leaves[k]);
      if (items_out && ni_total + k < items_cap) {
        items_out[2 * (ni_total + k)] = uint32_t(i);
        items_out[2 * (ni_total + k) + 1] = it.node;
      }
    }
    ni_total += items.size();
    const size_t at = nc_total;
    nc_total += oct_fold(items.data(), leaves.data(), items.size(), total, q.security_margin, q.collision_distance_threshold, req->num_max_contacts,
                         sw,
                         [&](uint32_t k, uint32_t node, const OctLeafOut<double>& lf) {
                           if (contacts && at + k < contacts_cap) oct_fill_contact(contacts[at + k], uint32_t(i), node, lf);
                         },
                         &out[i], dlb ? &dlb[i] : nullptr);
  }
  if (n_contacts) *n_contacts = nc_total;
  if (n_items_out) *n_items_out = ni_total;
  return 0;
}
