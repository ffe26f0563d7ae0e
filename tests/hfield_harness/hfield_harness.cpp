// TEST INFRASTRUCTURE: host build of the height-field device header (hpp-fcl_amd/csrc/hfcl_hfield.hpp) with g++, built by
// tests/test_hfield_cpu.py / tests/test_hfield_gpu.py into a temporary directory.  hh_collide runs the queries one after the other
// in the steps the kernels of hfcl_k_hfield.hip take: the solid's world box, the walk that lists the leaves, every listed leaf
// through the per-pair solver on one lane (SerialGroup<1>), the fold, the contacts.  Not a fallback: the product library neither
// links nor loads this file.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_hfield.hpp"

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

// field_table: 7 words a field (node_off, height_off, xg_off, yg_off, n_nodes, nx, ny); heights: clamped.  items_out (optional): the
// listed leaves of every query, 2 words an item (query, node), at most items_cap; n_items_out: how many were listed
extern "C" int hh_collide(const hfcl_shape* shapes, uint32_t n_shapes, const double* verts, uint32_t n_fields, const uint64_t* field_table,
                          const double* min_heights, const hfcl_hfield_node* nodes, const double* heights, const double* xgrid,
                          const double* ygrid, const uint32_t* hfield, const uint32_t* shape, const double* tfh_rows, const double* tfs_rows,
                          size_t n, const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out, double* dlb,
                          hfcl_contact* contacts, size_t contacts_cap, size_t* n_contacts, uint32_t* items_out, size_t items_cap,
                          size_t* n_items_out) {
  QParams<double> q;
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
  q.guess[0] = 1; q.guess[1] = 0; q.guess[2] = 0;
  q = hf_leaf_params(q);
  const bool skip_all = req->security_margin == -__builtin_inf();
  const double bd2 = req->break_distance * req->break_distance;
  static thread_local EpaScratch<double, EPA_MAX_ITER> scratch;
  size_t nc_total = 0, ni_total = 0;
  std::vector<HfItem<double>> items;
  std::vector<HfLeafOut<double>> leaves;
  for (size_t i = 0; i < n; ++i) {
    const bool sw = swapped && swapped[i];
    if (skip_all || hfield[i] >= n_fields || shape[i] >= n_shapes || !hf_kind_supported(shapes[shape[i]].type)) {
      hf_skipped_record(&out[i], dlb ? &dlb[i] : nullptr, sw);
      continue;
    }
    const uint64_t* ft = field_table + 7 * size_t(hfield[i]);
    const hfcl_hfield_node* fn = nodes + ft[0];
    const DShape<double> s = dshape(shapes[shape[i]]);
    const Pose<double> tfh = pose_from_abi<double>(tfh_rows + 12 * i), tfs = pose_from_abi<double>(tfs_rows + 12 * i);
    V3<double> blo, bhi;
    hf_solid_world_box(s, verts, tfs, blo, bhi);
    uint32_t stack[HF_STACK];
    bool overflow;
    items.clear();
    const double total = hf_walk(fn, uint32_t(ft[4]), tfh, blo, bhi, q.security_margin, bd2, stack, 1,
                                 [&](uint32_t node, double box_min) {
                                   HfItem<double> it;
                                   it.node = node;
                                   it.query = uint32_t(i);
                                   it.box_min = box_min;
                                   items.push_back(it);
                                 },
                                 overflow);
    if (overflow) return 1;
    HostSolid solid{s, verts};
    HfSweptSupport<double, HostSolid> ssup;
    ssup.s = s;
    ssup.solid = &solid;
    leaves.resize(items.size());
    for (size_t k = 0; k < items.size(); ++k) {
      HfPrisms<double> P;
      hf_leaf<double, SerialGroup<1>>(fn[items[k].node], heights + ft[1], uint32_t(ft[5]), xgrid + ft[2], ygrid + ft[3],
                                       min_heights[hfield[i]], tfh, tfs, solid, ssup, s.kind == K_CONVEX, swept_radius(s), q, &scratch, P,
                                       leaves[k]);
      if (items_out && ni_total + k < items_cap) {
        items_out[2 * (ni_total + k)] = uint32_t(i);
        items_out[2 * (ni_total + k) + 1] = items[k].node;
      }
    }
    ni_total += items.size();
    const size_t at = nc_total;
    nc_total += hf_fold(items.data(), leaves.data(), items.size(), total, q.security_margin, q.collision_distance_threshold, req->num_max_contacts,
                        sw,
                        [&](uint32_t k, uint32_t node, const HfLeafOut<double>& lf) {
                          if (contacts && at + k < contacts_cap) hf_fill_contact(contacts[at + k], uint32_t(i), node, lf, sw);
                        },
                        &out[i], dlb ? &dlb[i] : nullptr);
  }
  if (n_contacts) *n_contacts = nc_total;
  if (n_items_out) *n_items_out = ni_total;
  return 0;
}

// one leaf as the harness solves it, for the comparison with the model: out11 = distance, c1, c2, normal, addable
extern "C" int hh_leaf(const hfcl_shape* shape, const double* verts, const hfcl_hfield_node* node, const double* heights, uint32_t nx,
                       const double* xgrid, const double* ygrid, double min_height, const double* tfh_row, const double* tfs_row,
                       const hfcl_collision_request* req, double* out11) {
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
  q = hf_leaf_params(q);
  static thread_local EpaScratch<double, EPA_MAX_ITER> scratch;
  const DShape<double> s = dshape(*shape);
  HostSolid solid{s, verts};
  HfSweptSupport<double, HostSolid> ssup;
  ssup.s = s;
  ssup.solid = &solid;
  HfPrisms<double> P;
  HfLeafOut<double> lf;
  hf_leaf<double, SerialGroup<1>>(*node, heights, nx, xgrid, ygrid, min_height, pose_from_abi<double>(tfh_row), pose_from_abi<double>(tfs_row), solid,
                                   ssup, s.kind == K_CONVEX, swept_radius(s), q, &scratch, P, lf);
  out11[0] = lf.distance;
  out11[1] = lf.c1.x; out11[2] = lf.c1.y; out11[3] = lf.c1.z;
  out11[4] = lf.c2.x; out11[5] = lf.c2.y; out11[6] = lf.c2.z;
  out11[7] = lf.normal.x; out11[8] = lf.normal.y; out11[9] = lf.normal.z;
  out11[10] = double(lf.addable);
  return 0;
}
