// hfcl_k_octree.hip -- OcTree x convex solid collide() on the device (hfcl_octree_collide_batch*; the arithmetic: hfcl_octree.hpp).
// Built without contraction (FLAGS_k_octree): the records are the bits of the header's host build (tests/octree_harness).
//   k_oct_walk<EMIT>     a lane per query of a chunk: the solid's OBB from the library's local boxes, its products with the tree's pose
//                        once, then the depth-first walk of the node array (stack in LDS, a column per lane: node, next child and the
//                        box of each level of the path).  EMIT = false counts the reached leaves; EMIT = true, after the scan, lists
//                        them in walk order with their boxes and the running minimum of the box bounds, and writes the walk's overall
//                        box minimum.  Two walks and a scan (k_hf_scan of hfcl_k_hfield.hip): no atomics.
//   k_oct_leaf           a listed (query, leaf) item per BS_W-lane group: the leaf's Box and pose against the solid -- the closed form for a
//                        Sphere, else GJK / EPA (the group's lanes share a hull's support scan and EPA's face work; the full-capacity
//                        polytope in LDS, as k_hf_leaf)
//   k_oct_fold<CONTACTS> a lane per query: the replay of its items in order.  CONTACTS = false writes the record, the bound and the
//                        query's contact count; CONTACTS = true, after the scan of the counts, writes the contacts at their offsets.
// Every loop is bounded by what its comment names: a tree's node count, OCT_STACK, a hull's vertices, gjk_max_iterations /
// epa_max_iterations (hfcl_gjk.hpp / hfcl_epa.hpp), a query's item count.
#include "hfcl_dev.hpp"
#include "hfcl_octree.hpp"

using namespace hfcl;

// a query the kernels evaluate: ids inside the tables, a solid with an evaluator, not skipped by the request
static __device__ __forceinline__ bool oct_query_valid(const OctArgs& a, uint32_t i) {
  if (a.skip_all) return false;
  const uint32_t t = a.octree[i], s = a.shape[i];
  if (t >= a.n_trees || s >= a.n_shapes) return false;
  return oct_kind_supported(a.shapes[s].kind);
}

template <bool EMIT>
__global__ void __launch_bounds__(64) k_oct_walk(OctArgs a) {
  __shared__ uint32_t st_node[OCT_STACK][64];
  __shared__ uint32_t st_next[OCT_STACK][64];
  __shared__ double st_box[6 * OCT_STACK][64];
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= a.m) return;
  uint32_t cnt = 0;
  double total = Lim<double>::max();
  if (oct_query_valid(a, i)) {
    const DOctree tr = a.trees[a.octree[i]];
    const Pose<double> tft = load_pose(a.tf_t, i), tfs = load_pose(a.tf_s, i);
    const OctQuery<double> oq = oct_make_query(tft, tfs, a.local_boxes + 6 * size_t(a.shape[i]));
    uint64_t pos = EMIT ? a.offsets[i] : 0u;
    const uint64_t end = EMIT ? a.offsets[i + 1u] : 0u;
    bool overflow;
    total = oct_walk(a.nodes + tr.node_off, tr, tft, oq, a.q.security_margin, a.bd2, &st_node[0][threadIdx.x], &st_next[0][threadIdx.x],
                     &st_box[0][threadIdx.x], 64,
                     [&](uint32_t node, const V3<double>& lo, const V3<double>& hi, double box_min) {
                       if (EMIT && pos < end && pos < a.n_items) {  // (the second walk visits what the first one counted)
                         OctItem<double> it;
                         it.node = node;
                         it.query = i;
                         it.lo[0] = lo.x; it.lo[1] = lo.y; it.lo[2] = lo.z;
                         it.hi[0] = hi.x; it.hi[1] = hi.y; it.hi[2] = hi.z;
                         it.box_min = box_min;
                         a.items[pos] = it;
                       }
                       ++pos;
                       ++cnt;
                     },
                     overflow);
  }
  if (EMIT) a.box_total[i] = total;
  else a.counts[i] = cnt;
}

// support of the solid in its own frame, evaluated by the lane group (NoSweptSphere): what k_hf_leaf plugs into the solver
struct OctGroupSolid {
  DShape<double> s;
  HullRegs<double, BS_W> h;
  const double* v;
  int lig;
  __device__ __forceinline__ V3<double> operator()(const V3<double>& d) const {
    if (s.kind != K_CONVEX) return prim_support(s, d);
    if (s.num_points > uint32_t(HULL_MAX)) return scan_support<double, BS_W>(v, s.num_points, d, lig);
    return h.support(d, lig);
  }
};

__global__ void __launch_bounds__(64) k_oct_leaf(OctArgs a) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<double, EPA_MAX_ITER> scratch[G];
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint64_t it = uint64_t(blockIdx.x) * G + grp; it < a.n_items; it += uint64_t(gridDim.x) * G) {
    const OctItem<double> item = a.items[it];
    const uint32_t i = item.query;
    OctGroupSolid solid;
    solid.s = a.shapes[a.shape[i]];
    solid.v = a.verts + 3 * size_t(solid.s.vertex_offset);
    solid.lig = lig;
    if (solid.s.kind == K_CONVEX && solid.s.num_points <= uint32_t(HULL_MAX)) solid.h.load(solid.v, solid.s.num_points, lig);
    const Pose<double> tft = load_pose(a.tf_t, i), tfs = load_pose(a.tf_s, i);
    OctLeafOut<double> out;
    oct_leaf<double, LaneGroup<BS_W>>(mk<double>(item.lo[0], item.lo[1], item.lo[2]), mk<double>(item.hi[0], item.hi[1], item.hi[2]), tft, solid.s,
                                      a.verts, tfs, solid, a.q, &scratch[grp], out);
    if (lig == 0) a.leaves[it] = out;
    LaneGroup<BS_W>::sync();
  }
}

template <bool CONTACTS>
__global__ void __launch_bounds__(256) k_oct_fold(OctArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.m) return;
  const bool swapped = a.swapped && a.swapped[i];
  if (!oct_query_valid(a, i)) {
    if (!CONTACTS) {
      oct_skipped_record(&a.out[i], a.dlb ? &a.dlb[i] : nullptr, swapped);
      if (a.ccounts) a.ccounts[i] = 0u;
    }
    return;
  }
  const uint64_t begin = a.offsets[i], end = a.offsets[i + 1u];
  const uint64_t n_items = end > begin && end <= a.n_items ? end - begin : 0u;
  if (CONTACTS) {
    const uint64_t at = a.coffsets[i];
    oct_fold(a.items + begin, a.leaves + begin, n_items, a.box_total[i], a.q.security_margin, a.q.collision_distance_threshold, a.num_max_contacts,
             swapped,
             [&](uint32_t k, uint32_t node, const OctLeafOut<double>& lf) {
               if (at + k < a.contacts_cap) oct_fill_contact(a.contacts[at + k], a.pair0 + i, node, lf);
             },
             static_cast<hfcl_result*>(nullptr), static_cast<double*>(nullptr));
  } else {
    const uint32_t nc = oct_fold(a.items + begin, a.leaves + begin, n_items, a.box_total[i], a.q.security_margin, a.q.collision_distance_threshold,
                                 a.num_max_contacts, swapped, [](uint32_t, uint32_t, const OctLeafOut<double>&) {}, &a.out[i],
                                 a.dlb ? &a.dlb[i] : nullptr);
    if (a.ccounts) a.ccounts[i] = nc;
  }
}

void launch_oct_count(hipStream_t st, const OctArgs& a) {
  if (!a.m) return;
  hipLaunchKernelGGL(k_oct_walk<false>, dim3((a.m + 63u) / 64u), dim3(64), 0, st, a);
  launch_hf_scan(st, a.counts, a.offsets, a.m, nullptr);
}

void launch_oct_solve(hipStream_t st, const OctArgs& a, int max_blocks, bool want_contacts, const char** names, hipEvent_t* e0, hipEvent_t* e1) {
  static const char* const kn[OCT_TIMED_KERNELS] = {"k_oct_walk<emit>", "k_oct_leaf", "k_oct_fold", "k_hf_scan<contacts>", "k_oct_fold<contacts>"};
  for (int k = 0; k < OCT_TIMED_KERNELS; ++k) names[k] = kn[k];
  if (!a.m) return;
  auto begin = [&](int k) { if (e0) (void)hipEventRecord(e0[k], st); };
  auto end = [&](int k) { if (e1) (void)hipEventRecord(e1[k], st); };
  begin(0);
  hipLaunchKernelGGL(k_oct_walk<true>, dim3((a.m + 63u) / 64u), dim3(64), 0, st, a);
  end(0);
  begin(1);
  if (a.n_items) {
    constexpr uint64_t G = 64 / BS_W;
    const uint32_t grid = uint32_t(std::min<uint64_t>((a.n_items + G - 1u) / G, uint64_t(std::max(max_blocks, 1))));
    hipLaunchKernelGGL(k_oct_leaf, dim3(grid), dim3(64), 0, st, a);
  }
  end(1);
  begin(2);
  hipLaunchKernelGGL(k_oct_fold<false>, dim3((a.m + 255u) / 256u), dim3(256), 0, st, a);
  end(2);
  begin(3);
  if (want_contacts) launch_hf_scan(st, a.ccounts, a.coffsets, a.m, a.running);
  end(3);
  begin(4);
  if (want_contacts && a.contacts) hipLaunchKernelGGL(k_oct_fold<true>, dim3((a.m + 255u) / 256u), dim3(256), 0, st, a);
  end(4);
}
