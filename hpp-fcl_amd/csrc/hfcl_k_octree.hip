// hfcl_k_octree.hip -- OcTree x convex solid collide() on the device (hfcl_octree_collide_batch*; the arithmetic: hfcl_octree.hpp).
// Built without contraction (FLAGS_k_octree): the records are the bits of the header's host build (tests/octree_harness).
// The kernels are the listed-leaf pipeline's (hfcl_listed.hpp: k_listed_walk<EMIT>, k_listed_leaf, k_listed_fold<CONTACTS>; its scan,
// k_hf_scan, is defined in hfcl_k_hfield.hip) for OctKind, which plugs in:
//   the walk   the solid's OBB from the library's local boxes, its products with the tree's pose once, then the depth-first walk of the
//              node array (stack in LDS, a column per lane: node, next child and the box of each level of the path); an item is the
//              leaf's node, its box and the running minimum of the box bounds
//   the leaf   the leaf's Box and pose against the solid -- the closed form for a Sphere, else GJK / EPA
//   the fold   oct_fold, oct_fill_contact, oct_skipped_record
// Every loop is bounded by what its comment names: a tree's node count, OCT_STACK, a hull's vertices, gjk_max_iterations /
// epa_max_iterations (hfcl_gjk.hpp / hfcl_epa.hpp), a query's item count.
#include "hfcl_dev.hpp"
#include "hfcl_octree.hpp"

using namespace hfcl;

struct OctKind {
  using Args = OctArgs;
  using Item = OctItem<double>;
  using Leaf = OctLeafOut<double>;
  static constexpr const char* timer_names[LISTED_TIMED_KERNELS] = {"k_oct_walk<emit>", "k_oct_leaf", "k_oct_fold", "k_hf_scan<contacts>",
                                                                    "k_oct_fold<contacts>"};
  // a query the kernels evaluate: ids inside the tables, a solid with an evaluator, not skipped by the request
  static __device__ __forceinline__ bool valid(const Args& a, uint32_t i) {
    if (a.skip_all) return false;
    const uint32_t t = a.octree[i], s = a.shape[i];
    if (t >= a.n_trees || s >= a.n_shapes) return false;
    return oct_kind_supported(a.shapes[s].kind);
  }
  template <class Emit>
  static __device__ __forceinline__ double walk(const Args& a, uint32_t i, Emit emit) {
    __shared__ uint32_t st_node[OCT_STACK][64];
    __shared__ uint32_t st_next[OCT_STACK][64];
    __shared__ double st_box[6 * OCT_STACK][64];
    const DOctree tr = a.trees[a.octree[i]];
    const Pose<double> tft = load_pose(a.tf_c, i), tfs = load_pose(a.tf_s, i);
    const OctQuery<double> oq = oct_make_query(tft, tfs, a.local_boxes + 6 * size_t(a.shape[i]));
    bool overflow;
    return oct_walk(a.nodes + tr.node_off, tr, tft, oq, a.q.security_margin, a.bd2, &st_node[0][threadIdx.x], &st_next[0][threadIdx.x],
                    &st_box[0][threadIdx.x], 64,
                    [&](uint32_t node, const V3<double>& lo, const V3<double>& hi, double box_min) {
                      emit([&](Item& it) {
                        it.node = node;
                        it.lo[0] = lo.x; it.lo[1] = lo.y; it.lo[2] = lo.z;
                        it.hi[0] = hi.x; it.hi[1] = hi.y; it.hi[2] = hi.z;
                        it.box_min = box_min;
                      });
                    },
                    overflow);
  }
  static __device__ __forceinline__ void leaf(const Args& a, const Item& item, const GroupSolid& solid, EpaScratch<double, EPA_MAX_ITER>* scratch,
                                              int, Leaf& out) {
    const Pose<double> tft = load_pose(a.tf_c, item.query), tfs = load_pose(a.tf_s, item.query);
    oct_leaf<double, LaneGroup<BS_W>>(mk<double>(item.lo[0], item.lo[1], item.lo[2]), mk<double>(item.hi[0], item.hi[1], item.hi[2]), tft, solid.s,
                                      a.verts, tfs, solid, a.q, scratch, out);
  }
  template <class OnContact>
  static __device__ __forceinline__ uint32_t fold(const Args& a, uint64_t begin, uint64_t n_items, uint32_t i, bool swapped, OnContact on_contact,
                                                  hfcl_result* rec, double* dlb_out) {
    return oct_fold(a.items + begin, a.leaves + begin, n_items, a.box_total[i], a.q.security_margin, a.q.collision_distance_threshold,
                    a.num_max_contacts, swapped, on_contact, rec, dlb_out);
  }
  static __device__ __forceinline__ void fill_contact(hfcl_contact& c, uint32_t pair, uint32_t node, const Leaf& lf, bool) {
    oct_fill_contact(c, pair, node, lf);
  }
  static __device__ __forceinline__ void skipped_record(hfcl_result* rec, double* dlb_out, bool swapped) { oct_skipped_record(rec, dlb_out, swapped); }
};

void launch_oct_count(hipStream_t st, const OctArgs& a) { launch_listed_count<OctKind>(st, a); }
void launch_oct_solve(hipStream_t st, const OctArgs& a, int max_blocks, bool want_contacts, const char** names, hipEvent_t* e0, hipEvent_t* e1) {
  launch_listed_solve<OctKind>(st, a, max_blocks, want_contacts, names, e0, e1);
}
