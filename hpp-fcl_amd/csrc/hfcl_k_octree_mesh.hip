// hfcl_k_octree_mesh.hip -- OcTree x BVHModel<OBBRSS> collide() on the device (hfcl_octree_mesh_collide_batch*; the arithmetic:
// hfcl_octree_mesh.hpp).  Built without contraction (FLAGS_k_octree_mesh): the records are the bits of the header's host build
// (tests/octree_mesh_harness).
// The walk and the fold are the listed-leaf pipeline's kernels (hfcl_listed.hpp: k_listed_walk<EMIT>, k_listed_fold<CONTACTS>; its
// scan, k_hf_scan, is defined in hfcl_k_hfield.hip) for OctMeshKind, which plugs in:
//   the walk   the dual walk of the octree's node array and the mesh's OBB nodes over a path stack in LDS, a column per lane: an
//              octree frame (node, next child, box) per level the octree side descended, a mesh frame (first child, a byte of
//              bookkeeping) per level the mesh side did -- 16 + 64 frames, 76 KB a workgroup of 64 lanes, none of it in scratch;
//              an item is the leaf's node, its box, the triangle and the running minimum of the box bounds
//   the fold   octm_fold, octm_fill_contact, oct_skipped_record
// The leaf kernel is this unit's own: the pipeline's k_listed_leaf loads one solid per QUERY for its group, here the second operand is a
// triangle per ITEM.  A BS_W-lane group per listed item: the Box's support and the triangle moved into the box's frame through the fp64
// GJK / EPA of the per-pair solver, EPA's polytope in LDS.
// Every loop is bounded by what its comment names: the depth of the tree and of the BVH (OCT_STACK, OCTM_MESH_STACK),
// gjk_max_iterations / epa_max_iterations (hfcl_gjk.hpp / hfcl_epa.hpp), a query's item count.
#include "hfcl_dev.hpp"
#include "hfcl_octree_mesh.hpp"

using namespace hfcl;

struct OctMeshKind {
  using Args = OctMeshArgs;
  using Item = OctMeshItem<double>;
  using Leaf = OctMeshLeafOut<double>;
  static constexpr const char* timer_names[LISTED_TIMED_KERNELS] = {"k_octm_walk<emit>", "k_octm_leaf", "k_octm_fold", "k_hf_scan<contacts>",
                                                                    "k_octm_fold<contacts>"};
  // a query the kernels evaluate: ids inside the tables, a shape row that names a registered mesh, not skipped by the request
  static __device__ __forceinline__ bool valid(const Args& a, uint32_t i) {
    if (a.skip_all) return false;
    const uint32_t t = a.octree[i], s = a.shape[i];
    if (t >= a.n_trees || s >= a.n_shapes) return false;
    return a.shapes[s].kind == K_BVH && a.shapes[s].bvh_index < a.n_meshes;
  }
  template <class Emit>
  static __device__ __forceinline__ double walk(const Args& a, uint32_t i, Emit emit) {
    __shared__ uint32_t st_node[OCT_STACK][64];
    __shared__ uint32_t st_next[OCT_STACK][64];
    __shared__ double st_box[6 * OCT_STACK][64];
    __shared__ uint32_t st_m[OCTM_MESH_STACK][64];
    __shared__ uint8_t st_mo[OCTM_MESH_STACK][64];
    const DOctree tr = a.trees[a.octree[i]];
    const DMesh me = a.meshes[a.shapes[a.shape[i]].bvh_index];
    const Pose<double> tft = load_pose(a.tf_c, i), tfm = load_pose(a.tf_s, i);
    bool overflow;
    return octm_walk(a.nodes + tr.node_off, tr, tft, a.mnodes + me.node_off, me.n_nodes, tfm, a.q.security_margin, a.bd2, &st_node[0][threadIdx.x],
                     &st_next[0][threadIdx.x], &st_box[0][threadIdx.x], &st_m[0][threadIdx.x], &st_mo[0][threadIdx.x], 64,
                     [&](uint32_t node, const V3<double>& lo, const V3<double>& hi, uint32_t prim, double box_min) {
                       emit([&](Item& it) {
                         it.node = node;
                         it.prim = prim;
                         it.pad_ = 0u;
                         it.lo[0] = lo.x; it.lo[1] = lo.y; it.lo[2] = lo.z;
                         it.hi[0] = hi.x; it.hi[1] = hi.y; it.hi[2] = hi.z;
                         it.box_min = box_min;
                       });
                     },
                     overflow);
  }
  template <class OnContact>
  static __device__ __forceinline__ uint32_t fold(const Args& a, uint64_t begin, uint64_t n_items, uint32_t i, bool swapped, OnContact on_contact,
                                                  hfcl_result* rec, double* dlb_out) {
    return octm_fold(a.items + begin, a.leaves + begin, n_items, a.box_total[i], a.q.security_margin, a.q.collision_distance_threshold,
                     a.num_max_contacts, swapped, on_contact, rec, dlb_out);
  }
  static __device__ __forceinline__ void fill_contact(hfcl_contact& c, uint32_t pair, uint32_t node, const Leaf& lf, bool) {
    octm_fill_contact(c, pair, node, lf);
  }
  static __device__ __forceinline__ void skipped_record(hfcl_result* rec, double* dlb_out, bool swapped) { oct_skipped_record(rec, dlb_out, swapped); }
};

// A listed (query, octree leaf, triangle) item per BS_W-lane group.  The items of valid queries only are listed, so the ids are inside
// the tables; the triangle index is below the mesh's triangle count (hfcl_lib_add_bvh checks every leaf link)
__global__ void __launch_bounds__(64) k_octm_leaf(OctMeshArgs a) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<double, EPA_MAX_ITER> scratch[G];
  const int lane = threadIdx.x & 63, grp = lane / BS_W;
  for (uint64_t it = uint64_t(blockIdx.x) * G + grp; it < a.n_items; it += uint64_t(gridDim.x) * G) {
    const OctMeshItem<double> item = a.items[it];
    const DMesh me = a.meshes[a.shapes[a.shape[item.query]].bvh_index];
    const Pose<double> tft = load_pose(a.tf_c, item.query), tfm = load_pose(a.tf_s, item.query);
    OctMeshLeafOut<double> out;
    octm_leaf<double, LaneGroup<BS_W>>(mk<double>(item.lo[0], item.lo[1], item.lo[2]), mk<double>(item.hi[0], item.hi[1], item.hi[2]), tft,
                                       a.mverts + 3 * size_t(me.vert_off), a.mtris + 3 * (size_t(me.tri_off) + item.prim), tfm, a.q, &scratch[grp], out);
    out.prim = item.prim;
    out.pad_ = 0u;
    if ((lane & (BS_W - 1)) == 0) a.leaves[it] = out;
    LaneGroup<BS_W>::sync();
  }
}

void launch_octm_count(hipStream_t st, const OctMeshArgs& a) { launch_listed_count<OctMeshKind>(st, a); }

// launch_listed_solve with this unit's leaf kernel
void launch_octm_solve(hipStream_t st, const OctMeshArgs& a, int max_blocks, bool want_contacts, const char** names, hipEvent_t* e0, hipEvent_t* e1) {
  for (int k = 0; k < LISTED_TIMED_KERNELS; ++k) names[k] = OctMeshKind::timer_names[k];
  if (!a.m) return;
  auto begin = [&](int k) { if (e0) (void)hipEventRecord(e0[k], st); };
  auto end = [&](int k) { if (e1) (void)hipEventRecord(e1[k], st); };
  begin(0);
  hipLaunchKernelGGL((k_listed_walk<OctMeshKind, true>), dim3((a.m + 63u) / 64u), dim3(64), 0, st, a);
  end(0);
  begin(1);
  if (a.n_items) {
    constexpr uint64_t G = 64 / BS_W;
    const uint32_t grid = uint32_t(std::min<uint64_t>((a.n_items + G - 1u) / G, uint64_t(std::max(max_blocks, 1))));
    hipLaunchKernelGGL(k_octm_leaf, dim3(grid), dim3(64), 0, st, a);
  }
  end(1);
  begin(2);
  hipLaunchKernelGGL((k_listed_fold<OctMeshKind, false>), dim3((a.m + 255u) / 256u), dim3(256), 0, st, a);
  end(2);
  begin(3);
  if (want_contacts) launch_hf_scan(st, a.ccounts, a.coffsets, a.m, a.running);
  end(3);
  begin(4);
  if (want_contacts && a.contacts) hipLaunchKernelGGL((k_listed_fold<OctMeshKind, true>), dim3((a.m + 255u) / 256u), dim3(256), 0, st, a);
  end(4);
}
