// hfcl_k_octree_mesh_distance.hip -- OcTree x BVHModel<OBBRSS> distance() on the device (hfcl_octree_mesh_distance_batch*; the
// arithmetic: hfcl_octree_mesh_distance.hpp).  Built without contraction (FLAGS_k_octree_mesh_distance): the records are the bits of the
// header's host build (tests/octree_mesh_distance_harness).
//   k_octm_distance  The descent into a child -- of the octree node or of the mesh node -- hangs on the running minimum, so a query is
//                    serial: neither the listed-leaf pipeline (whose walk must not depend on the leaves) nor k_oct_distance (one tree)
//                    can run it.  One BS_W-lane group per query, four groups to a 64-lane workgroup (the shape of k_oct_distance).
//                    Per group in LDS: the path stack (16 octree frames with the eight box distances of their children, 64 mesh frames
//                    with the two of theirs) and a full-capacity EPA polytope.  The loop of a group is "advance the walk to the next
//                    (leaf, triangle) pair to solve, or to its end; then solve": the groups of a wave meet at the solve, the Box x
//                    TriangleP solve of the collide leaf kernel (octm_leaf).  When a frame is pushed, lanes 0..7 (0..1) compute the box
//                    distances of its children in one step; the comparisons against the minimum are taken serially, in order.  Lane 0
//                    writes the record.  No atomics, no workspace, no read-back; no workgroup waits for another.
// Every loop is bounded by what its comment names: 2 * n_nodes * n_mesh_nodes + 2 steps of a walk and as many solved pairs, OCT_STACK,
// OCTM_MESH_STACK, gjk_max_iterations / epa_max_iterations (hfcl_gjk.hpp / hfcl_epa.hpp).
#include "hfcl_dev.hpp"
#include "hfcl_octree_mesh_distance.hpp"

using namespace hfcl;

__global__ void __launch_bounds__(64) k_octm_distance(OctMeshDistArgs a) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<double, EPA_MAX_ITER> scratch[G];
  __shared__ OctMeshDistStack<double> stack[G];
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint64_t i = uint64_t(blockIdx.x) * G + grp; i < a.m; i += uint64_t(gridDim.x) * G) {  // (bound: the chunk's queries)
    const bool swapped = a.swapped && a.swapped[i];
    const uint32_t t = a.octree[i], sid = a.shape[i];
    // ids inside the tables, a shape row that names a registered mesh: else a skipped record, as collide
    const bool valid = t < a.n_trees && sid < a.n_shapes && a.shapes[sid].kind == K_BVH && a.shapes[sid].bvh_index < a.n_meshes;
    if (!valid) {
      if (lig == 0) {
        oct_skipped_record(&a.out[i], nullptr, swapped);
        if (a.n_visited) a.n_visited[i] = 0u;
      }
      continue;
    }
    const DOctree tr = a.trees[t];
    const DMesh me = a.meshes[a.shapes[sid].bvh_index];
    const Pose<double> tft = load_pose(a.tf_t, i), tfm = load_pose(a.tf_m, i);
    OctMeshDistResult<double> r;
    bool overflow;
    // (a triangle index is below the mesh's triangle count, a child link inside its nodes: hfcl_lib_add_bvh checks every link)
    octm_distance_query<double, LaneGroup<BS_W>>(a.nodes + tr.node_off, tr, tft, a.mnodes + me.node_off, me.n_nodes, a.mverts + 3 * size_t(me.vert_off),
                                                 a.mtris + 3 * size_t(me.tri_off), tfm, a.q, &stack[grp], &scratch[grp], r, overflow,
                                                 OctMeshDistNoList());
    if (lig == 0) {
      hfcl_result rec;
      octmd_record(r, swapped, &rec);
      a.out[i] = rec;
      if (a.n_visited) a.n_visited[i] = r.visited;
    }
    LaneGroup<BS_W>::sync();
  }
}

void launch_octm_distance(hipStream_t st, const OctMeshDistArgs& a, int max_blocks) {
  if (!a.m) return;
  constexpr uint32_t G = 64 / BS_W;
  const uint32_t grid = std::min<uint32_t>((a.m + G - 1u) / G, uint32_t(std::max(max_blocks, 1)));
  hipLaunchKernelGGL(k_octm_distance, dim3(grid), dim3(64), 0, st, a);
}
