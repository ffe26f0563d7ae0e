// hfcl_k_octree_distance.hip -- OcTree x convex solid distance() on the device (hfcl_octree_distance_batch*; the arithmetic:
// hfcl_octree_distance.hpp).  Built without contraction (FLAGS_k_octree_distance): the records are the bits of the header's host build
// (tests/octree_distance_harness).
//   k_oct_distance   The descent into a child hangs on the running minimum, so a query is serial: one BS_W-lane group per query, four
//                    groups to a 64-lane workgroup (the shape of k_bvh_shape_distance).  Per group in LDS: the walk's stack (node, next
//                    child, box and the eight child-box distances of each level) and a full-capacity EPA polytope.  The loop of a
//                    group is "advance the walk to the next leaf to solve, or to its end; then solve": the groups of a wave meet at
//                    the solve, which is the group solver of the octree leaves (hfcl_k_octree.hip) (the group's lanes share a hull's support scan and EPA's face
//                    work).  When an inner node is pushed, lanes 0..7 compute the box distances of its eight children in one step; the
//                    comparisons against the minimum are taken serially in index order.  Lane 0 writes the record.  No atomics, no
//                    workspace, no read-back.
// Every loop is bounded by what its comment names: 2 * n_nodes + 2 steps of a walk, n_nodes solved leaves, OCT_STACK, a hull's vertices,
// gjk_max_iterations / epa_max_iterations (hfcl_gjk.hpp / hfcl_epa.hpp).
#include "hfcl_dev.hpp"
#include "hfcl_octree_distance.hpp"

using namespace hfcl;

__global__ void __launch_bounds__(64) k_oct_distance(OctDistArgs a) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<double, EPA_MAX_ITER> scratch[G];
  __shared__ OctDistStack<double> stack[G];
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint64_t i = uint64_t(blockIdx.x) * G + grp; i < a.m; i += uint64_t(gridDim.x) * G) {  // (bound: the chunk's queries)
    const bool swapped = a.swapped && a.swapped[i];
    const uint32_t t = a.octree[i], sid = a.shape[i];
    // ids inside the tables, a solid with an evaluator: else a skipped record, as collide
    const bool valid = t < a.n_trees && sid < a.n_shapes && oct_kind_supported(a.shapes[sid].kind);
    if (!valid) {
      if (lig == 0) {
        oct_skipped_record(&a.out[i], nullptr, swapped);
        if (a.n_visited) a.n_visited[i] = 0u;
      }
      continue;
    }
    const DOctree tr = a.trees[t];
    GroupSolid solid;  // (hfcl_listed.hpp: the group's support of the solid, as k_listed_leaf)
    solid.load(a, uint32_t(i), lig);
    const Pose<double> tft = load_pose(a.tf_t, i), tfs = load_pose(a.tf_s, i);
    OctDistResult<double> r;
    bool overflow;
    oct_distance_query<double, LaneGroup<BS_W>>(a.nodes + tr.node_off, tr, tft, solid.s, a.verts, tfs, solid, a.q, &stack[grp], &scratch[grp], r,
                                                overflow);
    if (lig == 0) {
      hfcl_result rec;
      oct_dist_record(r, swapped, &rec);
      a.out[i] = rec;
      if (a.n_visited) a.n_visited[i] = r.visited;
    }
    LaneGroup<BS_W>::sync();
  }
}

void launch_oct_distance(hipStream_t st, const OctDistArgs& a, int max_blocks) {
  if (!a.m) return;
  constexpr uint32_t G = 64 / BS_W;
  const uint32_t grid = std::min<uint32_t>((a.m + G - 1u) / G, uint32_t(std::max(max_blocks, 1)));
  hipLaunchKernelGGL(k_oct_distance, dim3(grid), dim3(64), 0, st, a);
}
