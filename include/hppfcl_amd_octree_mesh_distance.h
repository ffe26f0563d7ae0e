/* hppfcl_amd_octree_mesh_distance.h -- distance() between a registered hpp::fcl::OcTree (hppfcl_amd_octree.h) and a registered
 * BVHModel<OBBRSS> (hfcl_lib_add_bvh, named through a HFCL_BV_OBBRSS row of the shape table), batched, in both operand orders, in fp64.
 * Part of the C ABI of hppfcl_amd.h (which includes this file; the ABI version stays 5: the entry points below are additions).
 * hfcl_distance_batch*, hfcl_pair_supported, hfcl_octree_distance_pair_supported and the function matrices keep their answers: the pair
 * stays refused THERE; it has the calls below.  Trees, thresholds, meshes and their device copies are those of the collide calls.
 *
 * distance() (OcTreeSolver::OcTreeMeshDistance internal/traversal_node_octree.h:113-124, OcTreeMeshDistanceRecurse :371-458, the two
 * traversal nodes :1307-1353; BV/BV.h:66-73 and :132-140, BV/OBB.h:110-122, src/BV/AABB.cpp:115-133, narrowphase/narrowphase.h:319-336,
 * collision_data.h:1111-1124, src/distance.cpp:111-150).  The answer is the result of the reference's ORDERED dual walk.  One entry of the
 * recursion takes an octree node o with its box bv1, carried down by computeChildBV from the root box, and a mesh node m:
 *   1. Leaf pair: o has no children and m is a leaf.  An occupied o (occupancy >= occupancy_threshold) is solved: Box(max - min) at
 *      tf_octree * Transform3f(center) against the leaf's TriangleP through ShapeShapeDistance<Box, TriangleP> (the triangle moved into
 *      the box's frame, the Box is shape 0; enable_signed_distance from the request), then DistanceResult::update: a strict
 *      min_distance > distance takes the distance, the solver's own p1, p2 and normal in Box-first order, b1 = the node's index,
 *      b2 = the triangle's primitive id.  The entry returns min_distance <= 0, and a `true` ends the whole walk.  An o that is not
 *      occupied contributes nothing.
 *   2. An o that is not occupied ends its branch, also an unoccupied octree leaf against an inner mesh node.  Free and uncertain are the
 *      same here; free_threshold is not read.
 *   3. The octree side descends when m is a leaf, or when o has children and bv1.size() > bv(m).size().  bv1.size() is the squared FULL
 *      diagonal, bv(m).size() the squared norm of the HALF extents: the rule and the factor of four of the collide walk
 *      (hppfcl_amd_octree_mesh.h).  The existing children are taken in index order 0..7; for child i, aabb1 =
 *      Converter<AABB, AABB>(child_bv, tf_octree) (centre R * center + T, half side ||max - min|| * 0.5 on every axis), aabb2 =
 *      Converter<OBBRSS, AABB>(bv(m), tf_mesh) (centre tf_mesh.transform(obb.To), half side ||(2 e0, 2 e1, 2 e2)|| * 0.5; the RSS half
 *      is not read), d = aabb1.distance(aabb2), and the walk descends iff d < min_distance with the minimum as it stands at that moment.
 *   4. Otherwise the mesh side descends, the left child first, then the right: aabb1 is the conversion of the current bv1, aabb2 that of
 *      the child, the test the same d < min_distance against the minimum as it stands, which the left subtree may have lowered.
 *   5. The root pair gets no box test.
 * Both converted boxes enclose their bounding volumes, so d is a true lower bound: the ordered walk's distance equals the minimum over all
 * reachable occupied leaves x triangles whenever that minimum is positive (the Ellipsoid exception of hppfcl_amd_octree_distance.h has no
 * counterpart here).
 *
 * A choice: the empty tree.  For n_nodes == 0 the reference dereferences a null root.  This library answers with the untouched
 * DistanceResult: distance DBL_MAX, NaN points and normal, b1 = b2 = -1, n_visited 0 -- a choice, the one hfcl_octree_distance_batch made.
 *
 * Operand order.  MeshOcTreeDistanceTraversalNode calls OcTreeMeshDistance(model2, model1, tf2, tf1, ...), and src/distance.cpp swaps back
 * only for GEOM x BVH and height fields: distance(mesh, octree) returns the octree-first result UNSWAPPED.  swapped[i] = 1 states that the
 * caller's order was (mesh, octree): bit 23 of the record's status is set and no other byte changes.  tf_octree / tf_mesh are always the
 * tree's and the mesh's pose (12 doubles a row).  (The overload OcTreeSolver::MeshOcTreeDistance, :141-152, is never instantiated and is
 * not a source.)
 *
 * Records (one hfcl_result per query, the layout of hfcl_octree_distance_batch):
 *   distance       DistanceResult::min_distance (DBL_MAX where no pair was solved)
 *   normal, p1, p2 the solver's own for the pair that set the minimum; NaN where no pair was solved, and where the solver reports none (a
 *                  penetrating leaf without enable_signed_distance)
 *   b1, b2         the node's index in the registered node array, the triangle's index in the mesh (-1, -1: none)
 *   status         (HFCL_EPA_DID_NOT_RUN << 3); bit 7: min_distance <= 0; bit 23: the caller's order was (mesh, octree); bit 31: skipped
 *   num_contacts   0
 * n_visited (optional, n words): the number of (leaf, triangle) pairs the walk solved for each query (0 for a skipped one).
 *
 * Requests, all before any output.  As hfcl_octree_distance_batch*: a null library or request: HFCL_ERR_INVALID_ARGUMENT;
 * gjk_initial_guess other than DefaultGuess: HFCL_ERR_LIMIT; epa_max_iterations > 64: HFCL_ERR_LIMIT; rel_err, abs_err and
 * enable_nearest_points are not read.  As the mesh collide call for the second operand: host form -- an octree or shape id outside the
 * library HFCL_ERR_INVALID_ARGUMENT, a shape that is not a registered OBBRSS mesh HFCL_ERR_UNSUPPORTED_PAIR; the device form cannot see
 * the ids: there such a query gets a SKIPPED record (status bit 31, every other field 0 but bit 23) and the call returns HFCL_OK.
 * Without a device: HFCL_ERR_NO_DEVICE, as every compute entry point (no CPU fallback).
 *
 * The depth of a mesh.  The walk keeps one frame per level of the recursion: at most 16 for the octree and one per level of the mesh's
 * BVH.  A mesh whose BVH has more than HFCL_OCTREE_MESH_MAX_BVH_DEPTH levels (hppfcl_amd_octree_mesh.h; the root is level 1) is refused,
 * never walked in part: the host form returns HFCL_ERR_LIMIT when a mesh NAMED by the batch is deeper, the device form -- which cannot see
 * the ids -- when ANY registered mesh is deeper; nothing is written.
 *
 * Work on the device.  The running minimum makes a query serial: one 16-lane group per query walks the two trees over a path stack and
 * solves its (leaf, triangle) pairs one after the other; when a frame is pushed, lanes 0..7 compute the eight child-box distances of an
 * octree node in one step, lanes 0..1 the two of a mesh node.  No atomics, no workspace that grows with the walk, no read-back: the device
 * form is asynchronous on `stream` throughout (but for growing the library's device copies of newly registered trees and meshes).  The
 * queries of a call go in chunks of option `octree_chunk` (0 = automatic); records do not depend on it.  Option `octree_items` has no
 * meaning for this call.  A wave takes as long as its longest walk.
 *
 * The shims offer the call under names of their own (hpp::fcl::amd::distanceOcTreeMesh, amd::OcTreeBatch::distanceMesh;
 * compat.distance_octree_mesh).  The dispatch of hpp::fcl::distance() / ComputeDistance keeps refusing the pair: taking it there is the
 * follow-up, and it needs the two tests that hold the refusal (tests/test_octree_mesh_gpu.py, tests/cpp/test_octree_mesh.cpp) changed.
 *
 * Not done: the pair inside the distance() / ComputeDistance dispatch of the shims; BV types other than OBBRSS; octree x octree and
 * x height field; fp32 and hfcl_multi_* forms; cached and bounding-volume GJK guesses; a pooled continuation or wave-wide form for the
 * long walks (few queries with long walks use one group each); several pairs of a walk solved at once; octrees as scene objects. */
#ifndef HPPFCL_AMD_OCTREE_MESH_DISTANCE_H
#define HPPFCL_AMD_OCTREE_MESH_DISTANCE_H
#include "hppfcl_amd.h"
#include "hppfcl_amd_octree_mesh.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 1 for HFCL_BV_OBBRSS; 0 for everything else */
int hfcl_octree_mesh_distance_pair_supported(int32_t node_type);

int hfcl_octree_mesh_distance_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_mesh,
                                    size_t n, const uint8_t* swapped, const hfcl_distance_request* req, hfcl_result* out, uint32_t* n_visited);
/* the same call on device pointers, asynchronous on `stream` */
int hfcl_octree_mesh_distance_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                           const double* d_tf_mesh, size_t n, const uint8_t* d_swapped, const hfcl_distance_request* req,
                                           hfcl_result* d_out, uint32_t* d_n_visited, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_OCTREE_MESH_DISTANCE_H */
