/* hppfcl_amd_octree_distance.h -- distance() between a registered hpp::fcl::OcTree (hppfcl_amd_octree.h) and a convex solid -- Box,
 * Sphere, Capsule, Cone, Cylinder, Ellipsoid, Convex -- batched, in both operand orders, in fp64.  Part of the C ABI of hppfcl_amd.h
 * (which includes this file; the ABI version stays 5: the entry points below are additions).  hfcl_distance_batch*, hfcl_pair_supported
 * and the function matrices keep their answers: GEOM_OCTREE stays unsupported THERE.  Registration, thresholds and upload are those of
 * the collide calls: the same trees (hfcl_lib_add_octree, hfcl_lib_octree_set_thresholds), the same device copy.
 *
 * distance() (distance_matrix[GEOM_OCTREE][GEOM_*] and the transposed rows, src/distance_func_matrix.cpp:605-622;
 * OcTreeSolver::OcTreeShapeDistance / ShapeOcTreeDistance / OcTreeShapeDistanceRecurse, internal/traversal_node_octree.h:216-297).  The
 * answer is the result of the reference's ORDERED walk, not the minimum over all occupied leaves:
 *   1. aabb2 = computeBV<AABB>(solid, tf_solid), once per query: the per-kind formulas of the reference, no swept-sphere radius.
 *   2. A node without children is a leaf.  An occupied one (occupancy >= occupancy_threshold) is solved: Box(max - min) at
 *      tf_tree * Transform3f(center) against the solid through ShapeShapeDistance<Box, S> -- the per-pair distance() of this library for
 *      that box and pose (the closed form for a Sphere, GJK and EPA under enable_signed_distance for the rest) -- and
 *      DistanceResult::update (collision_data.h:1111-1124) takes it on a strict min_distance > distance, with the solver's own p1, p2 and
 *      normal (not rebuilt, unlike collide's contacts) and b1 = the node.  The walk ends as soon as min_distance <= 0
 *      (DistanceRequest::isSatisfied).  A leaf that is not occupied contributes nothing.
 *   3. An inner node that is not occupied ends its branch (free and uncertain are the same here: the recursion tests isNodeOccupied only;
 *      free_threshold is not read).
 *   4. The existing children of an occupied inner node are taken in index order 0..7: the child's box by computeChildBV, aabb1 =
 *      Converter<AABB, AABB>::convert(child_bv, tf_tree) (BV/BV.h:66-73: centre R * center + T, half side ||max - min|| * 0.5 on every
 *      axis), d = aabb1.distance(aabb2) (src/BV/AABB.cpp:115-133), and the walk descends iff d < min_distance with the minimum as it
 *      stands at that moment.
 *   5. The root gets no box test; a root without children is a leaf with the root box.
 *
 * Reproduced on purpose / a choice:
 *   - The Ellipsoid's box.  computeBV<AABB, Ellipsoid> is R * radii without absolute values, so under a rotation the box can have
 *     min > max on an axis, AABB::distance over-estimates on it, and the walk prunes leaves it should have visited: for an Ellipsoid the
 *     answer can be LARGER than the distance to the nearest occupied leaf (by up to 0.15 on the test trees).  This is the reference's
 *     answer and it is reproduced on purpose.  For the other six kinds the ordered walk equalled the brute-force minimum in every
 *     separated test query.
 *   - The empty tree.  For n_nodes == 0 the reference dereferences a null root.  This library answers with the untouched
 *     DistanceResult: distance DBL_MAX, NaN points and normal, b1 = b2 = -1, n_visited 0.  That is a choice.
 *
 * Operand order.  Distance<S, OcTree> runs ShapeOcTreeDistance, the same recursion with the poses exchanged, and src/distance.cpp swaps
 * back only for BVH and height fields.  So distance(solid, octree) returns the octree-first result UNSWAPPED, exactly as collide does:
 * the tree's node in b1, p1 on the tree's box, the normal from the box to the solid.  swapped[i] = 1 states that the caller's order was
 * (solid, octree): bit 23 of the record's status is set and no other byte changes.  tf_octree / tf_shape are always the tree's and the
 * solid's pose (12 doubles a row).
 *
 * Records (one hfcl_result per query):
 *   distance       DistanceResult::min_distance (DBL_MAX where no leaf was solved)
 *   normal, p1, p2 the solver's own for the leaf that set the minimum; NaN where no leaf was solved (and where the solver reports none:
 *                  a penetrating leaf without enable_signed_distance)
 *   b1, b2         that leaf's index in the registered node array (-1: none); b2 = -1
 *   status         bit 7: min_distance <= 0; bit 23: the caller's order was (solid, octree); bit 31: skipped.  The GJK and EPA fields
 *                  are written as the octree collide records write them: 0 and HFCL_EPA_DID_NOT_RUN
 *   num_contacts   0
 * n_visited (optional, n words): the number of leaves the walk solved for each query (0 for a skipped one).
 *
 * Requests, all before any output.  A null library: HFCL_ERR_INVALID_ARGUMENT; a null request: HFCL_ERR_INVALID_ARGUMENT, as
 * hfcl_distance_batch; gjk_initial_guess other than DefaultGuess: HFCL_ERR_LIMIT (CachedGuess chains the solver's guess from leaf to
 * leaf, BoundingVolumeGuess changes the leaf set-up); epa_max_iterations > 64: HFCL_ERR_LIMIT.  rel_err and abs_err are not read: the
 * reference's octree walk does not read them.  enable_nearest_points is not read either: the points are always written.  Host form: an
 * octree or shape id outside the library HFCL_ERR_INVALID_ARGUMENT, a solid without an evaluator
 * (hfcl_octree_distance_pair_supported) HFCL_ERR_UNSUPPORTED_PAIR.  The device form cannot see the ids: there such a query gets a
 * SKIPPED record (status bit 31, every other field 0 but bit 23) and the call returns HFCL_OK.  Without a device: HFCL_ERR_NO_DEVICE,
 * as every compute entry point (no CPU fallback).
 *
 * Work on the device.  The running minimum makes a query serial: one 16-lane group per query walks the tree and solves its leaves one
 * after the other; lanes 0..7 compute the eight child-box distances of an inner node in one step.  No atomics, no workspace that grows
 * with the leaf count, no read-back: the device form is asynchronous on `stream` throughout (but for growing the library's device copy of
 * newly registered trees).  The queries of a call go in chunks of option `octree_chunk` (0 = automatic); records do not depend on it.
 * Option `octree_items` has no meaning for this call.  A wave takes as long as its longest walk.
 *
 * Not done: Plane and Halfspace against an octree; fp32 and hfcl_multi_* forms; cached and bounding-volume GJK guesses; a lane-per-query
 * or pooled continuation form for the long walks; octree x octree; octrees in scenes.  (Octree x mesh: hppfcl_amd_octree_mesh_distance.h.) */
#ifndef HPPFCL_AMD_OCTREE_DISTANCE_H
#define HPPFCL_AMD_OCTREE_DISTANCE_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 1 for Box, Sphere, Capsule, Cone, Cylinder, Ellipsoid, Convex; 0 for everything else (Plane and Halfspace included) */
int hfcl_octree_distance_pair_supported(int32_t node_type_of_solid);

int hfcl_octree_distance_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_shape,
                               size_t n, const uint8_t* swapped, const hfcl_distance_request* req, hfcl_result* out, uint32_t* n_visited);
/* the same call on device pointers, asynchronous on `stream` */
int hfcl_octree_distance_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                      const double* d_tf_shape, size_t n, const uint8_t* d_swapped, const hfcl_distance_request* req,
                                      hfcl_result* d_out, uint32_t* d_n_visited, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_OCTREE_DISTANCE_H */
