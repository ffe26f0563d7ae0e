/* hppfcl_amd_octree_mesh.h -- hpp::fcl::OcTree against BVHModel<OBBRSS>: the batched collide(), in both operand orders, in fp64.  Part of
 * the C ABI of hppfcl_amd.h (which includes this file; the ABI version stays 5: the entry points below are additions).  The trees are
 * those of hppfcl_amd_octree.h (hfcl_lib_add_octree), the meshes those of hfcl_lib_add_bvh, named through a HFCL_BV_OBBRSS row of the
 * shape table (its bvh_index).  hfcl_octree_collide_batch*, hfcl_octree_pair_supported and hfcl_pair_supported keep their answers: a
 * mesh stays refused THERE; the pair has the calls below.
 *
 * collide() (OctreeCollide src/collision_func_matrix.cpp:52-75, OcTreeMeshIntersect / OcTreeMeshIntersectRecurse
 * internal/traversal_node_octree.h:100-139, 462-563).  One step on (octree node with its box, mesh node):
 *   - the empty tree (n_nodes == 0): no box test, no leaf, the bound stays DBL_MAX;
 *   - a node whose occupancy is <= free_threshold or < occupancy_threshold ends its branch, inner nodes included;
 *   - the box test, at EVERY entry (also when only the mesh side descended and the octree box is the same): the node's box under the
 *     tree's pose (convertBV<AABB, OBB>) against the OBB half of the mesh node under the mesh's pose (convertBV<OBBRSS, OBB>,
 *     BV/BV.h:94-113: extent copied, To = R * To + T, axes = R * axes; the RSS half is not read) through
 *     OBB::overlap(other, request, sqr) (src/BV/OBB.cpp:405-423); disjoint: updateDistanceLowerBoundFromBV and the branch ends;
 *   - octree leaf x mesh leaf: Box(max - min) at tf_octree * Transform3f(center) against the TriangleP of the mesh leaf through
 *     ShapeShapeDistance<Box, TriangleP> (GJKSolver::shapeDistance(S1, tf1, TriangleP, tf2), narrowphase.h:320-336: the triangle moved
 *     into the box's frame, the Box is shape 0, the result in Box-first order); updateDistanceLowerBoundFromLeaf(distance - margin);
 *     a contact while numContacts() < num_max_contacts and distance - margin <= collision_distance_threshold; the step returns
 *     isSatisfied();
 *   - which side descends: the octree's existing children in index order 0..7 when the mesh node is a leaf, or when the octree node
 *     has children and bv1.size() > bvn2.bv.size(); otherwise the mesh node's left child, then its right child.  The two sizes are NOT
 *     the same quantity: AABB::size() is the squared FULL diagonal (AABB.h:162), OBBRSS::size() the squared norm of the HALF extents
 *     (OBB.h:110, OBBRSS.h:114).  The factor of four is the reference's and is reproduced.
 *   Any `true` from below ends the whole walk.
 *
 * Operand order.  MeshOcTreeIntersect runs the same recursion with the operands exchanged (traversal_node_octree.h:128-139, 1118-1121)
 * and collide() swaps back only for GEOM x BVH / HFIELD (src/collision.cpp:92-108): collide(mesh, octree) returns the octree-first result
 * UNSWAPPED.  swapped[i] = 1 states that the caller's order was (mesh, octree): bit 23 of the record's status is set and no other byte
 * changes.  tf_octree / tf_mesh are always the tree's and the mesh's pose (12 doubles a row).
 *
 * Records (one hfcl_result per query):
 *   num_contacts   CollisionResult::numContacts()
 *   with a contact:    distance = the FIRST contact's penetration_depth; normal = its normal; p1, p2 = its nearest_points, which here are
 *                      the solver's OWN points c1, c2 (the eight-argument Contact constructor, collision_data.h:138-148; the octree x
 *                      solid path rebuilds them from pos and depth, this path does not); b1 = the leaf's index in the registered node
 *                      array; b2 = the triangle's index in the mesh, as the mesh x solid collide() reports it
 *   without a contact: distance = CollisionResult::distance_lower_bound; normal, p1, p2 = the result's (NaN where no leaf lowered the
 *                      bound); b1 = b2 = -1
 *   status         bit 7 the contact flag, bit 23 the caller's order was (mesh, octree), bit 31 skipped.  GJK / EPA status and iteration
 *                  fields are not reported: 0 and HFCL_EPA_DID_NOT_RUN are written.
 * distance_lower_bound (optional, n doubles): the bound AT THE MOMENT THE REFERENCE'S WALK STOPS -- box tests the reference never reaches
 * after isSatisfied() do not lower it; DBL_MAX for a skipped query.
 * contacts: NULL, or room for max_contacts_total hfcl_contact records (pair = the query, b1 = the node, b2 = the triangle; p1, p2 = c1,
 * c2), in query order and within a query in walk order; contacts beyond the capacity are counted in *n_contacts_out and dropped.
 *
 * Requests, all before any work, as hfcl_octree_collide_batch: num_max_contacts == 0: HFCL_ERR_INVALID_ARGUMENT; a finite negative
 * security_margin: HFCL_ERR_INVALID_ARGUMENT; security_margin == -inf: every record skipped; epa_max_iterations > 64: HFCL_ERR_LIMIT;
 * gjk_initial_guess other than DefaultGuess, or distance_upper_bound other than its default: HFCL_ERR_LIMIT.  Host form: an octree or
 * shape id outside the library: HFCL_ERR_INVALID_ARGUMENT; a shape that is not a registered mesh: HFCL_ERR_UNSUPPORTED_PAIR.  The device
 * form cannot see the ids: there such a query gets a SKIPPED record (status bit 31, every other field 0 but bit 23, bound DBL_MAX, no
 * contacts) and the call returns HFCL_OK.  Without a device: HFCL_ERR_NO_DEVICE.
 *
 * The depth of a mesh.  The walk keeps one frame per level of the recursion: at most 16 for the octree and one per level of the mesh's
 * BVH.  A mesh whose BVH has more than HFCL_OCTREE_MESH_MAX_BVH_DEPTH levels (the root is level 1) is refused, never walked in part: the
 * host form returns HFCL_ERR_LIMIT when a mesh NAMED by the batch is deeper, the device form -- which cannot see the ids -- when ANY
 * registered mesh is deeper; nothing is written.  The depths are computed on the host by the first call that needs them.
 *
 * Work on the device: the listed-leaf pipeline of hppfcl_amd_octree.h with the same options (`octree_chunk`, `octree_items`; records
 * depend on neither; one query that lists more than 2^26 (leaf, triangle) items: HFCL_ERR_LIMIT) and the same waits: once per chunk for
 * the item count, once at the end when n_contacts_out is given.  Per chunk: every query's dual walk is counted, the counts scanned, the
 * reached (leaf, triangle) pairs listed in walk order with their boxes, every item solved by a lane group, and one replay per query
 * folds its items in order.  A query is walked by ONE lane: few queries with long walks are bound by that walk.
 *
 * distance() for the pair (OcTreeMeshDistanceRecurse) has a header of its own: hppfcl_amd_octree_mesh_distance.h.
 *
 * Not done: octree x octree and x height field; BV types other than OBBRSS; fp32
 * and hfcl_multi_* forms; cached and bounding-volume GJK guesses; a finite distance_upper_bound; octrees as scene objects; a pooled or
 * wave-wide form of the walk; a leaf pass in rounds that stops at a query's first contact. */
#ifndef HPPFCL_AMD_OCTREE_MESH_H
#define HPPFCL_AMD_OCTREE_MESH_H
#include "hppfcl_amd.h"
#include "hppfcl_amd_octree.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HFCL_OCTREE_MESH_MAX_BVH_DEPTH 64u

/* 1 for HFCL_BV_OBBRSS; 0 for everything else */
int hfcl_octree_mesh_pair_supported(int32_t node_type);

int hfcl_octree_mesh_collide_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_mesh,
                                   size_t n, const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out,
                                   double* distance_lower_bound, hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out);
/* the same call on device pointers (n_contacts_out: host memory), asynchronous on `stream` but for the waits named above */
int hfcl_octree_mesh_collide_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                          const double* d_tf_mesh, size_t n, const uint8_t* d_swapped, const hfcl_collision_request* req,
                                          hfcl_result* d_out, double* d_distance_lower_bound, hfcl_contact* d_contacts,
                                          size_t max_contacts_total, size_t* n_contacts_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_OCTREE_MESH_H */
