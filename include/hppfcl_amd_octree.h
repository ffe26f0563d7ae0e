/* hppfcl_amd_octree.h -- hpp::fcl::OcTree (include/hpp/fcl/octree.h) against convex solids: the node array, the registration on a
 * library and the batched collide(), in both operand orders, in fp64.  Part of the C ABI of hppfcl_amd.h (which includes this file; the
 * ABI version stays 5: the entry points below are additions).  hfcl_collide_batch*, hfcl_pair_supported and the function matrices keep
 * their answers: GEOM_OCTREE stays unsupported THERE; octrees have the calls below.
 *
 * The tree.  The reference reads an octomap tree through four calls (getRoot, nodeHasChildren, nodeChildExists / getNodeChild,
 * getOccupancy) and computes every box itself: the root box is +-(1 << depth) * resolution / 2 on every axis (getRootBV,
 * octree.h:139-144), the box of child i halves its parent's along each axis, (min + max) * 0.5, the upper half where bit 0 / 1 / 2 of
 * i is set (computeChildBV, :299-324).  So a tree is a flat array of nodes: node 0 is the root; child[i] is the index of child i in
 * the array, 0 = no such child; occupancy is the node's probability.  A box is the result of that chain of halvings from the root -- with
 * a resolution such as 0.1 not key * resolution in the last bit -- and the walk below carries it down the path as the reference does.
 * n_nodes == 0 is the empty tree (`if (!root1) return false`): no box test, no leaf, the bound stays DBL_MAX.
 *
 * hfcl_octree_validate: depth in 1..16; every child index inside (0, n_nodes); every node but the root has exactly one parent (so the
 * array is one tree: no cycle, no orphan); no node lies deeper than `depth`; no NaN occupancy.  Each failure:
 * HFCL_ERR_INVALID_ARGUMENT.  hfcl_lib_add_octree validates the same way.
 *
 * hfcl_octree_from_points is makeOctree (src/octree.cpp:188-202) without octomap: per axis key = floor(x / resolution) + 2^(depth-1),
 * points whose key falls outside [0, 2^depth) on an axis (or is not finite) are dropped; one leaf at level `depth` per distinct key,
 * occupancy 0.7 for the first hit, raised by every further hit (log-odds + logit(0.7)) and clamped at 0.97; an inner node takes the
 * maximum of its children; nodes in depth-first preorder, children in index order (child bit 0 = x, 1 = y, 2 = z of the key's bit at
 * that level).  These constants are octomap's defaults AS REMEMBERED: octomap is not part of this project's build or tests and they
 * were NOT checked against it.  The collide answers depend only on occupancy >= occupancy_threshold and <= free_threshold.
 * nodes_out == NULL: the count alone; capacity below the count: HFCL_ERR_LIMIT (the count is still written).
 *
 * collide() (OctreeCollide src/collision_func_matrix.cpp:52-75, OcTreeShapeIntersect / OcTreeShapeIntersectRecurse
 * internal/traversal_node_octree.h:183-197, 299-369): the solid's LOCAL box (computeBV<AABB>(s, identity); here the library's local box
 * of the shape, which includes a swept-sphere radius) becomes an OBB under the solid's pose (convertBV, BV/BV.h:79-84).  A node whose
 * occupancy is <= free_threshold (free) or < occupancy_threshold (uncertain) ends its branch, inner nodes included; otherwise its box
 * under the tree's pose is an OBB, tested with OBB::overlap(other, request, sqr) (src/BV/OBB.cpp:405-423), every node, leaves included;
 * disjoint: updateDistanceLowerBoundFromBV (collision_data.h:1177-1184) and the branch ends.  A node without children is a leaf:
 * Box(max - min) at tf_tree * Transform3f(center) against the solid through ShapeShapeCollide<Box, S> -- the per-pair collide of this
 * library for that box and pose (the closed form for a Sphere, GJK / EPA for the rest).  Children are visited in index order 0..7; the
 * walk stops when num_max_contacts contacts exist.
 *
 * Operand order.  collide() swaps back only for GEOM x BVH / HFIELD (src/collision.cpp:92-108); there is no octree branch, and
 * ShapeOcTreeCollisionTraversalNode::leafCollides (traversal_node_octree.h:1053-1058) runs the octree-first query.  So
 * collide(solid, octree) returns the octree-first result UNSWAPPED: the tree's node in b1, the normal from the tree's box to the solid.
 * swapped[i] = 1 states that the caller's order was (solid, octree): bit 23 of the record's status is set and no other byte changes.
 *
 * Records (one hfcl_result per query; the conventions of hppfcl_amd_hfield.h):
 *   num_contacts   CollisionResult::numContacts()
 *   with a contact:    distance = the FIRST contact's penetration_depth; normal = its normal; p1, p2 = its nearest_points as the walk
 *                      REBUILDS them (Contact(o1, o2, b1, b2, pos, normal, depth), collision_data.h:126-136: pos -+ depth * normal / 2
 *                      with pos = (p1 + p2) / 2 of the solver's points -- not the solver's own points); b1 = the leaf's index in the
 *                      registered node array (the reference reports root1 - tree->getRoot(), a pointer difference between separately
 *                      allocated nodes, which cannot be reproduced), b2 = Contact::NONE (-1)
 *   without a contact: distance = CollisionResult::distance_lower_bound; normal, p1, p2 = the result's normal / nearest_points (the
 *                      solver's own, updateDistanceLowerBoundFromLeaf :1186-1197; NaN where no leaf lowered the bound); b1 = b2 = -1
 *   status         bit 7 the contact flag, bit 23 the caller's order was (solid, octree), bit 31 skipped (security_margin == -inf).  GJK /
 *                  EPA status and iteration fields are not reported: 0 and HFCL_EPA_DID_NOT_RUN are written.
 * distance_lower_bound (optional, n doubles): CollisionResult::distance_lower_bound of every query; DBL_MAX for a skipped query.
 * tf_octree / tf_shape are always the tree's and the solid's pose (12 doubles a row).
 * contacts: NULL, or room for max_contacts_total hfcl_contact records (pair = the query, b1 = the node, b2 = -1), in query order and
 * within a query in walk order; contacts beyond the capacity are counted in *n_contacts_out and dropped.  (The host form keeps the call's
 * list on the device: room for min(max_contacts_total, n * min(num_max_contacts, 2^26)) records.)
 *
 * Requests, all before any work.  num_max_contacts == 0: HFCL_ERR_INVALID_ARGUMENT; a finite negative security_margin:
 * HFCL_ERR_INVALID_ARGUMENT (OctreeCollide throws); security_margin == -inf: every record skipped (collision.cpp:73-76);
 * epa_max_iterations > 64: HFCL_ERR_LIMIT; gjk_initial_guess other than DefaultGuess (CachedGuess chains the solver's guess from leaf to
 * leaf, BoundingVolumeGuess changes the leaf set-up), or distance_upper_bound other than its default (DBL_MAX): HFCL_ERR_LIMIT.  A batch
 * that holds a solid without an evaluator (hfcl_octree_pair_supported) returns HFCL_ERR_UNSUPPORTED_PAIR, an octree or shape id
 * outside the library HFCL_ERR_INVALID_ARGUMENT (host form).  The device form cannot see the ids: there such a query gets a SKIPPED
 * record (status bit 31, every other field 0 but bit 23, bound DBL_MAX, no contacts) and the call returns HFCL_OK.  Without a device:
 * HFCL_ERR_NO_DEVICE, as every compute entry point.
 *
 * Not done: Plane and Halfspace against an octree (their local boxes are unbounded and the OBB conversion yields NaN centres);
 * octree x octree, x height field (x mesh: hppfcl_amd_octree_mesh.h); octrees as scene objects or environments; reading octomap's files; fp32 and hfcl_multi_*
 * forms; cached and bounding-volume GJK guesses; a finite distance_upper_bound.  (distance() against the same solids is in
 * hppfcl_amd_octree_distance.h: its pruning depends on the running minimum, so it is the reference's ordered walk, a query per lane
 * group, and not the route below.)
 *
 * Work on the device: the queries of a call go in chunks (option `octree_chunk`: queries per chunk, 0 = automatic; a chunk that lists
 * more (query, leaf) items than option `octree_items`, 0 = automatic: 2^20, is cut down, to one query at the least; records do not
 * depend on either; one query that lists more than 2^26 leaves: HFCL_ERR_LIMIT).  Per chunk: every query's walk is counted, the counts
 * scanned, the reached leaves listed in walk order with their boxes, every listed (query, leaf) item solved, and one replay per query
 * folds its items in order.  The device form waits on `stream` once per chunk for the item count (8 bytes; the item workspace is sized
 * by it) and once at the end when n_contacts_out is given; growing a workspace buffer frees the old one, which waits for the whole
 * device. */
#ifndef HPPFCL_AMD_OCTREE_H
#define HPPFCL_AMD_OCTREE_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HFCL_OCTREE_MAX_DEPTH 16u

typedef struct hfcl_octree_node {
  uint32_t child[8]; /* index of child i in the array; 0: none (node 0 is the root) */
  double occupancy;
} hfcl_octree_node; /* 40 bytes */

/* Host only */
int hfcl_octree_validate(const hfcl_octree_node* nodes, size_t n_nodes, uint32_t depth);
/* Host only.  xyz: n points, 3 doubles each */
int hfcl_octree_from_points(const double* xyz, size_t n, double resolution, uint32_t depth, hfcl_octree_node* nodes_out, size_t capacity,
                            size_t* n_nodes_out);
/* Validates and keeps a copy of the nodes (uploaded by the next collide call).  Returns the octree's index on the library, or -1.
 * The reference's defaults: occupancy_threshold = the octomap tree's own (0.5 unless set), free_threshold 0 (octree.h:66-87) */
int hfcl_lib_add_octree(hfcl_lib* lib, const hfcl_octree_node* nodes, size_t n_nodes, double resolution, uint32_t depth,
                        double occupancy_threshold, double free_threshold);
/* setOccupancyThres / setFreeThres.  Not while a call of this library is in flight */
int hfcl_lib_octree_set_thresholds(hfcl_lib* lib, int octree, double occupancy_threshold, double free_threshold);
size_t hfcl_lib_octree_count(const hfcl_lib* lib);
/* Forgets every registered octree (indices start at 0 again).  Not while a call of this library is in flight */
int hfcl_lib_clear_octrees(hfcl_lib* lib);
/* getRootBV: min xyz, max xyz = -+(1 << depth) * resolution / 2.  Host only */
int hfcl_octree_root_box(const hfcl_lib* lib, int octree, double* out6);
/* 1 for Box, Sphere, Capsule, Cone, Cylinder, Ellipsoid, Convex; 0 for everything else (Plane and Halfspace included) */
int hfcl_octree_pair_supported(int32_t node_type_of_solid);

int hfcl_octree_collide_batch(hfcl_lib* lib, const uint32_t* octree, const uint32_t* shape, const double* tf_octree, const double* tf_shape,
                              size_t n, const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out,
                              double* distance_lower_bound, hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out);
/* the same call on device pointers (n_contacts_out: host memory), asynchronous on `stream` but for the waits named above */
int hfcl_octree_collide_batch_device(hfcl_lib* lib, const uint32_t* d_octree, const uint32_t* d_shape, const double* d_tf_octree,
                                     const double* d_tf_shape, size_t n, const uint8_t* d_swapped, const hfcl_collision_request* req,
                                     hfcl_result* d_out, double* d_distance_lower_bound, hfcl_contact* d_contacts,
                                     size_t max_contacts_total, size_t* n_contacts_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_OCTREE_H */
