/* hppfcl_amd_hfield.h -- hpp::fcl::HeightField<AABB> (include/hpp/fcl/hfield.h) against convex solids: the tree builder, the
 * registration on a library and the batched collide(), in both operand orders, in fp64.  Part of the C ABI of hppfcl_amd.h (which
 * includes this file; the ABI version stays 5: the entry points below are additions).  hfcl_collide_batch*, hfcl_pair_supported and
 * the function matrices keep their answers: the HF node types stay unsupported THERE; height fields have the calls below.
 *
 * The geometry.  A height field is x_dim by y_dim, centred at the origin of its frame, with ny x nx heights (row-major: heights[y * nx + x])
 * over the grids  x_grid = LinSpaced(nx, -x_dim/2, +x_dim/2),  y_grid = LinSpaced(ny, +y_dim/2, -y_dim/2)  (y DESCENDING: row 0 is
 * the north edge).  Heights are clamped from below, max(h, min_height); the field is SOLID down to min_height.  LinSpaced is that of
 * Eigen >= 3.3: step = (high - low) / (n - 1), element i = low + i * step, the last element exactly `high` (both grids have
 * |high| == |low|, so Eigen's flipped form never applies).  Eigen is not part of this project's build or tests: the end points are
 * pinned by the reference's tests (test/hfields.cpp:72-77, 476-480), the last bit of the interior values is NOT checked against Eigen.
 *
 * The tree (HeightField::init / recursiveBuildTree, hfield.h:308-479), in the reference's numbering: node 0 is the root; the two
 * children of a node are appended at first_child, first_child + 1 when the node is visited (left subtree numbered before the right one
 * is entered); a node of x_size x y_size cells is split along x when x_size >= y_size, at size / 2; a node of 1 x 1 cells is a leaf
 * (first_child = 0).  2 * (nx-1) * (ny-1) - 1 nodes.  A node's box runs from (x_grid[x_id], y_grid[y_id], min_height) to
 * (x_grid[x_id + x_size], y_grid[y_id + y_size], max_height), min and max per component.  contact_active_faces of a leaf
 * (hfield.h:460-476): TOP = BOTTOM = 1 (they share the bit in the reference's enum; kept), NORTH = 2 (y_id == 0), EAST = 4 (last
 * column), SOUTH = 8 (last row), WEST = 16 (x_id == 0); 0 for inner nodes.
 *
 * Limits.  nx, ny >= 2 and every height finite, else HFCL_ERR_INVALID_ARGUMENT; a cell whose four clamped heights all equal min_height
 * is refused with HFCL_ERR_INVALID_ARGUMENT (the reference asserts max_height > min_height there); a side above 32 768 samples:
 * HFCL_ERR_LIMIT (the walk's stack holds 40 entries; such a tree is at most 30 levels deep).  A side triangle of a prism is degenerate
 * where a corner height equals min_height; the reference then reads an uninitialised projection (intersect.h:58-69) -- here such a
 * triangle is never the closest one (its distance counts as DBL_MAX).
 *
 * collide() (src/collision.cpp:69-129, HeightFieldShapeCollider, traversal_node_hfield_shape.h:514-654, collisionRecurse
 * traversal_recurse.cpp:44-85): inner nodes are box-tested against the solid's world AABB (computeBV<AABB, S>) with security_margin
 * and break_distance, leaves never; a leaf is two triangular prisms (buildConvexTriangles :121-232), each solved against the solid by
 * GJK / EPA with penetration (ShapeShapeDistance<Convex, S>), corrected by binCorrection (:321-400), combined (:456-508) and gated
 * (:621-639); left child before right; the walk stops when num_max_contacts contacts exist.
 *
 * Records (one hfcl_result per query; the conventions of the mesh x solid collide records):
 *   num_contacts   CollisionResult::numContacts()
 *   with a contact:    distance = the FIRST contact's penetration_depth; normal, p1, p2 = its normal and nearest_points;
 *                      b1 = the leaf's node index, b2 = Contact::NONE (-1)
 *   without a contact: distance = CollisionResult::distance_lower_bound; normal, p1, p2 = the result's normal / nearest_points
 *                      (NaN where the reference leaves them NaN: no leaf lowered the bound); b1 = b2 = -1
 *   status         bit 7 the contact flag, bit 23 the operands were swapped (below), bit 31 skipped (security_margin == -inf).  The GJK /
 *                  EPA status and iteration fields are NOT reported for these records: 0 and HFCL_EPA_DID_NOT_RUN are written.
 * distance_lower_bound (optional, n doubles): CollisionResult::distance_lower_bound of every query -- a record with a contact cannot
 * carry it.  DBL_MAX for a skipped query.
 * swapped: NULL, or n bytes; 1 = the query is collide(solid, hfield): computed as hfield x solid, then b1 / b2 and the nearest points
 * exchanged and the normal negated, in the record and in every contact (collision.cpp:92-108), bit 23 set.  tf_hfield / tf_shape are
 * always the height field's and the solid's pose (12 doubles a row, as everywhere in this ABI).
 * contacts: NULL, or room for max_contacts_total hfcl_contact records (pair = the query), in query order and within a query in the
 * reference's order; contacts beyond the capacity are counted in *n_contacts_out and dropped (the rule of hfcl_collide_batch_contacts).
 * (The host form keeps the call's list on the device: room for min(max_contacts_total, n * min(num_max_contacts, 2^26)) records, which
 * is all a call can produce.)
 *
 * Requests.  num_max_contacts == 0: HFCL_ERR_INVALID_ARGUMENT; epa_max_iterations > 64: HFCL_ERR_LIMIT; security_margin == -inf: every
 * record skipped; gjk_initial_guess other than DefaultGuess, or distance_upper_bound other than its default (DBL_MAX):
 * HFCL_ERR_LIMIT -- a cached guess chains from leaf to leaf inside one query and a finite upper bound turns leaf distances into
 * early-stopped bounds; both are left for later.  All of these before any work.  A batch that holds a solid without an evaluator
 * (hfcl_hfield_pair_supported) returns HFCL_ERR_UNSUPPORTED_PAIR, a height field or shape id outside the library
 * HFCL_ERR_INVALID_ARGUMENT (host form).  The device form cannot see the ids: there such a query -- an id outside the library's tables,
 * a solid without an evaluator -- gets a SKIPPED record (status bit 31, every other field 0 but the swap bit, bound DBL_MAX, no
 * contacts) and the call returns HFCL_OK; bit 31 in a device-form record therefore means "-inf margin" or "not a query this call
 * evaluates".  Without a device: HFCL_ERR_NO_DEVICE, as every compute entry point.
 *
 * Not done: HeightField<OBBRSS>; Plane and Halfspace against a height field (the reference has those rows); distance(); height field x
 * mesh / octree; cached and bounding-volume GJK guesses; a finite distance_upper_bound.
 *
 * Work on the device: the queries of a call go in chunks (option `hfield_chunk`: queries per chunk, 0 = automatic; a chunk that lists
 * more (query, leaf) items than option `hfield_items`, 0 = automatic: 2^20, is cut down, to one query at the least; records do not
 * depend on either; one query that lists more than 2^26 leaves: HFCL_ERR_LIMIT).  Per chunk: every query's walk is counted, the counts scanned, the visited leaves listed in walk order, every listed
 * (query, leaf) item solved, and one replay per query folds its items in order.  The device form waits on `stream` once per chunk for
 * the item count (8 bytes; the item workspace is sized by it) and once at the end when n_contacts_out is given; growing a workspace
 * buffer frees the old one, which waits for the whole device. */
#ifndef HPPFCL_AMD_HFIELD_H
#define HPPFCL_AMD_HFIELD_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HFCL_HFIELD_MAX_SIDE 32768u

enum { HFCL_HF_FACE_TOP = 1, HFCL_HF_FACE_BOTTOM = 1, HFCL_HF_FACE_NORTH = 2, HFCL_HF_FACE_EAST = 4, HFCL_HF_FACE_SOUTH = 8, HFCL_HF_FACE_WEST = 16 };

/* HFNode<AABB> (hfield.h:54-169) */
typedef struct hfcl_hfield_node {
  uint32_t first_child;            /* 0: a leaf */
  int32_t  x_id, x_size, y_id, y_size;
  int32_t  contact_active_faces;
  double   max_height;
  double   aabb_min[3], aabb_max[3];
} hfcl_hfield_node;                /* 80 bytes */

/* Host only.  nodes_out: room for 2 * (nx-1) * (ny-1) - 1 nodes, or NULL (the count alone); x_grid_out / y_grid_out: nx / ny doubles, or NULL */
int hfcl_hfield_build(double x_dim, double y_dim, const double* heights, size_t ny, size_t nx, double min_height,
                      hfcl_hfield_node* nodes_out, size_t* n_nodes_out, double* x_grid_out, double* y_grid_out);
/* Builds with the function above and uploads heights, grids and nodes.  Returns the height field's index on the library, or -1 */
int hfcl_lib_add_hfield(hfcl_lib* lib, double x_dim, double y_dim, const double* heights, size_t ny, size_t nx, double min_height);
size_t hfcl_lib_hfield_count(const hfcl_lib* lib);
/* Forgets every registered height field (indices start at 0 again; the device buffers are kept for the next registrations): what a
 * caller that registers a field again whenever its heights change calls now and then.  Not while a call of this library is in flight */
int hfcl_lib_clear_hfields(hfcl_lib* lib);
/* computeLocalAABB (hfield.h:278-287): min xyz, max xyz.  Host only */
int hfcl_hfield_local_aabb(const hfcl_lib* lib, int hfield, double* out6);
/* 1 for Box, Sphere, Capsule, Cone, Cylinder, Ellipsoid, Convex; 0 for everything else (Plane and Halfspace included) */
int hfcl_hfield_pair_supported(int32_t node_type_of_solid);

int hfcl_hfield_collide_batch(hfcl_lib* lib, const uint32_t* hfield, const uint32_t* shape, const double* tf_hfield, const double* tf_shape,
                              size_t n, const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out,
                              double* distance_lower_bound, hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out);
/* the same call on device pointers (n_contacts_out: host memory), asynchronous on `stream` but for the waits named above */
int hfcl_hfield_collide_batch_device(hfcl_lib* lib, const uint32_t* d_hfield, const uint32_t* d_shape, const double* d_tf_hfield,
                                     const double* d_tf_shape, size_t n, const uint8_t* d_swapped, const hfcl_collision_request* req,
                                     hfcl_result* d_out, double* d_distance_lower_bound, hfcl_contact* d_contacts,
                                     size_t max_contacts_total, size_t* n_contacts_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_HFIELD_H */
