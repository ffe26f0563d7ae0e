/* hppfcl_amd_terrain.h -- a height-field terrain under the moving objects of a scene: one HeightField<AABB> of the scene's library at
 * one pose, a list of the objects that are tested against it, and a call that answers, for a whole table of configurations,
 * DynamicAABBTreeCollisionManager::collide(CollisionObject* terrain, CollisionCallBackDefault) -- or the loop of
 * collide(hfield, tf, link, tf_link) over a robot's links.  Part of the C ABI of hppfcl_amd.h (which includes this file; the ABI version
 * stays 5: the entry points below are additions).  No new options: `hfield_chunk` and `hfield_items` (hppfcl_amd_hfield.h) govern these
 * calls too.  fp64 only, as height fields are.
 *
 * The terrain.  A scene has at most one: hfcl_scene_set_terrain replaces what was set (a caller who registers an updated field again
 * moves on to it this way).  `hfield` is an index of hfcl_lib_add_hfield on the scene's library, tf_terrain its pose (12 doubles, a row
 * as everywhere in this ABI).  `objects`: n_terrain_objects strictly ascending object indices -- the links tested against the ground --,
 * or NULL: every object in [0, hfcl_scene_n_moving(s)) at the time of the call (n_terrain_objects is not read then).  An index outside
 * the scene or a list that does not ascend: HFCL_ERR_INVALID_ARGUMENT; a listed object whose shape has no evaluator
 * (hfcl_hfield_pair_supported is 0: meshes, Plane, Halfspace, TriangleP): HFCL_ERR_UNSUPPORTED_PAIR.  An empty list is legal.  The list
 * and the pose go to the device once.
 *
 * The query.  moving_tf is the table every _env call takes: (n_conf, n_rows, 12) doubles with n_rows = hfcl_scene_n_moving(s) -- that
 * is the scene's objects when no environment is set.  With n_t listed objects o_0 < ... < o_{n_t-1}, query q = c * n_t + k is
 *     collide(hfield, tf_terrain, object_shape[o_k], moving_tf[c][o_k]).
 * out[q], bounds[q] and the contacts of query q (hfcl_contact::pair = q, in query order, contacts beyond max_contacts_total counted in
 * *n_contacts_out and dropped) are byte for byte what hfcl_hfield_collide_batch_device writes for that explicit query with
 * swapped = NULL, whatever `hfield_chunk` and `hfield_items` are.  out, bounds, summary and contacts may each be NULL (all of them and
 * n_contacts_out NULL: HFCL_ERR_INVALID_ARGUMENT); without `out` no buffer of n_conf * n_t records exists anywhere: a call that asks
 * for summaries alone keeps a bound and a status word per query besides the buffers of a chunk.
 *
 * summary[c] (hfcl_scene_summary, 24 bytes) folds the n_t queries of configuration c, and can be recomputed exactly from the records
 * and bounds:
 *   min_distance   the smallest bounds[q] (CollisionResult::distance_lower_bound: a record with a contact cannot carry it) over the
 *                  queries that are not skipped (status bit 31) and whose bound is not NaN; +inf if there is none
 *   min_pair       the lowest OBJECT INDEX o_k that attains it (0xFFFFFFFF if none)
 *   first_contact  the lowest object index whose record has the contact flag (0xFFFFFFFF if none)
 *   n_contacts     the records with the flag; > 0 is isCollision() of the default callback
 *   n_skipped      the records with bit 31
 *
 * Before any work: the request checks of hfcl_hfield_collide_batch* with their return codes; no terrain set, a height-field index
 * that is no longer on the library (hfcl_lib_clear_hfields), a listed object >= the current hfcl_scene_n_moving (an environment set
 * after the terrain): HFCL_ERR_INVALID_ARGUMENT; n_conf == 0: HFCL_OK; n_conf * n_t > 2^32 - 16: HFCL_ERR_LIMIT.  A scene made before
 * the last hfcl_lib_set_shapes is refused as by every scene call.  Without a device: HFCL_ERR_NO_DEVICE.
 *
 * Work on the device, per chunk of queries: one kernel writes the four per-query arrays of the height-field call (field id, shape id,
 * the terrain's pose, the object's pose gathered from the table) into a workspace the scene owns, sized by the chunk; the chunk goes
 * through the height-field call's own driver (same kernels, same launches); its status words are kept.  After the last chunk one wave
 * per configuration folds the kept bounds and status words.  The device form waits on `stream` where
 * hfcl_hfield_collide_batch_device does: once per chunk, and once more for the count when n_contacts_out is given. */
#ifndef HPPFCL_AMD_TERRAIN_H
#define HPPFCL_AMD_TERRAIN_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

int    hfcl_scene_set_terrain(hfcl_scene* s, uint32_t hfield, const double* tf_terrain /* 12 */,
                              const uint32_t* objects, size_t n_terrain_objects);
int    hfcl_scene_clear_terrain(hfcl_scene* s);
size_t hfcl_scene_n_terrain_objects(const hfcl_scene* s);          /* 0: none set, or null scene */
int    hfcl_scene_collide_terrain(hfcl_scene* s, const double* moving_tf, size_t n_conf, const hfcl_collision_request* req,
                                  hfcl_result* out, double* bounds, hfcl_scene_summary* summary,
                                  hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out);
/* the same call on device pointers (n_contacts_out: host memory), asynchronous on `stream` but for the waits named above */
int    hfcl_scene_collide_terrain_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, const hfcl_collision_request* req,
                                         hfcl_result* d_out, double* d_bounds, hfcl_scene_summary* d_summary,
                                         hfcl_contact* d_contacts, size_t max_contacts_total, size_t* n_contacts_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_TERRAIN_H */
