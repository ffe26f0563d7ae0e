/* hppfcl_amd_cull.h -- scene queries with the pair list culled per configuration on the device.  Part of the C ABI of
 * hppfcl_amd.h (which includes this file; the ABI version stays 5: the entry points below are additions).
 *
 * hfcl_scene_collide / hfcl_scene_distance run the narrow phase on every listed pair of every configuration.  A caller of the
 * reference never does: per configuration DynamicAABBTreeCollisionManager::collide(callback) invokes the callback only for pairs
 * whose world AABBs overlap (src/broadphase/broadphase_dynamic_AABB_tree.cpp:252-293; hfcl_broadphase_self_pairs restates it on
 * the host for one configuration).  The calls below do that test on the device, for every configuration of a pose table that is
 * already there: the flat query range q = c * n_pairs + p is compacted to the ascending list of the queries whose two world boxes
 * touch, and the scene calls run on that list.  The scene's pair list stays the set of candidates (a robot model's pairs, all
 * pairs of a few bodies); the unculled calls stay for callers whose list already is a broadphase result.
 *
 * Boxes.  One local box per library shape -- computeLocalAABB of the shape, the swept-sphere radius included; for a
 * BVHModel<OBBRSS> the box of the model's vertices (BVHModelBase::computeLocalAABB) -- is kept on the device.  The world box of
 * (configuration, object) is what hfcl_world_aabbs computes, bit for bit (CollisionObject::computeAABB: the translation alone
 * under an identity rotation, interval arithmetic otherwise); the _f32 forms widen the 7-float pose to double, rebuild the
 * rotation as hfcl_collide_batch_qt does and go on in double.  Boxes are always doubles.  Unbounded boxes (Plane, Halfspace) are
 * treated no differently.
 * The test.  A query survives when its two boxes touch after each was grown by `inflate` on every side (AABB::expand; inflate >= 0,
 * and 0 is the reference's manager): closed intervals as AABB::overlap, and a NaN keeps the pair.
 * The list.  Ascending, bitwise reproducible, independent of how the range is cut into chunks (option `scene_cull_chunk`, 0 =
 * automatic, at most 2^31; n_conf * n_pairs is not bounded by 2^32).  conf_begin[c], c = 0 .. n_conf, is the number of survivors with
 * q < c * n_pairs: configuration c owns the list entries conf_begin[c] .. conf_begin[c + 1].
 *
 * Request checks, HFCL_ERR_UNSUPPORTED_PAIR reporting (over the surviving records only), invalidation by hfcl_lib_set_shapes, the
 * workspace (the library's, grown on demand: a call that grows it waits for the device) and "calls on scenes of one library must
 * not overlap" are as for the unculled calls.  inflate < 0 or NaN: HFCL_ERR_INVALID_ARGUMENT before any work. */
#ifndef HPPFCL_AMD_CULL_H
#define HPPFCL_AMD_CULL_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* World boxes of every (configuration, object): aabbs_out holds n_conf * n_objects * 6 doubles (min xyz, max xyz).  Host arrays,
 * blocking; the _device forms take device pointers and are asynchronous on `stream`. */
int hfcl_scene_world_aabbs(hfcl_scene* s, const double* object_tf, size_t n_conf, double* aabbs_out);
int hfcl_scene_world_aabbs_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double* aabbs_out);
int hfcl_scene_world_aabbs_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, double* d_aabbs_out, void* stream);
int hfcl_scene_world_aabbs_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, double* d_aabbs_out, void* stream);

/* The cull alone.  Host arrays, blocking.  query_ids: NULL (count only) or `capacity` entries; conf_begin: NULL or n_conf + 1;
 * *n_listed is always set.  With query_ids != NULL and capacity < *n_listed: HFCL_ERR_LIMIT, nothing else written (never
 * truncates). */
int hfcl_scene_cull(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, uint64_t* query_ids, size_t capacity,
                    uint64_t* conf_begin, size_t* n_listed);
int hfcl_scene_cull_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, uint64_t* query_ids, size_t capacity,
                        uint64_t* conf_begin, size_t* n_listed);
/* Device pointers, asynchronous on `stream`; nothing is read back.  *d_n_listed (required) is the true count, ids at positions
 * >= capacity are not written: the caller compares the two.  d_query_ids: NULL (count only) or `capacity` entries; d_conf_begin:
 * NULL or n_conf + 1. */
int hfcl_scene_cull_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, double inflate, uint64_t* d_query_ids, size_t capacity,
                           uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream);
int hfcl_scene_cull_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, double inflate, uint64_t* d_query_ids,
                               size_t capacity, uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream);

/* The scene calls on a list of queries.  Record k -- and guess k, in and out -- is for query d_query_ids[k], and record k is byte
 * for byte what the unculled scene call writes at that q.  d_out: NULL or n_listed records; d_summary: NULL or n_conf (not both
 * NULL); d_conf_begin is required when d_summary is given.  The summary of configuration c is the fold over its list entries
 * (p = id - c * n_pairs); a configuration without entries gets min_distance = +inf, min_pair = first_contact = 0xFFFFFFFF, zero
 * counts.  The list goes through the batch entry points in chunks (option `scene_chunk`) as the unculled form does; the summaries
 * do not depend on the chunks.  THE LIST IS NOT CHECKED: the ids must be ascending and below n_conf * n_pairs, and d_conf_begin
 * must be theirs, as hfcl_scene_cull_device leaves them.  n_listed == 0: HFCL_OK, the summaries (if any) as above. */
int hfcl_scene_collide_listed_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const uint64_t* d_query_ids, size_t n_listed,
                                     const uint64_t* d_conf_begin, const hfcl_collision_request* req, hfcl_result* d_out,
                                     hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream);
int hfcl_scene_distance_listed_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const uint64_t* d_query_ids, size_t n_listed,
                                      const uint64_t* d_conf_begin, const hfcl_distance_request* req, hfcl_result* d_out,
                                      hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream);
int hfcl_scene_collide_listed_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const uint64_t* d_query_ids,
                                         size_t n_listed, const uint64_t* d_conf_begin, const hfcl_collision_request* req,
                                         hfcl_result_f32* d_out, hfcl_scene_summary* d_summary, void* stream);
int hfcl_scene_distance_listed_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const uint64_t* d_query_ids,
                                          size_t n_listed, const uint64_t* d_conf_begin, const hfcl_distance_request* req,
                                          hfcl_result_f32* d_out, hfcl_scene_summary* d_summary, void* stream);

/* Host convenience forms: the table crosses the link once, the cull runs, the count comes back (8 bytes, the one read-back before
 * the narrow phase), the list goes through the narrow phase in chunks whose records leave as those of hfcl_scene_collide do, the
 * summaries come back at the end.  out: NULL (summaries only: no record leaves the device) or out_capacity records; query_ids_out:
 * NULL or out_capacity; conf_begin_out: NULL or n_conf + 1; summary: NULL or n_conf (out and summary not both NULL); guess_in /
 * guess_out: NULL or one per list entry (guess_out: out_capacity).  *n_listed is set.  With out, guess_out or query_ids_out given
 * and out_capacity < *n_listed: HFCL_ERR_LIMIT before any narrow-phase work.  *n_listed == 0: HFCL_OK, the summaries those of
 * configurations without entries. */
int hfcl_scene_collide_culled(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, const hfcl_collision_request* req,
                              hfcl_result* out, size_t out_capacity, uint64_t* query_ids_out, uint64_t* conf_begin_out,
                              hfcl_scene_summary* summary, const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed);
int hfcl_scene_distance_culled(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, const hfcl_distance_request* req,
                               hfcl_result* out, size_t out_capacity, uint64_t* query_ids_out, uint64_t* conf_begin_out,
                               hfcl_scene_summary* summary, const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed);
int hfcl_scene_collide_culled_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, const hfcl_collision_request* req,
                                  hfcl_result_f32* out, size_t out_capacity, uint64_t* query_ids_out, uint64_t* conf_begin_out,
                                  hfcl_scene_summary* summary, size_t* n_listed);
int hfcl_scene_distance_culled_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, const hfcl_distance_request* req,
                                   hfcl_result_f32* out, size_t out_capacity, uint64_t* query_ids_out, uint64_t* conf_begin_out,
                                   hfcl_scene_summary* summary, size_t* n_listed);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_CULL_H */
