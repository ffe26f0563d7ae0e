/* hppfcl_amd_pairs.h -- the self-collision pairs of a scene, made per configuration on the device, and the scene calls on such a list.
 * Part of the C ABI of hppfcl_amd.h (which includes this file; the ABI version stays 5: the entry points below are additions).
 *
 * Every other scene call starts from a pair list the caller fixed in advance.  A caller of the reference does not: per configuration
 * DynamicAABBTreeCollisionManager::collide(callback) finds the pairs whose world AABBs overlap itself.  hfcl_broadphase_self_pairs does
 * that on the host for one configuration; the calls below do it on the device for every configuration of a pose table that is already
 * there, without a list: a tiled test of all pairs of world boxes -- no tree, no sorting, no atomics --, compacted by count / scan / emit.
 * 5 * 10^9 box tests (100 000 objects) are milliseconds of the device's time; scenes far beyond that want a tree or a grid, which this is
 * not -- or the second way to the same list, sort and sweep along one axis, which the option `scene_pairs_sorted` chooses
 * (hppfcl_amd_pairs_sorted.h, included below: what it costs, and the one wait it adds to the device forms).
 *
 * The list.  Entry k is a pair (i, j), i < j, two uint32 object indices.  The list holds, for configuration c ascending, then i ascending,
 * then j ascending, every pair whose two world boxes touch after each was grown by `inflate` on every side.  The boxes are those of
 * hfcl_scene_world_aabbs, the test is the one of the cull (hppfcl_amd_cull.h: closed intervals, a NaN keeps the pair, unbounded Plane /
 * Halfspace boxes are treated no differently; inflate >= 0, and 0 is the reference's manager).  conf_begin[c], c = 0 .. n_conf, is the number
 * of entries of the configurations before c: configuration c owns the entries conf_begin[c] .. conf_begin[c + 1].  With inflate = 0 the
 * entries of configuration c are, entry for entry, what hfcl_broadphase_self_pairs(hfcl_world_aabbs(configuration c)) returns for boxes
 * without a NaN.  The scene's own pair list plays no part.  The bytes of the list do not depend on how the work is cut into launches:
 * option `scene_cull_chunk` is, for these calls, the rows (configuration, object) per chunk (0: automatic, 2^20), and scenes of at most
 * `scene_pairs_small_max` objects (default 32, at most 64) take a wave-per-configuration form of the same test.
 * Limits: n_objects <= 2^22 (HFCL_ERR_LIMIT beyond).  n_conf == 0 or n_objects < 2: HFCL_OK, count 0, conf_begin all zero.
 * Object groups and a group matrix (hppfcl_amd_groups.h: hfcl_scene_set_groups) leave of this list the pairs whose groups may pair --
 * a robot's links without their neighbours, a robot against an environment without environment x environment; none set: every pair.
 *
 * Without a HIP device every call below returns HFCL_ERR_NO_DEVICE.  inflate < 0 or NaN: HFCL_ERR_INVALID_ARGUMENT before any work.
 * Invalidation by hfcl_lib_set_shapes, the workspace (the library's, grown on demand: a call that grows it waits for the device) and
 * "calls on scenes of one library must not overlap" are as for the other scene calls. */
#ifndef HPPFCL_AMD_PAIRS_H
#define HPPFCL_AMD_PAIRS_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The list alone.  Host arrays, blocking.  pairs: NULL (count only) or 2 * capacity words; conf_begin: NULL or n_conf + 1; *n_listed is
 * always set.  With pairs != NULL and capacity < *n_listed: HFCL_ERR_LIMIT, nothing else written (never truncates). */
int hfcl_scene_self_pairs(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, uint32_t* pairs, size_t capacity,
                          uint64_t* conf_begin, size_t* n_listed);
int hfcl_scene_self_pairs_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, uint32_t* pairs, size_t capacity,
                              uint64_t* conf_begin, size_t* n_listed);
/* Device pointers, asynchronous on `stream`; nothing is read back.  *d_n_listed (required) is the true count, entries at positions
 * >= capacity are not written: the caller compares the two.  d_pairs: NULL (count only) or 2 * capacity words, 8-byte aligned;
 * d_conf_begin: NULL or n_conf + 1. */
int hfcl_scene_self_pairs_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, double inflate, uint32_t* d_pairs, size_t capacity,
                                 uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream);
int hfcl_scene_self_pairs_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, double inflate, uint32_t* d_pairs,
                                     size_t capacity, uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream);

/* The scene calls on such a list.  Record k -- and guess k, in and out -- is byte for byte what hfcl_collide_batch_device /
 * hfcl_distance_batch_device write for (object_shape[i_k], object_shape[j_k], tf[c][i_k], tf[c][j_k]), c the configuration whose conf_begin
 * span holds k.  Requests, refusals and the skipped-record rules are those of the _listed forms of hppfcl_amd_cull.h.  d_out: NULL or
 * n_listed records; d_summary: NULL or n_conf (not both NULL); d_conf_begin is required.  The summary of configuration c is the fold over
 * its entries, with min_pair and first_contact the entry's RANK inside the configuration, k - conf_begin[c]: the pair is
 * pairs[conf_begin[c] + rank].  A configuration without entries gets min_distance = +inf, min_pair = first_contact = 0xFFFFFFFF, zero
 * counts.  The list goes through the batch entry points in chunks (option `scene_chunk`); the summaries do not depend on the chunks.
 * Workspace of the summaries: the fold cuts a configuration's entries into pieces of 256 and keeps 24 bytes per piece and configuration,
 * for as many pieces as the LONGEST configuration could have -- min(n_listed, n_objects (n_objects - 1) / 2) entries, since the lengths
 * of the spans are known on the device only: n_conf * ceil(that / 256) * 24 bytes (nothing when that is at most 256).  Many
 * configurations of scenes of thousands of objects make this large (1000 x 5000 objects with 5 M entries: 470 MB); call per group of
 * configurations there.
 * THE LIST IS NOT CHECKED: i < j < n_objects, and d_conf_begin must be its spans (ascending, conf_begin[0] = 0, conf_begin[n_conf] =
 * n_listed), as hfcl_scene_self_pairs_device leaves them.  n_listed == 0: HFCL_OK, the summaries (if any) as above. */
int hfcl_scene_collide_pairs_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                    const uint64_t* d_conf_begin, const hfcl_collision_request* req, hfcl_result* d_out,
                                    hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream);
int hfcl_scene_distance_pairs_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                     const uint64_t* d_conf_begin, const hfcl_distance_request* req, hfcl_result* d_out,
                                     hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream);
int hfcl_scene_collide_pairs_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                        const uint64_t* d_conf_begin, const hfcl_collision_request* req, hfcl_result_f32* d_out,
                                        hfcl_scene_summary* d_summary, void* stream);
int hfcl_scene_distance_pairs_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                         const uint64_t* d_conf_begin, const hfcl_distance_request* req, hfcl_result_f32* d_out,
                                         hfcl_scene_summary* d_summary, void* stream);

/* Host convenience forms, shaped like hfcl_scene_collide_culled: the table crosses the link once; boxes, then pairs; the count comes
 * back (8 bytes, the one read-back before the narrow phase); the list goes through the narrow phase in chunks whose records leave as
 * those of hfcl_scene_collide do; the summaries come back at the end.  out: NULL (summaries only: no record leaves the device) or
 * out_capacity records; pairs_out: NULL or 2 * out_capacity words; conf_begin_out: NULL or n_conf + 1; summary: NULL or n_conf (out and
 * summary not both NULL); guess_in / guess_out: NULL or one per list entry (guess_out: out_capacity).  *n_listed is set.  With out,
 * guess_out or pairs_out given and out_capacity < *n_listed: HFCL_ERR_LIMIT before any narrow-phase work. */
int hfcl_scene_collide_self(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, const hfcl_collision_request* req,
                            hfcl_result* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out, hfcl_scene_summary* summary,
                            const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed);
int hfcl_scene_distance_self(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, const hfcl_distance_request* req,
                             hfcl_result* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out, hfcl_scene_summary* summary,
                             const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed);
int hfcl_scene_collide_self_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, const hfcl_collision_request* req,
                                hfcl_result_f32* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out,
                                hfcl_scene_summary* summary, size_t* n_listed);
int hfcl_scene_distance_self_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, const hfcl_distance_request* req,
                                 hfcl_result_f32* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out,
                                 hfcl_scene_summary* summary, size_t* n_listed);

#ifdef __cplusplus
}
#endif
#include "hppfcl_amd_pairs_sorted.h"
#endif /* HPPFCL_AMD_PAIRS_H */
