/* hppfcl_amd_env.h -- a static environment kept on the device, and the scene calls that take the moving objects' poses alone.
 * Part of the C ABI of hppfcl_amd.h (which includes this file; the ABI version stays 5: the entry points below are additions).
 *
 * Every other scene call takes a pose table of (n_conf, n_objects, W) rows, so a robot among obstacles repeats the obstacles' rows in every
 * configuration.  A scene with an environment knows that part of it stands still: the poses of objects [n_moving, n_objects) are set once
 * and stay on the device with their world boxes and one box per tile of PAIRS_TILE = 256 consecutive environment objects; the calls below
 * take a table of (n_conf, n_moving, W) rows.  Nothing else changes: every other call, with or without an environment set, takes its full
 * table, runs the kernels it ran and writes the bytes it wrote.
 *
 * The environment.  hfcl_scene_set_environment{,_f32}(scene, n_moving, poses): 0 <= n_moving <= n_objects (HFCL_ERR_INVALID_ARGUMENT
 * beyond); n_env = n_objects - n_moving rows of 12 doubles (_f32: 7 floats), the row formats of the pose tables; NULL only with n_env == 0,
 * which is legal.  The rows are copied to the device once and the call blocks.  A scene has one environment: either setter replaces it.
 * The precision of the setter is the precision of the _env calls that may follow: a call of the other precision returns
 * HFCL_ERR_INVALID_ARGUMENT with a message that says so -- the two pose formats are not converted into each other.  The set call computes
 * the environment's world boxes with the kernel of hfcl_scene_world_aabbs*: they are bit for bit the boxes that call gives for the
 * environment's rows of a full table (of the library's shapes and meshes at the time of the set call).  hfcl_scene_clear_environment drops
 * it; hfcl_scene_n_moving is n_objects when none is set (0 for a null scene).  hfcl_scene_environment_aabbs reads back the n_env x 6 boxes
 * and the ceil(n_env / 256) x 6 tile boxes; either output may be NULL.
 *
 * Tile boxes.  Tile t holds the environment objects [256 t, 256 (t + 1)), counted from the first environment object: the tile edges do
 * not move with n_moving.  Per coordinate the tile's min is the min over its members' mins and its max the max over their maxes, folded in
 * member order from +inf / -inf (m = x < m ? x : m; M = x > M ? x : M); a NaN member coordinate makes that coordinate -inf (a min) or +inf
 * (a max).  That is conservative under the test of the lists (hppfcl_amd_cull.h: six comparisons, each false on a NaN): a tile is skipped
 * only if its box, grown by `inflate` with the subtraction and addition its members get, does not touch the union -- same rule -- of the
 * grown boxes of the 16 rows a workgroup holds, so a skipped tile holds no listed pair.  Skipping changes time, never bytes.  Unbounded
 * Plane / Halfspace boxes need no special case.  The tile boxes only help when consecutive environment objects are neighbours in space:
 * put the moving objects first and the environment in a spatial order (the Python layer's engine.spatial_order: Morton codes).
 *
 * The full table and the list.  The full table of configuration c is moving[c] (n_moving rows) followed by the environment's rows.  The
 * env list of a call is, entry for entry, the list hfcl_scene_self_pairs* gives for the full tables with the same `inflate` and the same
 * groups (if hfcl_scene_set_groups was called), minus every entry with i >= n_moving; conf_begin is recounted after that removal.  So the
 * list holds moving x moving pairs (i < j < n_moving) and moving x environment pairs, never environment x environment pairs; order is c,
 * then i, then j ascending, j an index into the full scene.  The bytes do not depend on how the call is cut into launches: option
 * `scene_cull_chunk` is, for these calls, the moving rows per chunk, option `scene_env_span` the column tiles per workgroup (0: automatic).
 * Count-only calls, the capacity rules (HFCL_ERR_LIMIT in the host form, never a truncated list; nothing written at or beyond `capacity`
 * and the true count in *d_n_listed in the device form), the checks of `inflate` and n_conf == 0 are those of hfcl_scene_self_pairs*
 * (hppfcl_amd_pairs.h).  Without an environment set: HFCL_ERR_INVALID_ARGUMENT.  n_moving == 0: HFCL_OK, an empty list.
 * Limits: n_moving <= 2^22 and n_env <= 2^22 (HFCL_ERR_LIMIT beyond).
 *
 * Without a HIP device every call below but hfcl_scene_n_moving returns HFCL_ERR_NO_DEVICE.  Invalidation by hfcl_lib_set_shapes, the
 * workspace and "calls on scenes of one library must not overlap" are as for the other scene calls. */
#ifndef HPPFCL_AMD_ENV_H
#define HPPFCL_AMD_ENV_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

int hfcl_scene_set_environment(hfcl_scene* s, size_t n_moving, const double* env_tf);
int hfcl_scene_set_environment_f32(hfcl_scene* s, size_t n_moving, const float* env_pose);
int hfcl_scene_clear_environment(hfcl_scene* s);
size_t hfcl_scene_n_moving(const hfcl_scene* s);
/* aabbs_out: NULL or n_env x 6; tile_aabbs_out: NULL or ceil(n_env / 256) x 6.  No environment set: HFCL_ERR_INVALID_ARGUMENT. */
int hfcl_scene_environment_aabbs(hfcl_scene* s, double* aabbs_out, double* tile_aabbs_out);

/* The list alone: the signatures and rules of hfcl_scene_self_pairs* with a (n_conf, n_moving, W) table. */
int hfcl_scene_env_pairs(hfcl_scene* s, const double* moving_tf, size_t n_conf, double inflate, uint32_t* pairs, size_t capacity,
                         uint64_t* conf_begin, size_t* n_listed);
int hfcl_scene_env_pairs_f32(hfcl_scene* s, const float* moving_pose, size_t n_conf, double inflate, uint32_t* pairs, size_t capacity,
                             uint64_t* conf_begin, size_t* n_listed);
int hfcl_scene_env_pairs_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, double inflate, uint32_t* d_pairs, size_t capacity,
                                uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream);
int hfcl_scene_env_pairs_device_f32(hfcl_scene* s, const float* d_moving_pose, size_t n_conf, double inflate, uint32_t* d_pairs,
                                    size_t capacity, uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream);

/* The narrow phase on such a list: the contracts of hfcl_scene_*_pairs_device* (hppfcl_amd_pairs.h) word for word -- records and guesses
 * byte for byte the per-pair batch calls', summaries by rank inside the configuration, THE LIST IS NOT CHECKED (i < n_moving, i < j <
 * n_objects), d_conf_begin required -- with the pose row of j >= n_moving taken from the environment.  The summaries' workspace bound uses
 * the longest possible configuration, min(n_listed, n_moving (n_moving - 1) / 2 + n_moving * n_env) entries. */
int hfcl_scene_collide_env_pairs_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                        const uint64_t* d_conf_begin, const hfcl_collision_request* req, hfcl_result* d_out,
                                        hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream);
int hfcl_scene_distance_env_pairs_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                         const uint64_t* d_conf_begin, const hfcl_distance_request* req, hfcl_result* d_out,
                                         hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream);
int hfcl_scene_collide_env_pairs_device_f32(hfcl_scene* s, const float* d_moving_pose, size_t n_conf, const uint32_t* d_pairs,
                                            size_t n_listed, const uint64_t* d_conf_begin, const hfcl_collision_request* req,
                                            hfcl_result_f32* d_out, hfcl_scene_summary* d_summary, void* stream);
int hfcl_scene_distance_env_pairs_device_f32(hfcl_scene* s, const float* d_moving_pose, size_t n_conf, const uint32_t* d_pairs,
                                             size_t n_listed, const uint64_t* d_conf_begin, const hfcl_distance_request* req,
                                             hfcl_result_f32* d_out, hfcl_scene_summary* d_summary, void* stream);

/* Host convenience forms, shaped like hfcl_scene_*_self: the moving table crosses the link once; boxes, then the list; the count comes
 * back (8 bytes); the list goes through the narrow phase in chunks; the summaries come back at the end.  Outputs and HFCL_ERR_LIMIT as
 * for hfcl_scene_*_self. */
int hfcl_scene_collide_env(hfcl_scene* s, const double* moving_tf, size_t n_conf, double inflate, const hfcl_collision_request* req,
                           hfcl_result* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out, hfcl_scene_summary* summary,
                           const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed);
int hfcl_scene_distance_env(hfcl_scene* s, const double* moving_tf, size_t n_conf, double inflate, const hfcl_distance_request* req,
                            hfcl_result* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out, hfcl_scene_summary* summary,
                            const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed);
int hfcl_scene_collide_env_f32(hfcl_scene* s, const float* moving_pose, size_t n_conf, double inflate, const hfcl_collision_request* req,
                               hfcl_result_f32* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out,
                               hfcl_scene_summary* summary, size_t* n_listed);
int hfcl_scene_distance_env_f32(hfcl_scene* s, const float* moving_pose, size_t n_conf, double inflate, const hfcl_distance_request* req,
                                hfcl_result_f32* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out,
                                hfcl_scene_summary* summary, size_t* n_listed);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_ENV_H */
