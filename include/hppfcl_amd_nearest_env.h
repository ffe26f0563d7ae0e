/* hppfcl_amd_nearest_env.h -- the clearance of the moving objects of a scene among an environment kept on the device: per configuration
 * the smallest distance over every allowed pair that has a moving object in it, and the pair that has it, with the pairs made AND pruned
 * on the device from a pose table of the moving objects alone.  No pair list, no `inflate`, no row of the table for an obstacle.
 * Part of the C ABI of hppfcl_amd.h (which includes this file; the ABI version stays 5: the entry points below are additions).
 *
 * In the reference this is DynamicAABBTreeCollisionManager::distance(otherManager, DistanceCallBackDefault) of a robot's manager against
 * the manager of the standing obstacles, together with the robot's own distance(DistanceCallBackDefault).  It is hfcl_scene_nearest_self
 * (hppfcl_amd_nearest_self.h) for a scene with an environment (hppfcl_amd_env.h: hfcl_scene_set_environment*): the call takes a
 * (n_conf, n_moving, W) table, the environment's rows, boxes and one box per tile of 256 environment objects stay on the device.
 *
 * Full table.  The full table of configuration c is moving[c] (n_moving rows) followed by the environment's rows.
 * Candidates.  The candidates of configuration c are the pairs (i, j) with i < n_moving and i < j < n_objects; with
 * hfcl_scene_set_groups in force (hppfcl_amd_groups.h) only those with bit group[j] of collides[group[i]] set.  Environment x
 * environment pairs are never candidates.  The scene's own pair list plays no part.  P_env is the list of the candidates in
 * lexicographic order.
 * The bound.  L(c, i, j) is the bound of hppfcl_amd_nearest.h from the two world boxes of hfcl_scene_world_aabbs on the full table, bit
 * for bit: r = 2^-40 (fp64 forms), 2^-18 (fp32 forms); -inf when the boxes touch or anything is not finite.  Nothing is inflated.
 * The passes.  seed[c] = the lexicographically lowest (i, j) attaining the smallest L of configuration c.  Pass 1 evaluates the
 * candidates with (L = -inf or (i, j) = seed[c]) and L <= upper_bound; thr[c] = min(upper_bound, min_distance of pass 1); pass 2
 * evaluates the candidates not in pass 1 with L <= thr[c].  Both lists are in (c, i, j) order with a conf_begin, exactly like a list
 * hfcl_scene_env_pairs* makes; their bytes do not depend on how the call is cut (options `scene_cull_chunk`: moving rows per chunk,
 * `scene_env_span`: column tiles per workgroup, `scene_chunk` for the narrow phase) or on whether whole tiles were dropped by distance
 * (option `scene_nearest_env_prune`, below).  Each list goes through the narrow phase of hfcl_scene_distance_env_pairs_device with
 * summaries of its own; the two are combined per configuration: the smaller min_distance, on a tie the lower (i, j); the counts add up.
 *
 * What is promised.  Wherever the minimum of hfcl_scene_distance on P_env (full table) is <= upper_bound: out[c].min_distance is that
 * minimum bit for bit, (min_i, min_j) = P_env[min_pair], and min_records[c] is byte for byte record c * |P_env| + min_pair of that call.
 * Elsewhere min_distance is some value > upper_bound, or +inf: it means only "farther than upper_bound".  n_evaluated[0..1],
 * out[c].n_evaluated and out[c].n_skipped equal what hfcl_scene_nearest on P_env reports: the same bounds, the same predicates, the same
 * tie rule.  The same clearances, records and counts come from hfcl_scene_nearest_self on the full table when its groups forbid exactly
 * the environment x environment pairs on top of the caller's groups.
 * What the equality rests on: every computed distance is >= L of its pair, as in hppfcl_amd_nearest_self.h (converged GJK / EPA, mesh
 * walks with rel_err = abs_err = 0).
 *
 * Tiles dropped by distance.  A workgroup holds 16 moving rows of a configuration.  For an environment tile it computes Lt, a lower
 * bound of L(i, j) over every row i it holds and every member j of the tile, from the union of its rows' boxes, the tile's box, the
 * largest diagonal and the largest |coordinate| of either side -- the operations of the bound in their order, each monotone under
 * rounding.  Lt = -inf when a member or a row coordinate is not finite, when the tile's box touches the union, or when a coordinate
 * exceeds 2^500; a finite Lt also says that no pair of the cell has L = -inf.  Pass 1 skips the tile when Lt > -inf and seed[c] is not (a
 * row of the workgroup, a column of the tile); pass 2 skips it when Lt > thr[c]; the seeds skip by groups only; moving tiles are never
 * dropped by distance.  A skipped tile holds no pair of the pass: skipping changes time and never a byte.  Option
 * `scene_nearest_env_prune` (default 1): 0 drops no tile by distance.  As with the env lists the tile boxes only help when consecutive
 * environment objects are neighbours in space.  hfcl_scene_set_environment* leaves the per-box and per-tile terms of the bound on the
 * device beside the boxes (16 bytes a box, 16 a tile); a second set call replaces them.
 *
 * Errors, before any work: a NaN upper_bound, a null `out` or a null request with a scene: HFCL_ERR_INVALID_ARGUMENT.  No environment
 * set: HFCL_ERR_INVALID_ARGUMENT; one set in the other precision: HFCL_ERR_INVALID_ARGUMENT with the message of the env calls.  No device:
 * HFCL_ERR_NO_DEVICE.  n_moving > 2^22 or n_env > 2^22, or a pass list one of whose configurations could hold 2^32 entries:
 * HFCL_ERR_LIMIT.
 * Edge cases.  n_conf == 0: HFCL_OK.  n_moving == 0, or a configuration without a candidate or without an evaluated record that counts:
 * min_distance = +inf, min_i = min_j = 0xFFFFFFFF, the counts of what was evaluated (zero when nothing was), a min record with status
 * bit 31 and distance = +inf -- the "no record" answers of hfcl_scene_nearest_self.
 * min_records: NULL, or n_conf records.  n_evaluated: NULL, or two counts: the pairs evaluated in pass 1 and in pass 2 (host memory in
 * the device forms too).
 *
 * Device forms: device pointers, enqueued on `stream` -- but the call waits on that stream twice, for the two list counts (8 bytes
 * each, the only read-backs; the host forms read back the same two).  The lists are sized by a guess (16 entries per configuration and
 * moving object) and a list that outgrows it is counted, scanned and emitted once more into a buffer of its size; growing a workspace
 * buffer frees the old one, which waits for the whole device.  Nothing of the size of the full table is ever allocated: the workspace
 * holds the boxes of a chunk's moving rows and 16 bytes per (configuration, moving row, span).  As with the other device forms, pairs
 * without an evaluator are not reported by the return value.
 * Request checks, HFCL_ERR_UNSUPPORTED_PAIR reporting (host forms, over the evaluated records only), invalidation by
 * hfcl_lib_set_shapes, the shared workspace and "calls on scenes of one library must not overlap" are as for the other scene calls. */
#ifndef HPPFCL_AMD_NEAREST_ENV_H
#define HPPFCL_AMD_NEAREST_ENV_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The signatures of hfcl_scene_nearest_self* with a (n_conf, n_moving, W) table; the output is hfcl_scene_clearance, unchanged. */
int hfcl_scene_nearest_env(hfcl_scene* s, const double* moving_tf, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                           hfcl_scene_clearance* out, hfcl_result* min_records, size_t* n_evaluated);
int hfcl_scene_nearest_env_f32(hfcl_scene* s, const float* moving_pose, size_t n_conf, const hfcl_distance_request* req,
                               double upper_bound, hfcl_scene_clearance* out, hfcl_result_f32* min_records, size_t* n_evaluated);
int hfcl_scene_nearest_env_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, const hfcl_distance_request* req,
                                  double upper_bound, hfcl_scene_clearance* d_out, hfcl_result* d_min_records, size_t* n_evaluated,
                                  void* stream);
int hfcl_scene_nearest_env_device_f32(hfcl_scene* s, const float* d_moving_pose, size_t n_conf, const hfcl_distance_request* req,
                                      double upper_bound, hfcl_scene_clearance* d_out, hfcl_result_f32* d_min_records,
                                      size_t* n_evaluated, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_NEAREST_ENV_H */
