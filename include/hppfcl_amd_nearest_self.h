/* hppfcl_amd_nearest_self.h -- the clearance of a scene from the pose table and the object groups alone: per configuration the smallest
 * distance over every allowed pair of objects and the pair that has it, with the pairs made AND pruned on the device.  No pair list, no
 * `inflate`.  Part of the C ABI of hppfcl_amd.h (which includes this file; the ABI version stays 5: the entry points below are additions).
 *
 * In the reference this is DynamicAABBTreeCollisionManager::distance(otherManager, DistanceCallBackDefault).  It answers the question
 * hfcl_scene_distance answers on the explicit list P of every allowed pair in lexicographic order, and the one hfcl_scene_nearest
 * (hppfcl_amd_nearest.h) answers on P with its two pruned passes -- here without anybody keeping P.
 *
 * Candidates.  The candidates of configuration c are all (i, j), i < j < n_objects; with hfcl_scene_set_groups in force
 * (hppfcl_amd_groups.h) only those with bit group[j] of collides[group[i]] set.  The scene's own pair list plays no part.
 * The bound.  L(c, i, j) is the bound of hppfcl_amd_nearest.h from the two world boxes of hfcl_scene_world_aabbs, bit for bit:
 * r = 2^-40 (fp64 forms), 2^-18 (fp32 forms); -inf when the boxes touch or anything is not finite.  Nothing is inflated.
 * The passes.  seed[c] = the lexicographically lowest (i, j) attaining the smallest L of configuration c.  Pass 1 evaluates the
 * candidates with (L = -inf or (i, j) = seed[c]) and L <= upper_bound; thr[c] = min(upper_bound, min_distance of pass 1); pass 2
 * evaluates the candidates not in pass 1 with L <= thr[c].  Both lists are in (c, i, j) order with a conf_begin, exactly like a list
 * the self-pairs calls of hppfcl_amd_pairs.h make; their bytes do not depend on how the call is cut into chunks (options
 * `scene_cull_chunk` for the lists, `scene_chunk` for the narrow phase) or on which kernel form ran (`scene_pairs_small_max`).  Each
 * list goes through the narrow phase of hfcl_scene_distance_pairs_device with summaries of its own; the two are combined per
 * configuration: the smaller min_distance, on a tie the lower (i, j); the counts add up.
 *
 * What is promised.  Let P be the list of all candidates in lexicographic order.  Wherever the minimum of hfcl_scene_distance on P is
 * <= upper_bound: out[c].min_distance is that minimum bit for bit, (min_i, min_j) = P[min_pair], and min_records[c] is byte for byte
 * record c * |P| + min_pair of that call.  Elsewhere min_distance is some value > upper_bound, or +inf: it means only "farther than
 * upper_bound".  n_evaluated[0..1], out[c].n_evaluated and out[c].n_skipped equal what hfcl_scene_nearest on P reports: the same
 * bounds, the same predicates, the same tie rule.
 * What the equality rests on: every computed distance is >= L of its pair, i.e. the narrow phase returns the distance of the two shapes
 * or an upper estimate of it, up to the bound's slack.  That holds for converged GJK / EPA and for the mesh walks with
 * rel_err = abs_err = 0; a request that stops the solvers early (a small gjk_max_iterations, a loose gjk_tolerance) can leave a record
 * below the true distance by more than the slack, and the pruned answer may then differ from the unpruned one.
 *
 * Edge cases.  n_conf == 0: HFCL_OK.  n_objects < 2, or a configuration without a candidate or without an evaluated record that counts
 * (all skipped or NaN): min_distance = +inf, min_i = min_j = 0xFFFFFFFF, the counts of what was evaluated (zero when nothing was), a min
 * record with status bit 31 and distance = +inf.  A NaN upper_bound, a null `out` or a null request with a scene:
 * HFCL_ERR_INVALID_ARGUMENT before any work.  No device: HFCL_ERR_NO_DEVICE.  More than 2^22 objects, or a pass list one of whose
 * configurations could hold 2^32 entries: HFCL_ERR_LIMIT.
 * min_records: NULL, or n_conf records.  n_evaluated: NULL, or two counts: the pairs evaluated in pass 1 and in pass 2 (host memory in
 * the device forms too).
 *
 * Device forms: device pointers, enqueued on `stream` -- but the call waits on that stream twice, for the two list counts (8 bytes
 * each, the only read-backs; the host forms read back the same two).  The lists are sized by a guess (16 entries per configuration and
 * object) and a list that outgrows it is counted, scanned and emitted once more into a buffer of its size; growing a workspace buffer
 * frees the old one, which waits for the whole device.  As with the other device forms, pairs without an evaluator are not reported by
 * the return value.  The all-pairs sweep is walked five times (seeds, count and emit of each pass): where P fits in memory,
 * hfcl_scene_nearest on P does less work.
 * Request checks, HFCL_ERR_UNSUPPORTED_PAIR reporting (host forms, over the evaluated records only), invalidation by
 * hfcl_lib_set_shapes, the shared workspace and "calls on scenes of one library must not overlap" are as for the other scene calls. */
#ifndef HPPFCL_AMD_NEAREST_SELF_H
#define HPPFCL_AMD_NEAREST_SELF_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hfcl_scene_clearance {
  double   min_distance;     /* +inf: no evaluated record counts */
  uint32_t min_i, min_j;     /* the pair, i < j; 0xFFFFFFFF both when there is none */
  uint32_t n_evaluated;      /* records of this configuration the two passes evaluated */
  uint32_t n_skipped;        /* of those, the records with status bit 31 (as hfcl_scene_summary::n_skipped) */
} hfcl_scene_clearance;      /* 24 bytes */

int hfcl_scene_nearest_self(hfcl_scene* s, const double* object_tf, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                            hfcl_scene_clearance* out, hfcl_result* min_records, size_t* n_evaluated);
int hfcl_scene_nearest_self_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, const hfcl_distance_request* req,
                                double upper_bound, hfcl_scene_clearance* out, hfcl_result_f32* min_records, size_t* n_evaluated);
int hfcl_scene_nearest_self_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const hfcl_distance_request* req,
                                   double upper_bound, hfcl_scene_clearance* d_out, hfcl_result* d_min_records, size_t* n_evaluated,
                                   void* stream);
int hfcl_scene_nearest_self_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const hfcl_distance_request* req,
                                       double upper_bound, hfcl_scene_clearance* d_out, hfcl_result_f32* d_min_records,
                                       size_t* n_evaluated, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_NEAREST_SELF_H */
