/* hppfcl_amd_nearest.h -- the clearance of a scene: per configuration the smallest distance over the listed pairs and the pair that
 * has it, with the pairs pruned by a bound from their world boxes.  Part of the C ABI of hppfcl_amd.h (which includes this file; the
 * ABI version stays 5: the entry points below are additions).
 *
 * In the reference this is DynamicAABBTreeCollisionManager::distance with DistanceCallBackDefault, which skips every pair whose boxes
 * are already farther apart than the minimum found so far.  hfcl_scene_distance gives the same answer in
 * hfcl_scene_summary::min_distance / min_pair by running the narrow phase on every listed pair; the calls below give it by running
 * the narrow phase on a few per cent of them, in two passes over two lists.
 *
 * The bound.  For a query q = c * n_pairs + p with the world boxes a, b of its two objects (the table hfcl_scene_world_aabbs
 * computes, bit for bit):  g_k = max(a.min_k - b.max_k, b.min_k - a.max_k);  lb = sqrt((max(g_x,0)^2 + max(g_y,0)^2) + max(g_z,0)^2);
 * e = the sum of the two boxes' diagonal lengths; M = the largest absolute coordinate of the two boxes;
 *   L(q) = lb - (2e-10 * e + r * M),   r = 2^-40 (fp64 forms), 2^-18 (fp32 forms);
 *   L(q) = -inf when no g_k > 0 (the boxes touch: closed intervals) or when anything above is not finite (NaN poses, the +-DBL_MAX
 *   boxes of Plane and Halfspace).
 * The 2e-10 * e term covers the 1 + 1e-10 inflation of Box, Cone and Cylinder supports, the r * M term the rounding of the narrow phase.
 * The passes.  seed[c] = the lowest p attaining the smallest L of configuration c.  Pass 1 evaluates the queries with
 * (L = -inf or p = seed[c]) and L <= upper_bound; thr[c] = min(upper_bound, min_distance of pass 1); pass 2 evaluates the queries not
 * in pass 1 with L <= thr[c] and merges into the same summaries.  Both lists are ascending and do not depend on the chunking (options
 * `scene_cull_chunk` for the lists, `scene_chunk` for the narrow phase, as in hppfcl_amd_cull.h).
 *
 * Summary fields.  min_distance / min_pair equal those of hfcl_scene_distance whenever that minimum is <= upper_bound (a pair attaining
 * the minimum d has L <= d <= thr[c] and is evaluated, as is every lower-indexed pair attaining it; the records of a listed call are
 * byte for byte the unculled records).  first_contact, n_contacts and n_skipped are folds over the EVALUATED records only.
 * What the equality rests on: every computed distance is >= L of its query, i.e. the narrow phase returns the distance of the two
 * shapes or an upper estimate of it, up to the slack above.  That holds for converged GJK / EPA and for the mesh walks with
 * rel_err = abs_err = 0; a request that stops the solvers early (a small gjk_max_iterations, a loose gjk_tolerance) can leave a
 * record below the true distance by more than the slack, and the pruned answer may then differ from the unculled one.
 * Unculled minimum above upper_bound: min_distance is then some value > upper_bound, or +inf -- it means only "farther than
 * upper_bound".  upper_bound = +inf is the manager's starting value.
 * Configuration without records.  A configuration with no evaluated record whose value counts (none listed, all skipped or NaN) gets
 * min_distance = +inf, min_pair = first_contact = 0xFFFFFFFF; its min record has status bit 31 and distance = +inf.
 * min_records: NULL, or n_conf records -- record c is the record of query c * n_pairs + min_pair, byte for byte the unculled one.
 * n_evaluated: NULL, or two counts: the queries evaluated in pass 1 and in pass 2 (host memory in the device forms too).
 *
 * Device forms: device pointers, enqueued on `stream` -- but the call waits on that stream twice, for the two list counts (8 bytes
 * each, the only read-backs; the host forms read back the same two).  Workspace: the world boxes of the WHOLE table
 * (n_conf * n_objects * 48 bytes) are resident during a call, whatever `scene_cull_chunk` is; the lists are sized by a guess (an eighth
 * of the queries) and a list that outgrows it is marked, scanned and emitted once more into a larger buffer; growing a workspace buffer
 * (the first call, a larger table, a longer list, min records) frees the old one, which waits for the whole device.  As with the other device forms, pairs without an evaluator are
 * not reported by the return value.
 * Request checks, HFCL_ERR_UNSUPPORTED_PAIR reporting (host forms, over the evaluated records only), invalidation by
 * hfcl_lib_set_shapes, the shared workspace and "calls on scenes of one library must not overlap" are as for the culled calls;
 * n_pairs == 0 or n_conf == 0: HFCL_OK, the summaries (and min records) of configurations without records.  A NaN upper_bound or a
 * null summary: HFCL_ERR_INVALID_ARGUMENT before any work. */
#ifndef HPPFCL_AMD_NEAREST_H
#define HPPFCL_AMD_NEAREST_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

int hfcl_scene_nearest(hfcl_scene* s, const double* object_tf, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                       hfcl_scene_summary* summary, hfcl_result* min_records, size_t* n_evaluated);
int hfcl_scene_nearest_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                           hfcl_scene_summary* summary, hfcl_result_f32* min_records, size_t* n_evaluated);
int hfcl_scene_nearest_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const hfcl_distance_request* req,
                              double upper_bound, hfcl_scene_summary* d_summary, hfcl_result* d_min_records, size_t* n_evaluated,
                              void* stream);
int hfcl_scene_nearest_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const hfcl_distance_request* req,
                                  double upper_bound, hfcl_scene_summary* d_summary, hfcl_result_f32* d_min_records, size_t* n_evaluated,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_NEAREST_H */
