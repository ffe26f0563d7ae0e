/* hppfcl_amd_groups.h -- object groups and a group matrix for the pair lists a scene makes on the device.
 * Part of the C ABI of hppfcl_amd.h (which includes this file; the ABI version stays 5: the entry points below are additions).
 *
 * hfcl_scene_self_pairs* and hfcl_scene_*_self (hppfcl_amd_pairs.h) list EVERY pair i < j whose world boxes touch.  A planner wants
 * fewer: a robot's neighbouring links always touch, and the objects of one static environment are never tested against each other --
 * a caller of the reference keeps two managers and calls DynamicAABBTreeCollisionManager::collide(otherManager, callback).  What
 * collision libraries call an allowed-collision matrix or collision groups says both: every object of a scene belongs to a group
 * (at most 64 groups), and a symmetric group matrix says which groups may pair.
 *
 * With groups set, the list of hfcl_scene_self_pairs{,_f32,_device,_device_f32} and of hfcl_scene_{collide,distance}_self{,_f32} holds,
 * in the same (c, i, j) order and with conf_begin counted accordingly, exactly those entries of the list without groups for which bit
 * object_group[j] of collides[object_group[i]] is set -- two objects of one group g included: listed iff bit g of collides[g] is set.
 * inflate, NaN, unbounded boxes, capacity, count-only, the independence of the chunks, the limits and the rank rule of the summaries are
 * unchanged; without groups every call writes the bytes it wrote before.  The hfcl_scene_*_pairs_device* forms take a list and are not
 * affected; neither are the scene's own pair list, the cull and hfcl_scene_nearest*.
 * Two identities:
 *  - a matrix of all ones (any assignment of groups) gives the list without groups, byte for byte;
 *  - groups 0 = objects [0, n_a), 1 = [n_a, n) with collides = {0b10, 0b01}: the entries of configuration c are, entry for entry,
 *    hfcl_broadphase_pairs_between(boxes[c][0 .. n_a), boxes[c][n_a .. n)) with n_a added to every j -- what
 *    collide(otherManager, callback) hands to a CollisionCallBackCollect.
 * The all-pairs sweep does not look at what the matrix rules out wholesale: per tile of 256 consecutive objects the scene keeps the set
 * of groups present, and a block of 16 consecutive rows skips every column tile none of whose groups may pair with any of its rows'
 * (and leaves at once when its rows may pair with nothing).  So order the objects by group where that is possible -- robot first,
 * environment second: the environment x environment part of the box tests is then never done.
 *
 * Without a HIP device every call below returns HFCL_ERR_NO_DEVICE; a null scene: HFCL_ERR_INVALID_ARGUMENT; a scene made before
 * hfcl_lib_set_shapes: HFCL_ERR_INVALID_ARGUMENT, as for the other scene calls. */
#ifndef HPPFCL_AMD_GROUPS_H
#define HPPFCL_AMD_GROUPS_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* object_group: n_objects bytes, each < n_groups.  collides: n_groups words; bit h of collides[g] set = an object of group g and an
 * object of group h may be listed as a pair.  1 <= n_groups <= 64.  Checked on the host before anything is copied; each of these is
 * HFCL_ERR_INVALID_ARGUMENT with a message that says which, and leaves the scene as it was: n_groups outside 1..64, a group number
 * >= n_groups, a bit >= n_groups set in a word, a matrix that is not symmetric (bit h of collides[g] != bit g of collides[h]), a null
 * pointer.  The tables replace the ones set before; freeing those waits for the device (a query in flight on some stream may still be
 * reading them), as hfcl_scene_set_pairs does. */
int    hfcl_scene_set_groups(hfcl_scene* s, const uint8_t* object_group, size_t n_groups, const uint64_t* collides);
/* Back to the list of every touching pair.  Frees the tables (waits for the device).  Without groups set: HFCL_OK. */
int    hfcl_scene_clear_groups(hfcl_scene* s);
size_t hfcl_scene_num_groups(const hfcl_scene* s);      /* 0: no groups set (or a null scene) */

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_GROUPS_H */
