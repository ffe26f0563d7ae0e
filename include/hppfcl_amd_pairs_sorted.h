/* hppfcl_amd_pairs_sorted.h -- the self-collision pairs of a scene by sort and sweep along one axis: a second way to make THE SAME
 * LIST as the calls of hppfcl_amd_pairs.h (which includes this file; the ABI version stays 5: one query is added), for scenes in which
 * everything moves and the all-pairs test is too much work -- 100 000 objects are 5 * 10^9 box tests of which one in 5 000 hits, 10^6
 * objects a hundred times that.
 *
 * Chosen by the library option `scene_pairs_sorted`: 0 (the default) never -- every call runs the kernels it ran and writes the bytes it
 * wrote --, 1 always: hfcl_scene_self_pairs, _f32, _device, _device_f32, hfcl_scene_collide_self / hfcl_scene_distance_self and their
 * _f32 forms then make their list this way for every scene of two objects or more, whatever `scene_pairs_small_max` says.  There is
 * no automatic switch.  hfcl_scene_nearest_self* and the _env calls are not concerned.  Object groups (hppfcl_amd_groups.h) apply as
 * they do to the all-pairs list.  The list, conf_begin and the count are byte for byte those of the all-pairs form: the same boxes, the
 * same test on the doubles, NaN boxes kept, unbounded boxes no different.
 *
 * The method.  The call goes in chunks of whole configurations (`scene_cull_chunk` rows, at least one configuration).  Per
 * (configuration, object) a key: the box's min along the sweep axis, grown by `inflate`, rounded DOWN to fp32.  The keys of a chunk are
 * sorted (a device-wide radix sort, the configuration above the key); a sorted position pairs with the later positions whose key is not
 * above its own grown max -- a window, its end found by binary search; the exact test decides inside the window; the hits are sorted
 * into the list's order (c, i, j ascending).  Rounding down only widens windows, so no touching pair is skipped.  Option
 * `scene_pairs_sorted_axis`: the sweep axis 0, 1 or 2, or 3 (the default) -- chosen per configuration on the device: the axis on which
 * the boxes' centres spread widest, ties to the lowest.  The list does not depend on the axis or on the chunks.
 *
 * ONE CONTRACT CHANGE, with the option set only: the number of hits of a chunk sizes the workspace of their sort, so the DEVICE forms
 * (hfcl_scene_self_pairs_device*) WAIT ON `stream` once per chunk for 8 bytes, as hfcl_hfield_collide_batch_device does; "nothing is
 * read back" and "asynchronous" hold with the option at 0 only.  The host forms wait as they did.
 *
 * Cost.  Work is the sum of the windows, not n^2: boxes spread along the axis make windows of n^(2/3) positions in a scene of even
 * density.  THE WORST CASE STAYS QUADRATIC: boxes that all overlap on the sweep axis (a stack of plates swept across the stack, many
 * unbounded boxes) have whole configurations as windows -- the all-pairs test again with two sorts on top.  One unbounded box (a tilted
 * Plane) costs one workgroup's walk over its configuration.  Workspace: about 140 bytes a row of a chunk, 16 bytes a hit of a chunk, and
 * the sorts' temporary storage.  Limits as hppfcl_amd_pairs.h. */
#ifndef HPPFCL_AMD_PAIRS_SORTED_H
#define HPPFCL_AMD_PAIRS_SORTED_H
#include "hppfcl_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* How the scene's last list of self pairs was made: 0 the tiled all-pairs test, 1 its wave-per-configuration form, 2 sort and sweep;
 * -1: none was made yet (calls that had nothing to list do not count), or s is NULL.  What the host decided: no read-back. */
int hfcl_scene_last_pairs_form(const hfcl_scene* s);

#ifdef __cplusplus
}
#endif
#endif /* HPPFCL_AMD_PAIRS_SORTED_H */
