// hfcl_terrain.hpp -- a height-field terrain under a scene's moving objects (hppfcl_amd_terrain.h): the arithmetic shared by the kernels
// of hfcl_k_terrain.hip and the host build of the tests (tests/terrain_harness): which (configuration, listed object) a flat query is,
// where its pose row sits in the table, and the fold of a configuration's (bound, status) entries into a hfcl_scene_summary.  Plain
// integer / comparison code: builds with hipcc and with g++.
#pragma once
#include "hfcl_scene.hpp"

namespace hfcl {

// ---- flat query range: q = c * n_t + k, k the rank in the terrain's object list -----------------------------------------------
HFCL_HD void terrain_query(uint64_t q, uint32_t n_t, uint64_t& c, uint32_t& k) {
  c = q / n_t;
  k = uint32_t(q - c * n_t);
}

// The expansion of a chunk [q0, q0 + m): the four per-query arrays the height-field driver reads.  One lane per 16-byte vector of a
// 96-byte pose row: lane t serves row t / 6 of the chunk, vector t % 6 of both of its pose rows; the lane of vector 0 writes the ids.
struct TerrainExpandArgs {
  const double* table;           // (n_conf, n_rows, 12): the moving objects' poses
  const double* tf_terrain;      // 12 doubles, 16-byte aligned
  const uint32_t* objects;       // the n_t listed objects, ascending, every one < n_rows
  const uint32_t* object_shape;  // shape of every object of the scene
  uint64_t n_rows;
  uint32_t n_t;
  uint32_t hfield;
  uint64_t q0;
  uint32_t m;
  uint32_t* out_hfield;          // m
  uint32_t* out_shape;           // m
  double* out_tfh;               // m x 12
  double* out_tfs;               // m x 12
};
// lane t of the chunk: row and vector, the listed object of the row and the first double of that vector in the table
HFCL_HD void terrain_expand_lane(const TerrainExpandArgs& a, uint64_t t, uint32_t& row, uint32_t& part, uint32_t& object, uint64_t& src) {
  row = uint32_t(t / 6u);
  part = uint32_t(t - uint64_t(row) * 6u);
  uint64_t c;
  uint32_t k;
  terrain_query(a.q0 + row, a.n_t, c, k);
  object = a.objects[k];
  src = scene_pose_row(c, a.n_rows, object, 12u) + 2u * part;
}

// ---- the fold ---------------------------------------------------------------------------------------------------------------
// Entry k of configuration c is (bounds[c * n_t + k], status[c * n_t + k]) of object objects[k].  The key of the minimum is (bound,
// object index): scene_fold_record with the bound as the value and the object as the pair -- a skipped entry counts in n_skipped alone,
// a NaN bound never wins (hfcl_scene.hpp: scene_better), the contact flag counts whatever the bound is.  Lanes stride the entries;
// partial summaries merge with scene_fold_merge, whose result does not depend on the order: neither the lane count nor the chunks of
// the call that produced the entries show in the summary.
HFCL_HD void terrain_fold_lane(hfcl_scene_summary& s, const double* bounds, const uint32_t* status, const uint32_t* objects, uint64_t c, uint32_t n_t,
                               uint32_t lane, uint32_t lanes) {
  scene_summary_init(s);
  const uint64_t base = c * n_t;
  for (uint64_t k = lane; k < n_t; k += lanes) scene_fold_record(s, bounds[base + k], status[base + k], objects[k]);
}

// the fold's parameter block (k_terrain_fold): one wave per configuration
struct TerrainFoldArgs {
  const double* bounds;     // n_conf * n_t
  const uint32_t* status;   // n_conf * n_t
  const uint32_t* objects;  // n_t
  uint64_t n_conf;
  uint32_t n_t;
  hfcl_scene_summary* summary;
};

}  // namespace hfcl

#if defined(__HIPCC__)
// hfcl_k_terrain.hip; asynchronous on st, no error checking of their own
void launch_terrain_expand(hipStream_t st, const hfcl::TerrainExpandArgs& a, int max_blocks);
void launch_terrain_status(hipStream_t st, const hfcl_result* rec, uint32_t* status, uint32_t m, int max_blocks);
void launch_terrain_fold(hipStream_t st, const hfcl::TerrainFoldArgs& a, int max_blocks);
#endif
