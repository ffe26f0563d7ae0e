// hfcl_env.hpp -- a static environment kept on the device (include/hppfcl_amd_env.h: hfcl_scene_set_environment*, hfcl_scene_env_pairs*,
// hfcl_scene_*_env*): the arithmetic shared by the kernels of hfcl_k_env.hip, the host unit and the host build of the tests
// (tests/env_harness).  Objects [0, n_moving) of a scene move, objects [n_moving, n_objects) are the environment: their world boxes and
// one box per tile of PAIRS_TILE consecutive environment objects are computed once.  Builds with hipcc and with g++.
//
// Columns.  The columns of a configuration are cut into tiles of PAIRS_TILE: first the tiles of the moving objects [0, n_moving) -- the
// last one shorter --, then the tiles of the environment, counted from the first environment object, so that their edges -- and their
// boxes -- do not move with n_moving.  Tile u < tiles_moving holds the columns j = u PAIRS_TILE + k < n_moving, tile u >= tiles_moving
// the columns j = n_moving + (u - tiles_moving) PAIRS_TILE + k < n_objects.
// Cells.  The work unit is a cell: a row block (hfcl_pairs.hpp: PAIRS_ROWS consecutive moving rows of one configuration) times a span of
// `span_len` consecutive column tiles.  Cell x of a chunk is span x % n_spans of row block x / n_spans.  Counts are kept per (row, span),
// at index row * n_spans + span: scanned in that order -- row-major -- the positions come out in (c, i, j) order, and the scan is the one of
// hfcl_k_pairs.hip with rows x spans as its rows.
#pragma once
#include "hfcl_pairs.hpp"

namespace hfcl {

// ---- tile boxes ------------------------------------------------------------------------------------------------------------
// one step of the fold of a min / a max: a NaN makes the coordinate -inf / +inf for good (nothing is below -inf)
HFCL_HD double env_fold_min(double m, double x) { return x != x ? -__builtin_inf() : (x < m ? x : m); }
HFCL_HD double env_fold_max(double m, double x) { return x != x ? __builtin_inf() : (x > m ? x : m); }
HFCL_HD uint32_t env_tiles(uint32_t n_env) { return (n_env + PAIRS_TILE - 1u) / PAIRS_TILE; }
// coordinate k (0..2: min, 3..5: max) of the box of tile t of the environment's n_env boxes: the fold in member order
HFCL_HD double env_tile_coord(const double* env_boxes, uint32_t n_env, uint32_t t, uint32_t k) {
  const uint32_t e0 = t * PAIRS_TILE, e1 = n_env - e0 > PAIRS_TILE ? e0 + PAIRS_TILE : n_env;
  double m = k < 3u ? __builtin_inf() : -__builtin_inf();
  for (uint32_t e = e0; e < e1; ++e) m = k < 3u ? env_fold_min(m, env_boxes[6u * size_t(e) + k]) : env_fold_max(m, env_boxes[6u * size_t(e) + k]);
  return m;
}
// the union of the grown boxes of the rows [i0, i1) of a configuration's moving boxes: the same fold over boxes grown as pairs_grow grows them
HFCL_HD void env_union(const double* boxes, uint32_t i0, uint32_t i1, double inflate, double* u) {
  for (int k = 0; k < 3; ++k) {
    u[k] = __builtin_inf();
    u[3 + k] = -__builtin_inf();
  }
  for (uint32_t i = i0; i < i1; ++i) {
    double g[6];
    pairs_grow(boxes + 6u * size_t(i), inflate, g);
    for (int k = 0; k < 3; ++k) {
      u[k] = env_fold_min(u[k], g[k]);
      u[3 + k] = env_fold_max(u[3 + k], g[3 + k]);
    }
  }
}
// a row block skips an environment tile whose grown box does not touch the union of its rows' grown boxes.  The tile's box holds every
// member's, the union every row's, growing is monotone and a NaN coordinate became the infinity that fails no comparison: a pair of a
// row and a member that cull_boxes_touch keeps is never skipped
HFCL_HD bool env_tile_skipped(const double* tile_box, double inflate, const double* union_grown) {
  double g[6];
  pairs_grow(tile_box, inflate, g);
  return !cull_boxes_touch(union_grown, g);
}

// ---- cells ---------------------------------------------------------------------------------------------------------------
// a (row, span) count is below span_len * PAIRS_TILE, and a scan workgroup adds PAIRS_SCAN_BLOCK of them in 32 bits
constexpr uint32_t ENV_SPAN_MAX = uint32_t((uint64_t(1) << 32) / PAIRS_SCAN_BLOCK / PAIRS_TILE);
// workgroups per compute unit the automatic span length aims at (option `scene_env_span` 0)
constexpr uint32_t ENV_AUTO_PER_CU = 4u;
constexpr uint32_t ENV_MAX_OBJECTS = 1u << 22;         // n_moving and n_env, each
constexpr uint64_t ENV_CHUNK_SCAN_ROWS = uint64_t(1) << 22;   // (row, span) counts per chunk when the option does not say (12 B each)
constexpr uint64_t ENV_CHUNK_SCAN_ROWS_MAX = uint64_t(1) << 28;  // ... at most, whatever it says
struct EnvGeometry {
  uint32_t n_moving, n_env;
  uint32_t tiles_moving, tiles;  // tiles of the moving columns, of all columns
  uint32_t span_len, n_spans;
};
// span_len: tiles per span as asked for (0: all of them in one span); what is possible: at least 1, at most ENV_SPAN_MAX, and no more
// spans than keep n_moving * n_spans in 32 bits (the scan's row arithmetic)
HFCL_HD EnvGeometry env_geometry(uint32_t n_moving, uint32_t n_env, uint32_t span_len) {
  EnvGeometry g;
  g.n_moving = n_moving;
  g.n_env = n_env;
  g.tiles_moving = (n_moving + PAIRS_TILE - 1u) / PAIRS_TILE;
  g.tiles = g.tiles_moving + env_tiles(n_env);
  const uint32_t tiles = g.tiles ? g.tiles : 1u;
  if (span_len == 0u || span_len > tiles) span_len = tiles;
  const uint32_t spans_max = n_moving ? 0xFFFFFFFFu / n_moving : 1u;
  const uint32_t least = (tiles + spans_max - 1u) / spans_max;
  if (span_len < least) span_len = least;
  // (a span longer than ENV_SPAN_MAX tiles is cut: with both limits at 2^22 objects the two bounds never conflict --
  //  at most 2^15 tiles, at least 2^10 - 1 spans allowed, so `least` is at most 33)
  if (span_len > ENV_SPAN_MAX) span_len = ENV_SPAN_MAX;
  g.span_len = span_len;
  g.n_spans = (tiles + span_len - 1u) / span_len;
  return g;
}
// the automatic span length: a call of n_blocks row blocks on n_cus compute units gets about `per_cu` workgroups per unit
HFCL_HD uint32_t env_auto_span(uint32_t tiles, uint64_t n_blocks, uint32_t n_cus, uint32_t per_cu) {
  const uint64_t want = uint64_t(n_cus) * per_cu;
  const uint64_t spans = n_blocks >= want ? 1u : (want + n_blocks - 1u) / (n_blocks ? n_blocks : 1u);
  const uint64_t len = tiles / spans;
  return len < 1u ? 1u : uint32_t(len);
}
// first column tile a block whose first row is i0 looks at: the moving tile that holds column i0 + 1, or the first environment tile
HFCL_HD uint32_t env_first_tile(uint32_t i0, uint32_t tiles_moving) {
  const uint32_t u = (i0 + 1u) / PAIRS_TILE;
  return u < tiles_moving ? u : tiles_moving;
}
// column tile u: its first column as an index into its own table (moving boxes of the configuration / environment boxes) and into the full
// scene, and the end of its table as an index into the full scene
HFCL_HD void env_tile_columns(const EnvGeometry& g, uint32_t u, bool& env, uint32_t& base, uint32_t& j0, uint32_t& j_end) {
  env = u >= g.tiles_moving;
  base = (env ? u - g.tiles_moving : u) * PAIRS_TILE;
  j0 = env ? g.n_moving + base : base;
  j_end = env ? g.n_moving + g.n_env : g.n_moving;
}
// the groups present in column tile u, a bit each (hfcl_pairs.hpp: pairs_tile_word over this tiling); group: of the full scene
HFCL_HD uint64_t env_tile_word(const EnvGeometry& g, const uint8_t* group, uint32_t u) {
  bool env;
  uint32_t base, j0, j_end;
  env_tile_columns(g, u, env, base, j0, j_end);
  uint64_t word = 0;
  for (uint32_t j = j0; j < j_end && j - j0 < PAIRS_TILE; ++j) word |= uint64_t(1) << (group[j] & 63u);
  return word;
}
// row blocks per chunk of a call of n_blocks > 0 blocks: `option` moving rows (0: as many as give ENV_CHUNK_SCAN_ROWS counts), in whole
// blocks, at least one, at most what gives ENV_CHUNK_SCAN_ROWS_MAX counts
HFCL_HD uint64_t env_chunk_blocks(const EnvGeometry& g, uint64_t n_blocks, uint64_t option) {
  const uint64_t rows = option ? option : ENV_CHUNK_SCAN_ROWS / g.n_spans;
  const uint64_t most = ENV_CHUNK_SCAN_ROWS_MAX / g.n_spans / PAIRS_ROWS;
  uint64_t per = rows / PAIRS_ROWS;
  if (per > most) per = most;
  if (per < 1u) per = 1u;
  if (per > n_blocks) per = n_blocks;
  return per;
}

// ---- the scene calls on such a list --------------------------------------------------------------------------------------------
// pieces of SCENE_FOLD_SHARE entries a configuration of an env list can have: no configuration has more entries than the list, or than
// moving x moving plus moving x environment pairs
HFCL_HD uint64_t env_shares(uint64_t n_listed, uint64_t n_moving, uint64_t n_env) {
  const uint64_t mm = n_moving < 2u ? 0u : (n_moving % 2u ? n_moving * ((n_moving - 1u) / 2u) : (n_moving / 2u) * (n_moving - 1u));
  const uint64_t all = mm + n_moving * n_env;
  const uint64_t most = n_listed < all ? n_listed : all;
  const uint64_t shares = (most + SCENE_FOLD_SHARE - 1u) / SCENE_FOLD_SHARE;
  return shares ? shares : 1u;
}

}  // namespace hfcl
