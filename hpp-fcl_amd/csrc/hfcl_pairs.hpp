// hfcl_pairs.hpp -- the self-collision pairs of a scene per configuration (hfcl_scene_self_pairs*) and the scene calls on such a list
// (hfcl_scene_*_pairs_device*, hfcl_scene_*_self): the arithmetic shared by the kernels of hfcl_k_pairs.hip, the host unit and the host build
// of the tests (tests/pairs_harness).  A tiled all-pairs test of the world boxes of hfcl_cull.hpp -- no tree, no sorting, no atomics --,
// compacted by count / scan / emit as the cull compacts its flat range.  Builds with hipcc and with g++.
//
// Rows.  Row r = c * n_objects + i of the table is object i of configuration c; its entries are the pairs (i, j), j > i, whose two boxes,
// each grown by `inflate`, touch.  The list is the rows' entries in row order, j ascending inside a row: c, then i, then j ascending.
// Row blocks.  A configuration's rows are cut into blocks of `rows_per_block` consecutive rows (the last one shorter); block g of the call is
// block g % blocks_per_conf of configuration g / blocks_per_conf.  A workgroup (large scenes) or a wave (scenes of at most PAIRS_SMALL_MAX
// objects: the whole configuration is one block) owns a block.  A call goes through its blocks in chunks of consecutive blocks; the rows of
// a chunk are consecutive rows of the table, so a chunk's row counts and row offsets are indexed by row - first row of the chunk.
#pragma once
#include "hfcl_cull.hpp"

namespace hfcl {

// large scenes: columns staged in LDS per tile (6 x PAIRS_TILE doubles, 12 KiB), rows a wave tests at once (their grown boxes in
// registers), rows per workgroup of four waves
// (HFCL_PAIRS_TILE / HFCL_PAIRS_WAVE_ROWS: variant builds of tools/build_variant.sh, units k_pairs and host_scene together)
#ifndef HFCL_PAIRS_TILE
#define HFCL_PAIRS_TILE 256
#endif
#ifndef HFCL_PAIRS_WAVE_ROWS
#define HFCL_PAIRS_WAVE_ROWS 4
#endif
constexpr uint32_t PAIRS_TILE = HFCL_PAIRS_TILE;
constexpr uint32_t PAIRS_WAVE_ROWS = HFCL_PAIRS_WAVE_ROWS;
static_assert(PAIRS_TILE % 64u == 0u && PAIRS_TILE >= 64u && PAIRS_WAVE_ROWS >= 1u, "a tile is whole 64-column steps");
constexpr uint32_t PAIRS_ROWS = 4u * PAIRS_WAVE_ROWS;
// small scenes: a wave per configuration, lane = column
constexpr uint32_t PAIRS_SMALL_MAX = 64u;
// rows per workgroup of the scan
constexpr uint32_t PAIRS_SCAN_BLOCK = 1024u;
// rows per chunk when the option does not say (the row counts and offsets of a chunk: 12 B a row)
constexpr uint64_t PAIRS_CHUNK_ROWS = uint64_t(1) << 20;

// ---- the predicate ---------------------------------------------------------------------------------------------------------
// box a grown as cull_keep grows it (AABB::expand): the same subtraction and addition, done once per box instead of once per test
HFCL_HD void pairs_grow(const double* a, double inflate, double* g) {
  for (int k = 0; k < 3; ++k) {
    g[k] = a[k] - inflate;
    g[3 + k] = a[3 + k] + inflate;
  }
}
// (i, j) is listed: j a column of the row, inside the configuration, and the grown boxes touch (cull_boxes_touch: closed, a NaN keeps)
HFCL_HD bool pairs_keep(uint32_t i, uint32_t j, uint32_t n_objects, const double* grown_i, const double* grown_j) {
  return j > i && j < n_objects && cull_boxes_touch(grown_i, grown_j);
}

// ---- row blocks ------------------------------------------------------------------------------------------------------------
struct PairsGeometry {
  uint32_t n_objects;
  uint32_t rows_per_block;   // PAIRS_ROWS, or n_objects (small scenes)
  uint32_t blocks_per_conf;
};
HFCL_HD PairsGeometry pairs_geometry(uint32_t n_objects, bool small) {
  PairsGeometry g;
  g.n_objects = n_objects;
  g.rows_per_block = small ? n_objects : PAIRS_ROWS;
  g.blocks_per_conf = (n_objects + g.rows_per_block - 1u) / g.rows_per_block;
  return g;
}
// block g: its configuration and its rows [i0, i1) there
HFCL_HD void pairs_block(const PairsGeometry& geo, uint64_t g, uint64_t& c, uint32_t& i0, uint32_t& i1) {
  c = g / geo.blocks_per_conf;
  const uint32_t b = uint32_t(g - c * geo.blocks_per_conf);
  i0 = b * geo.rows_per_block;
  i1 = geo.n_objects - i0 > geo.rows_per_block ? i0 + geo.rows_per_block : geo.n_objects;
}
// first row of block g in the table (g = the call's number of blocks: the number of rows)
HFCL_HD uint64_t pairs_block_row(const PairsGeometry& geo, uint64_t g) {
  const uint64_t c = g / geo.blocks_per_conf;
  return c * geo.n_objects + (g - c * geo.blocks_per_conf) * geo.rows_per_block;
}
// first column tile a block whose first row is i0 looks at: the one that holds column i0 + 1
HFCL_HD uint32_t pairs_first_tile(uint32_t i0) { return (i0 + 1u) / PAIRS_TILE * PAIRS_TILE; }
// blocks per chunk of a call of n_blocks > 0 blocks: `option` rows (0: PAIRS_CHUNK_ROWS), in whole blocks, at least one; the call in equal chunks
HFCL_HD uint64_t pairs_chunk_blocks(const PairsGeometry& geo, uint64_t n_blocks, uint64_t option) {
  const uint64_t rows = option ? option : PAIRS_CHUNK_ROWS;
  uint64_t per = rows / geo.rows_per_block;
  if (per < 1u) per = 1u;
  if (per > n_blocks) per = n_blocks;
  if (option) return per;
  const uint64_t n_chunks = (n_blocks + per - 1u) / per;
  return (n_blocks + n_chunks - 1u) / n_chunks;
}

// ---- object groups (include/hppfcl_amd_groups.h) -------------------------------------------------------------------------------
// Every object has a group below PAIRS_MAX_GROUPS; collides[g] is the row mask of an object of group g: bit h set = it may pair with an
// object of group h.  (i, j) is listed iff pairs_keep and pairs_allowed(collides[group[i]], group[j]).
constexpr uint32_t PAIRS_MAX_GROUPS = 64u;
HFCL_HD bool pairs_allowed(uint64_t row_mask, uint32_t col_group) { return ((row_mask >> (col_group & 63u)) & 1u) != 0u; }
// column tiles of a scene, and the word of tile t: the groups its objects [t PAIRS_TILE, (t + 1) PAIRS_TILE) have, a bit each
HFCL_HD uint32_t pairs_tiles(uint32_t n_objects) { return (n_objects + PAIRS_TILE - 1u) / PAIRS_TILE; }
HFCL_HD uint64_t pairs_tile_word(const uint8_t* group, uint32_t n_objects, uint32_t t) {
  uint64_t word = 0;
  for (uint32_t j = t * PAIRS_TILE; j < n_objects && j - t * PAIRS_TILE < PAIRS_TILE; ++j) word |= uint64_t(1) << (group[j] & 63u);
  return word;
}
// the mask of a row block: the OR of its rows' masks -- every group some row [i0, i1) of the block may pair with.  One value for the
// whole block: what it skips is decided in front of a workgroup barrier, so every wave must decide the same
HFCL_HD uint64_t pairs_block_mask(const uint8_t* group, const uint64_t* collides, uint32_t i0, uint32_t i1) {
  uint64_t mask = 0;
  for (uint32_t i = i0; i < i1; ++i) mask |= collides[group[i] & 63u];
  return mask;
}
// a block skips a column tile none of whose groups any of its rows may pair with (a block whose mask is 0 skips them all: it leaves)
HFCL_HD bool pairs_tile_skipped(uint64_t tile_word, uint64_t block_mask) { return (tile_word & block_mask) == 0u; }

// ---- the scan ----------------------------------------------------------------------------------------------------------------
// row `row` of the table starts at `offset` with `count` entries: what it says about conf_begin and the total
HFCL_HD void pairs_row_marks(uint64_t row, uint64_t offset, uint32_t count, uint32_t n_objects, uint64_t total_rows, uint64_t n_conf,
                             uint64_t* conf_begin, uint64_t* n_listed) {
  if (conf_begin && row % n_objects == 0u) conf_begin[row / n_objects] = offset;
  if (row == total_rows - 1u) {
    if (conf_begin) conf_begin[n_conf] = offset + count;
    if (n_listed) *n_listed = offset + count;
  }
}

// ---- the scene calls on a list -------------------------------------------------------------------------------------------------
// the configuration whose span conf_begin[c] <= k < conf_begin[c + 1] holds entry k (k below conf_begin[n_conf]; configurations without
// entries lie in between): the last c with conf_begin[c] <= k
HFCL_HD uint64_t pairs_conf_of(const uint64_t* conf_begin, uint64_t n_conf, uint64_t k) {
  uint64_t lo = 0, hi = n_conf;  // the answer is in [lo, hi)
  while (hi - lo > 1u) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    if (conf_begin[mid] <= k) lo = mid;
    else hi = mid;
  }
  return lo;
}
// ... given that it is not before `c` (the configuration of an entry before k): a few steps forward, then the search
HFCL_HD uint64_t pairs_conf_from(const uint64_t* conf_begin, uint64_t n_conf, uint64_t c, uint64_t k) {
  for (int step = 0; step < 4; ++step) {
    if (c + 1u >= n_conf || conf_begin[c + 1u] > k) return c;
    ++c;
  }
  return pairs_conf_of(conf_begin, n_conf, k);
}
// pieces of SCENE_FOLD_SHARE entries a configuration of such a list can have: no configuration has more entries than the list, or than pairs
HFCL_HD uint64_t pairs_shares(uint64_t n_listed, uint64_t n_objects) {
  const uint64_t all = n_objects < 2u ? 0u : (n_objects % 2u ? n_objects * ((n_objects - 1u) / 2u) : (n_objects / 2u) * (n_objects - 1u));
  const uint64_t most = n_listed < all ? n_listed : all;
  const uint64_t shares = (most + SCENE_FOLD_SHARE - 1u) / SCENE_FOLD_SHARE;
  return shares ? shares : 1u;
}

}  // namespace hfcl
