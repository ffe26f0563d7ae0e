// TEST INFRASTRUCTURE: host build of the self-pairs header (hpp-fcl_amd/csrc/hfcl_pairs.hpp) with g++ for the kernels with object groups,
// built by tests/test_scene_groups_cpu.py into a temporary directory.  gh_self_pairs runs the workgroups, waves and lanes of
// k_pairs_sweep_groups / k_pairs_small_groups (count), the three scan kernels and the emit, chunk by chunk, as hfcl_host_scene.hip cuts
// the call -- with the tile words, the block's mask and the skipping of hfcl_pairs.hpp -- and counts what it skipped.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_pairs.hpp"

using namespace hfcl;

namespace {

struct Chunk {
  const double* boxes;  // the WHOLE table's world boxes (the device keeps those of the chunk's configurations: c_box0 = 0 here)
  PairsGeometry geo;
  bool small;
  uint64_t g0, row0, total_rows, n_conf;
  uint32_t n_blocks, n_rows;
  double inflate;
  const uint8_t* group;               // n_objects
  uint64_t collides[PAIRS_MAX_GROUPS];
  std::vector<uint64_t> tile_groups;  // what hfcl_scene_set_groups builds
  std::vector<uint32_t> row_counts;
  std::vector<uint64_t> row_offsets;
  uint32_t* pairs;
  uint64_t capacity;
  uint64_t* conf_begin;
  uint64_t* n_listed;
  uint64_t stats[4];  // count pass: tiles skipped, tiles looked at or skipped, blocks that left at once, blocks
};

// k_pairs_sweep_groups<EMIT>: workgroup `b` of the chunk
void sweep(Chunk& k, uint32_t b, bool emit) {
  const uint32_t n = k.geo.n_objects;
  uint64_t c;
  uint32_t i0, i1;
  pairs_block(k.geo, k.g0 + b, c, i0, i1);
  const double* boxes = k.boxes + 6 * (c * n);
  const uint64_t chunk_row = c * n + i0 - k.row0;
  const uint64_t U = pairs_block_mask(k.group, k.collides, i0, i1);  // (the same in all four waves)
  if (!emit) {
    ++k.stats[3];
    for (uint32_t base = pairs_first_tile(i0); base < n; base += PAIRS_TILE) {
      ++k.stats[1];
      if (pairs_tile_skipped(k.tile_groups[base / PAIRS_TILE], U)) ++k.stats[0];
    }
  }
  if (U == 0) {  // the block leaves at once; the scan still reads its rows' counts
    if (!emit) {
      ++k.stats[2];
      for (uint32_t i = i0; i < i1; ++i) k.row_counts[chunk_row + (i - i0)] = 0;
    }
    return;
  }
  std::vector<double> tile(6 * PAIRS_TILE);
  std::vector<uint8_t> tile_group(PAIRS_TILE, 0xEE);  // (columns past n: stale values, refused by j < n)
  for (uint32_t wave = 0; wave < 4; ++wave) {
    double row_box[PAIRS_WAVE_ROWS][6];
    uint32_t row_i[PAIRS_WAVE_ROWS], count[PAIRS_WAVE_ROWS];
    uint64_t pos[PAIRS_WAVE_ROWS], row_mask[PAIRS_WAVE_ROWS];
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
      const uint32_t i = i0 + wave * PAIRS_WAVE_ROWS + r;
      const bool there = i < i1;
      row_i[r] = there ? i : n;
      row_mask[r] = there ? k.collides[k.group[i]] : 0;
      count[r] = 0;
      pairs_grow(boxes + 6 * size_t(there ? i : i0), k.inflate, row_box[r]);
      pos[r] = emit && there ? k.row_offsets[chunk_row + wave * PAIRS_WAVE_ROWS + r] : 0;
    }
    for (uint32_t base = pairs_first_tile(i0); base < n; base += PAIRS_TILE) {
      if (pairs_tile_skipped(k.tile_groups[base / PAIRS_TILE], U)) continue;
      for (uint32_t col = 0; col < PAIRS_TILE && base + col < n; ++col) {  // the tile, grown, component by component, and its groups
        double g[6];
        pairs_grow(boxes + 6 * size_t(base + col), k.inflate, g);
        for (int q = 0; q < 6; ++q) tile[q * PAIRS_TILE + col] = g[q];
        tile_group[col] = k.group[base + col];
      }
      for (uint32_t step = 0; step < PAIRS_TILE; step += 64)
        for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
          uint64_t ballot = 0;
          for (uint32_t lane = 0; lane < 64; ++lane) {
            double col_box[6];
            for (int q = 0; q < 6; ++q) col_box[q] = tile[q * PAIRS_TILE + step + lane];
            if (pairs_keep(row_i[r], base + step + lane, n, row_box[r], col_box) && pairs_allowed(row_mask[r], tile_group[step + lane]))
              ballot |= uint64_t(1) << lane;
          }
          for (uint32_t lane = 0; emit && lane < 64; ++lane) {
            const uint64_t p = pos[r] + count[r] + cull_rank(ballot, lane);
            if (((ballot >> lane) & 1u) && p < k.capacity) {
              k.pairs[2 * p] = row_i[r];
              k.pairs[2 * p + 1] = base + step + lane;
            }
          }
          count[r] += cull_popcount(ballot);
        }
    }
    for (uint32_t r = 0; !emit && r < PAIRS_WAVE_ROWS; ++r)
      if (row_i[r] < n) k.row_counts[chunk_row + wave * PAIRS_WAVE_ROWS + r] = count[r];
  }
}

// k_pairs_small_groups<EMIT>: wave `b` of the chunk
void small(Chunk& k, uint32_t b, bool emit) {
  const uint32_t n = k.geo.n_objects;
  const uint64_t c = k.g0 + b;
  const double* boxes = k.boxes + 6 * (c * n);
  const uint64_t chunk_row = c * n - k.row0;
  double col_box[64][6];
  uint32_t col_group[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    pairs_grow(boxes + 6 * size_t(lane < n ? lane : 0), k.inflate, col_box[lane]);
    col_group[lane] = k.group[lane < n ? lane : 0];
  }
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t row_mask = k.collides[k.group[i]];
    uint64_t ballot = 0;
    for (uint32_t lane = 0; lane < 64; ++lane)
      if (pairs_keep(i, lane, n, col_box[i], col_box[lane]) && pairs_allowed(row_mask, col_group[lane])) ballot |= uint64_t(1) << lane;
    if (!emit) k.row_counts[chunk_row + i] = cull_popcount(ballot);
    for (uint32_t lane = 0; emit && lane < 64; ++lane) {
      const uint64_t p = k.row_offsets[chunk_row + i] + cull_rank(ballot, lane);
      if (((ballot >> lane) & 1u) && p < k.capacity) {
        k.pairs[2 * p] = i;
        k.pairs[2 * p + 1] = lane;
      }
    }
  }
}

}  // namespace

// the whole call: chunk_rows = the option (0: automatic), small_max = the option; returns the count.  pairs: 2 * capacity words;
// stats: nullptr or four words (Chunk::stats), summed over the count passes of all chunks
extern "C" uint64_t gh_self_pairs(const double* boxes, uint32_t n_objects, uint64_t n_conf, double inflate, uint64_t chunk_rows, uint32_t small_max,
                                  const uint8_t* group, uint32_t n_groups, const uint64_t* collides, uint32_t* pairs, uint64_t capacity,
                                  uint64_t* conf_begin, uint64_t* stats) {
  Chunk k;
  k.boxes = boxes;
  k.small = n_objects <= (small_max < PAIRS_SMALL_MAX ? small_max : PAIRS_SMALL_MAX);
  k.geo = pairs_geometry(n_objects, k.small);
  k.total_rows = n_conf * n_objects;
  k.n_conf = n_conf;
  k.inflate = inflate;
  k.group = group;
  memset(k.collides, 0, sizeof(k.collides));
  memcpy(k.collides, collides, n_groups * sizeof(uint64_t));
  k.tile_groups.resize(pairs_tiles(n_objects));
  for (uint32_t t = 0; t < k.tile_groups.size(); ++t) k.tile_groups[t] = pairs_tile_word(group, n_objects, t);
  k.pairs = pairs;
  k.capacity = pairs ? capacity : 0;
  k.conf_begin = conf_begin;
  memset(k.stats, 0, sizeof(k.stats));
  uint64_t n_listed = 0, running = 0;
  k.n_listed = &n_listed;
  const uint64_t n_blocks = n_conf * k.geo.blocks_per_conf;
  const uint64_t per = pairs_chunk_blocks(k.geo, n_blocks, chunk_rows);
  for (uint64_t g0 = 0; g0 < n_blocks; g0 += per) {
    k.g0 = g0;
    k.n_blocks = uint32_t(per < n_blocks - g0 ? per : n_blocks - g0);
    k.row0 = pairs_block_row(k.geo, g0);
    k.n_rows = uint32_t(pairs_block_row(k.geo, g0 + k.n_blocks) - k.row0);
    k.row_counts.assign(k.n_rows, 0xABABABABu);  // (every row's count must be written, those of a block that leaves at once too)
    k.row_offsets.assign(k.n_rows, 0);
    for (uint32_t b = 0; b < k.n_blocks; ++b) k.small ? small(k, b, false) : sweep(k, b, false);
    // k_pairs_scan_sums / _top / _rows
    const uint32_t n_sums = (k.n_rows + PAIRS_SCAN_BLOCK - 1) / PAIRS_SCAN_BLOCK;
    std::vector<uint32_t> sums(n_sums, 0);
    std::vector<uint64_t> sum_offsets(n_sums);
    for (uint32_t r = 0; r < k.n_rows; ++r) sums[r / PAIRS_SCAN_BLOCK] += k.row_counts[r];
    for (uint32_t b = 0; b < n_sums; ++b) {
      sum_offsets[b] = running;
      running += sums[b];
    }
    for (uint32_t b = 0; b < n_sums; ++b) {
      uint64_t off = sum_offsets[b];
      for (uint32_t r = b * PAIRS_SCAN_BLOCK; r < k.n_rows && r < (b + 1) * PAIRS_SCAN_BLOCK; ++r) {
        k.row_offsets[r] = off;
        pairs_row_marks(k.row0 + r, off, k.row_counts[r], n_objects, k.total_rows, n_conf, conf_begin, k.n_listed);
        off += k.row_counts[r];
      }
    }
    if (k.capacity)
      for (uint32_t b = 0; b < k.n_blocks; ++b) k.small ? small(k, b, true) : sweep(k, b, true);
  }
  if (stats) memcpy(stats, k.stats, sizeof(k.stats));
  return n_listed;
}

// the tile words of a scene as hfcl_scene_set_groups builds them: words[pairs_tiles(n_objects)]; returns their number
extern "C" uint32_t gh_tile_words(const uint8_t* group, uint32_t n_objects, uint64_t* words) {
  const uint32_t n_tiles = pairs_tiles(n_objects);
  for (uint32_t t = 0; t < n_tiles; ++t) words[t] = pairs_tile_word(group, n_objects, t);
  return n_tiles;
}
