// TEST INFRASTRUCTURE: host build of the self-pairs header (hpp-fcl_amd/csrc/hfcl_pairs.hpp) with g++, built by
// tests/test_scene_pairs_cpu.py into a temporary directory.  ph_self_pairs runs the workgroups, waves and lanes of k_pairs_sweep /
// k_pairs_small (count), the three scan kernels and the emit, chunk by chunk, as hfcl_host_scene.hip cuts the call; ph_conf_of runs the
// span searches of the expansion and the fold of a list of pairs; ph_fold_ranked the fold with the rank rule.
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
  std::vector<uint32_t> row_counts;
  std::vector<uint64_t> row_offsets;
  uint32_t* pairs;
  uint64_t capacity;
  uint64_t* conf_begin;
  uint64_t* n_listed;
};

// k_pairs_sweep<EMIT>: workgroup `b` of the chunk
void sweep(Chunk& k, uint32_t b, bool emit) {
  const uint32_t n = k.geo.n_objects;
  uint64_t c;
  uint32_t i0, i1;
  pairs_block(k.geo, k.g0 + b, c, i0, i1);
  const double* boxes = k.boxes + 6 * (c * n);
  const uint64_t chunk_row = c * n + i0 - k.row0;
  std::vector<double> tile(6 * PAIRS_TILE);
  for (uint32_t wave = 0; wave < 4; ++wave) {
    double row_box[PAIRS_WAVE_ROWS][6];
    uint32_t row_i[PAIRS_WAVE_ROWS], count[PAIRS_WAVE_ROWS];
    uint64_t pos[PAIRS_WAVE_ROWS];
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
      const uint32_t i = i0 + wave * PAIRS_WAVE_ROWS + r;
      const bool there = i < i1;
      row_i[r] = there ? i : n;
      count[r] = 0;
      pairs_grow(boxes + 6 * size_t(there ? i : i0), k.inflate, row_box[r]);
      pos[r] = emit && there ? k.row_offsets[chunk_row + wave * PAIRS_WAVE_ROWS + r] : 0;
    }
    for (uint32_t base = pairs_first_tile(i0); base < n; base += PAIRS_TILE) {
      for (uint32_t col = 0; col < PAIRS_TILE && base + col < n; ++col) {  // the tile, grown, component by component
        double g[6];
        pairs_grow(boxes + 6 * size_t(base + col), k.inflate, g);
        for (int q = 0; q < 6; ++q) tile[q * PAIRS_TILE + col] = g[q];
      }
      for (uint32_t step = 0; step < PAIRS_TILE; step += 64)
        for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
          uint64_t ballot = 0;
          for (uint32_t lane = 0; lane < 64; ++lane) {
            double col_box[6];
            for (int q = 0; q < 6; ++q) col_box[q] = tile[q * PAIRS_TILE + step + lane];
            if (pairs_keep(row_i[r], base + step + lane, n, row_box[r], col_box)) ballot |= uint64_t(1) << lane;
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

// k_pairs_small<EMIT>: wave `b` of the chunk
void small(Chunk& k, uint32_t b, bool emit) {
  const uint32_t n = k.geo.n_objects;
  const uint64_t c = k.g0 + b;
  const double* boxes = k.boxes + 6 * (c * n);
  const uint64_t chunk_row = c * n - k.row0;
  double col_box[64][6];
  for (uint32_t lane = 0; lane < 64; ++lane) pairs_grow(boxes + 6 * size_t(lane < n ? lane : 0), k.inflate, col_box[lane]);
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t ballot = 0;
    for (uint32_t lane = 0; lane < 64; ++lane)
      if (pairs_keep(i, lane, n, col_box[i], col_box[lane])) ballot |= uint64_t(1) << lane;
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

// the whole call: chunk_rows = the option (0: automatic), small_max = the option; returns the count.  pairs: 2 * capacity words
extern "C" uint64_t ph_self_pairs(const double* boxes, uint32_t n_objects, uint64_t n_conf, double inflate, uint64_t chunk_rows, uint32_t small_max,
                                  uint32_t* pairs, uint64_t capacity, uint64_t* conf_begin, uint64_t* n_chunks_out) {
  Chunk k;
  k.boxes = boxes;
  k.small = n_objects <= (small_max < PAIRS_SMALL_MAX ? small_max : PAIRS_SMALL_MAX);
  k.geo = pairs_geometry(n_objects, k.small);
  k.total_rows = n_conf * n_objects;
  k.n_conf = n_conf;
  k.inflate = inflate;
  k.pairs = pairs;
  k.capacity = pairs ? capacity : 0;
  k.conf_begin = conf_begin;
  uint64_t n_listed = 0, running = 0, n_chunks = 0;
  k.n_listed = &n_listed;
  const uint64_t n_blocks = n_conf * k.geo.blocks_per_conf;
  const uint64_t per = pairs_chunk_blocks(k.geo, n_blocks, chunk_rows);
  for (uint64_t g0 = 0; g0 < n_blocks; g0 += per, ++n_chunks) {
    k.g0 = g0;
    k.n_blocks = uint32_t(per < n_blocks - g0 ? per : n_blocks - g0);
    k.row0 = pairs_block_row(k.geo, g0);
    k.n_rows = uint32_t(pairs_block_row(k.geo, g0 + k.n_blocks) - k.row0);
    k.row_counts.assign(k.n_rows, 0xABABABABu);  // (every row's count must be written)
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
  if (n_chunks_out) *n_chunks_out = n_chunks;
  return n_listed;
}

// the configuration of every entry of a list: the search, and the forward walk from the configuration of the entry `stride` before
extern "C" void ph_conf_of(const uint64_t* conf_begin, uint64_t n_conf, uint64_t n_listed, uint64_t stride, uint64_t* by_search, uint64_t* by_walk) {
  for (uint64_t k = 0; k < n_listed; ++k) {
    by_search[k] = pairs_conf_of(conf_begin, n_conf, k);
    const uint64_t first = k - k % stride;  // (a wave's first row)
    by_walk[k] = pairs_conf_from(conf_begin, n_conf, pairs_conf_of(conf_begin, n_conf, first), k);
  }
}
extern "C" uint64_t ph_shares(uint64_t n_listed, uint64_t n_objects) { return pairs_shares(n_listed, n_objects); }

// k_scene_fold_listed<R, RANKED = true> / _combine over the chunks [k0, k0 + chunk) of a list: the pieces of a configuration are cut at
// multiples of SCENE_FOLD_SHARE from its begin, `shares` of them at most; the pair index of entry k is k - conf_begin[c]
template <typename R>
static void fold_ranked(const R* rec, const uint64_t* conf_begin, uint64_t n_listed, uint64_t n_conf, uint32_t shares, double margin, int collide,
                        uint64_t chunk, hfcl_scene_summary* summary) {
  for (uint64_t c = 0; c < n_conf; ++c) scene_summary_init(summary[c]);
  for (uint64_t k0 = 0; k0 < n_listed; k0 += chunk) {
    const uint64_t k1 = k0 + chunk < n_listed ? k0 + chunk : n_listed;
    const uint64_t c_lo = pairs_conf_of(conf_begin, n_conf, k0);
    const uint64_t span = pairs_conf_of(conf_begin, n_conf, k1 - 1) - c_lo + 1;
    std::vector<hfcl_scene_summary> partials(span * shares);
    for (uint64_t w = 0; w < span * shares; ++w) {
      const uint64_t c = c_lo + w / shares;
      uint64_t lo, hi;
      scene_listed_piece(conf_begin[c], conf_begin[c + 1], uint32_t(w % shares), k0, k1, lo, hi);
      scene_summary_init(partials[w]);
      for (uint64_t k = lo; k < hi; ++k) {
        const double v = scene_value(rec[k].distance, decltype(rec[k].distance)(margin), collide != 0);
        scene_fold_record(partials[w], v, rec[k].status, uint32_t(k - conf_begin[c]));
      }
    }
    for (uint64_t w = 0; w < span; ++w)
      for (uint32_t g = 0; g < shares; ++g) scene_fold_merge(summary[c_lo + w], partials[w * shares + g]);
  }
}
extern "C" void ph_fold_ranked(const hfcl_result* rec, const uint64_t* conf_begin, uint64_t n_listed, uint64_t n_conf, uint32_t shares, double margin,
                               int collide, uint64_t chunk, hfcl_scene_summary* summary) {
  fold_ranked(rec, conf_begin, n_listed, n_conf, shares, margin, collide, chunk, summary);
}
extern "C" void ph_fold_ranked_f32(const hfcl_result_f32* rec, const uint64_t* conf_begin, uint64_t n_listed, uint64_t n_conf, uint32_t shares,
                                   double margin, int collide, uint64_t chunk, hfcl_scene_summary* summary) {
  fold_ranked(rec, conf_begin, n_listed, n_conf, shares, margin, collide, chunk, summary);
}
