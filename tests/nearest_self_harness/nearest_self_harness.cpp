// TEST INFRASTRUCTURE: host build of the header of the clearance on device-made pairs (hpp-fcl_amd/csrc/hfcl_nearest_self.hpp) with g++,
// built by tests/test_scene_nearest_self_cpu.py into a temporary directory.  nsh_bounds computes the bound both ways; nsh_sweep runs the
// workgroups, waves and lanes of k_nself_sweep / k_nself_small in one of their modes (the seeds with k_nself_seed_combine behind the tiled
// form; count, the three scan kernels and emit of a pass), chunk by chunk, as hfcl_host_scene.hip cuts the call; nsh_threshold and
// nsh_combine run what follows the narrow phase.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_nearest_self.hpp"

using namespace hfcl;

namespace {

struct Call {
  const double* boxes;  // the WHOLE table's world boxes (c_box0 = 0 here)
  const uint8_t* group;  // nullptr: no groups
  const uint64_t* collides;
  std::vector<uint64_t> tile_groups;
  PairsGeometry geo;
  bool small;
  double r, D;
  int mode;  // 0: seeds, 1 / 2: the pass
  uint64_t* seed;
  const double* thr;
  std::vector<NselfRowSeed> row_seeds;  // the whole table
  // the chunk
  uint64_t g0, row0;
  uint32_t n_blocks, n_rows;
  std::vector<uint32_t> row_counts;
  std::vector<uint64_t> row_offsets;
  uint32_t* pairs;
  uint64_t capacity;
};

struct Lane {
  double L;
  uint64_t key;
};

// k_nself_sweep<MODE, GROUPS>: workgroup `b` of the chunk; emit: MODE emit, else MODE seed / count
void sweep(Call& k, uint32_t b, bool emit) {
  const uint32_t n = k.geo.n_objects;
  uint64_t c;
  uint32_t i0, i1;
  pairs_block(k.geo, k.g0 + b, c, i0, i1);
  const double* boxes = k.boxes + 6 * (c * n);
  const uint64_t chunk_row = c * n + i0 - k.row0;
  uint64_t block_mask = 0;
  if (k.group) {
    block_mask = pairs_block_mask(k.group, k.collides, i0, i1);
    if (block_mask == 0) {
      for (uint32_t t = 0; t < i1 - i0; ++t) {
        if (k.mode == 0) k.row_seeds[c * n + i0 + t] = NselfRowSeed{__builtin_inf(), SCENE_NONE, 0};
        else if (!emit) k.row_counts[chunk_row + t] = 0;
      }
      return;
    }
  }
  const uint64_t seed = k.mode ? k.seed[c] : NSELF_NO_PAIR;
  const double thr = k.mode == 2 ? k.thr[c] : 0.0;
  std::vector<double> tile(8 * PAIRS_TILE);
  std::vector<uint8_t> tile_group(PAIRS_TILE);
  for (uint32_t wave = 0; wave < 4; ++wave) {
    double row_box[PAIRS_WAVE_ROWS][6];
    NearestBoxTerms row_terms[PAIRS_WAVE_ROWS];
    uint32_t row_i[PAIRS_WAVE_ROWS], count[PAIRS_WAVE_ROWS];
    uint64_t pos[PAIRS_WAVE_ROWS], row_mask[PAIRS_WAVE_ROWS];
    Lane best[PAIRS_WAVE_ROWS][64];
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
      const uint32_t i = i0 + wave * PAIRS_WAVE_ROWS + r;
      const bool there = i < i1;
      row_i[r] = there ? i : n;
      count[r] = 0;
      row_mask[r] = k.group && there ? k.collides[k.group[i] & 63u] : 0;
      for (int q = 0; q < 6; ++q) row_box[r][q] = boxes[6 * size_t(there ? i : i0) + q];
      const NearestBoxTerms t = nearest_box_terms(row_box[r]);
      row_terms[r] = nself_unpack(t.diagonal, nself_pack_largest(t));
      pos[r] = emit && there ? k.row_offsets[chunk_row + wave * PAIRS_WAVE_ROWS + r] : 0;
      for (uint32_t lane = 0; lane < 64; ++lane) best[r][lane] = Lane{__builtin_inf(), NSELF_NO_PAIR};
    }
    for (uint32_t base = pairs_first_tile(i0); base < n; base += PAIRS_TILE) {
      if (k.group && pairs_tile_skipped(k.tile_groups[base / PAIRS_TILE], block_mask)) continue;
      for (uint32_t col = 0; col < PAIRS_TILE && base + col < n; ++col) {
        const double* box = boxes + 6 * size_t(base + col);
        const NearestBoxTerms t = nearest_box_terms(box);
        for (int q = 0; q < 6; ++q) tile[q * PAIRS_TILE + col] = box[q];
        tile[6 * PAIRS_TILE + col] = t.diagonal;
        tile[7 * PAIRS_TILE + col] = nself_pack_largest(t);
        if (k.group) tile_group[col] = k.group[base + col];
      }
      for (uint32_t step = 0; step < PAIRS_TILE; step += 64)
        for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
          uint64_t ballot = 0;
          for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t j = base + step + lane;
            double col_box[6];
            for (int q = 0; q < 6; ++q) col_box[q] = tile[q * PAIRS_TILE + step + lane];
            const NearestBoxTerms col_terms = nself_unpack(tile[6 * PAIRS_TILE + step + lane], tile[7 * PAIRS_TILE + step + lane]);
            const bool candidate = j > row_i[r] && j < n && (!k.group || pairs_allowed(row_mask[r], tile_group[step + lane]));
            if (!candidate) continue;  // (stale columns of the tile are never looked at by a candidate)
            const double L = nearest_bound_terms(row_box[r], row_terms[r], col_box, col_terms, k.r);
            if (k.mode == 0) {
              if (L < best[r][lane].L) best[r][lane] = Lane{L, j};
            } else if (nself_in_pass(k.mode, L, nself_key(row_i[r], j), seed, k.D, thr)) {
              ballot |= uint64_t(1) << lane;
            }
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
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
      if (row_i[r] >= n) continue;
      if (k.mode == 0) {  // the butterfly: a minimum with a tie rule, whatever the order of the merges
        NselfSeed s;
        nself_seed_init(s);
        for (uint32_t lane = 64; lane-- > 0;) nself_seed_merge(s, best[r][lane].L, best[r][lane].key);
        k.row_seeds[c * n + row_i[r]] = NselfRowSeed{s.L, s.key == NSELF_NO_PAIR ? SCENE_NONE : uint32_t(s.key), 0};
      } else if (!emit) {
        k.row_counts[chunk_row + wave * PAIRS_WAVE_ROWS + r] = count[r];
      }
    }
  }
}

// k_nself_small<MODE, GROUPS>: wave `b` of the chunk
void small(Call& k, uint32_t b, bool emit) {
  const uint32_t n = k.geo.n_objects;
  const uint64_t c = k.g0 + b;
  const double* boxes = k.boxes + 6 * (c * n);
  const uint64_t chunk_row = c * n - k.row0;
  const uint64_t seed = k.mode ? k.seed[c] : NSELF_NO_PAIR;
  const double thr = k.mode == 2 ? k.thr[c] : 0.0;
  double col_box[64][6];
  NearestBoxTerms col_terms[64];
  NselfSeed best[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    for (int q = 0; q < 6; ++q) col_box[lane][q] = boxes[6 * size_t(lane < n ? lane : 0) + q];
    const NearestBoxTerms t = nearest_box_terms(col_box[lane]);
    col_terms[lane] = nself_unpack(t.diagonal, nself_pack_largest(t));
    nself_seed_init(best[lane]);
  }
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t ballot = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const bool candidate = lane > i && lane < n && (!k.group || pairs_allowed(k.collides[k.group[i] & 63u], k.group[lane < n ? lane : 0]));
      if (!candidate) continue;
      const double L = nearest_bound_terms(col_box[i], col_terms[i], col_box[lane], col_terms[lane], k.r);
      if (k.mode == 0) {
        if (L < best[lane].L) {
          best[lane].L = L;
          best[lane].key = nself_key(i, lane);
        }
      } else if (nself_in_pass(k.mode, L, nself_key(i, lane), seed, k.D, thr)) {
        ballot |= uint64_t(1) << lane;
      }
    }
    if (k.mode && !emit) k.row_counts[chunk_row + i] = cull_popcount(ballot);
    for (uint32_t lane = 0; emit && lane < 64; ++lane) {
      const uint64_t p = k.row_offsets[chunk_row + i] + cull_rank(ballot, lane);
      if (((ballot >> lane) & 1u) && p < k.capacity) {
        k.pairs[2 * p] = i;
        k.pairs[2 * p + 1] = lane;
      }
    }
  }
  if (k.mode == 0) {
    NselfSeed s;
    nself_seed_init(s);
    for (uint32_t lane = 64; lane-- > 0;) nself_seed_merge(s, best[lane].L, best[lane].key);  // (any order)
    k.seed[c] = s.key;
  }
}

}  // namespace

// nearest_bound and nearest_bound_terms of n box pairs
extern "C" void nsh_bounds(const double* a, const double* b, uint64_t n, double r, double* plain, double* by_terms) {
  for (uint64_t k = 0; k < n; ++k) {
    plain[k] = nearest_bound(a + 6 * k, b + 6 * k, r);
    const NearestBoxTerms ta = nearest_box_terms(a + 6 * k), tb = nearest_box_terms(b + 6 * k);
    // through the two doubles the kernels stage
    by_terms[k] = nearest_bound_terms(a + 6 * k, nself_unpack(ta.diagonal, nself_pack_largest(ta)), b + 6 * k,
                                      nself_unpack(tb.diagonal, nself_pack_largest(tb)), r);
  }
}
extern "C" uint64_t nsh_sizes(int what) { return what == 0 ? sizeof(hfcl_scene_clearance) : what == 1 ? sizeof(NselfRowSeed) : PAIRS_TILE; }

// One walk of the table.  mode 0: seed[n_conf] is written.  mode 1 / 2: the list of the pass (pairs: 2 * capacity words; capacity 0: the
// count alone), conf_begin; seed (and thr, mode 2) are read.  chunk_rows = the option (0: automatic), small_max = the option.  Returns the count.
extern "C" uint64_t nsh_sweep(const double* boxes, uint32_t n_objects, uint64_t n_conf, const uint8_t* group, const uint64_t* collides, double r,
                              double D, int mode, uint64_t chunk_rows, uint32_t small_max, uint64_t* seed, const double* thr, uint32_t* pairs,
                              uint64_t capacity, uint64_t* conf_begin) {
  Call k;
  k.boxes = boxes;
  k.group = group;
  k.collides = collides;
  for (uint32_t t = 0; group && t < pairs_tiles(n_objects); ++t) k.tile_groups.push_back(pairs_tile_word(group, n_objects, t));
  k.small = n_objects <= (small_max < PAIRS_SMALL_MAX ? small_max : PAIRS_SMALL_MAX);
  k.geo = pairs_geometry(n_objects, k.small);
  k.r = r;
  k.D = D;
  k.mode = mode;
  k.seed = seed;
  k.thr = thr;
  k.pairs = pairs;
  k.capacity = pairs ? capacity : 0;
  const uint64_t total_rows = n_conf * n_objects;
  if (mode == 0 && !k.small) k.row_seeds.assign(total_rows, NselfRowSeed{0.0, 0xABABABABu, 0});  // (every row's partial must be written)
  uint64_t n_listed = 0, running = 0;
  const uint64_t n_blocks = n_conf * k.geo.blocks_per_conf;
  const uint64_t per = pairs_chunk_blocks(k.geo, n_blocks, chunk_rows);
  for (uint64_t g0 = 0; g0 < n_blocks; g0 += per) {
    k.g0 = g0;
    k.n_blocks = uint32_t(per < n_blocks - g0 ? per : n_blocks - g0);
    k.row0 = pairs_block_row(k.geo, g0);
    k.n_rows = uint32_t(pairs_block_row(k.geo, g0 + k.n_blocks) - k.row0);
    k.row_counts.assign(k.n_rows, 0xABABABABu);  // (every row's count must be written)
    k.row_offsets.assign(k.n_rows, 0);
    for (uint32_t b = 0; b < k.n_blocks; ++b) k.small ? small(k, b, false) : sweep(k, b, false);
    if (mode == 0) continue;
    for (uint32_t row = 0; row < k.n_rows; ++row) {  // k_pairs_scan_*
      k.row_offsets[row] = running;
      pairs_row_marks(k.row0 + row, running, k.row_counts[row], n_objects, total_rows, n_conf, conf_begin, &n_listed);
      running += k.row_counts[row];
    }
    if (k.capacity)
      for (uint32_t b = 0; b < k.n_blocks; ++b) k.small ? small(k, b, true) : sweep(k, b, true);
  }
  if (mode == 0 && !k.small)  // k_nself_seed_combine
    for (uint64_t c = 0; c < n_conf; ++c) {
      NselfSeed s;
      nself_seed_init(s);
      for (uint32_t i = n_objects; i-- > 0;) {  // (any order)
        const NselfRowSeed o = k.row_seeds[c * n_objects + i];
        if (o.j != SCENE_NONE) nself_seed_merge(s, o.L, nself_key(i, o.j));
      }
      seed[c] = s.key;
    }
  return n_listed;
}

extern "C" void nsh_threshold(const hfcl_scene_summary* summary, uint64_t n_conf, double D, double* thr) {
  for (uint64_t c = 0; c < n_conf; ++c) thr[c] = nearest_threshold(D, summary[c].min_distance);
}

// k_nself_combine<hfcl_result>; a null conf_begin: no list
extern "C" void nsh_combine(uint64_t n_conf, const hfcl_scene_summary* sum1, const hfcl_scene_summary* sum2, const uint32_t* pairs1,
                            const uint32_t* pairs2, const uint64_t* cb1, const uint64_t* cb2, const hfcl_result* rec1, const hfcl_result* rec2,
                            hfcl_scene_clearance* out, hfcl_result* min_out) {
  const hfcl_scene_summary* sum[2] = {sum1, sum2};
  const uint32_t* pairs[2] = {pairs1, pairs2};
  const uint64_t* cb[2] = {cb1, cb2};
  const hfcl_result* rec[2] = {rec1, rec2};
  for (uint64_t c = 0; c < n_conf; ++c) nself_combine<hfcl_result>(c, sum, pairs, cb, rec, out[c], min_out ? min_out + c : nullptr);
}
