// TEST INFRASTRUCTURE: host build of the header of the clearance among a kept environment (hpp-fcl_amd/csrc/hfcl_nearest_env.hpp) with g++,
// built by tests/test_scene_nearest_env_cpu.py into a temporary directory.  neh_terms computes the set-time tables; neh_property the
// bound of a (row block, tile) cell beside the bounds of all its pairs; neh_sweep runs the cells of k_nenv_sweep in one of its modes (the
// seed partials with k_nenv_seed_combine behind them; count, the three scan kernels over the (row, span) counts and emit of a pass),
// chunk by chunk and span by span, as hfcl_host_scene.hip cuts the call, and counts what it dropped by distance; neh_threshold and
// neh_combine run what follows the narrow phase.
// cell() restates the loop of k_nenv_sweep on the host, it does not share it with the kernel: what this build covers is the header's
// arithmetic and the cutting into cells, spans and chunks, not the kernel's staging through LDS, its ballots or its barriers -- those are
// covered by tests/test_scene_nearest_env_gpu.py alone, against yardsticks that do not run the kernel.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_nearest_env.hpp"

using namespace hfcl;

namespace {

struct Call {
  const double* moving;  // n_conf x n_moving world boxes
  const double* env;     // n_env world boxes
  std::vector<double> tile_boxes, env_terms, tile_terms;
  EnvGeometry geo;
  PairsGeometry rows;
  uint64_t n_conf, row0;  // row0: the chunk's first moving row
  const uint8_t* group;   // nullptr: no groups; else of the full scene
  uint64_t collides[PAIRS_MAX_GROUPS];
  std::vector<uint64_t> tile_groups;
  double r, D;
  int mode;  // 0: seeds, 1 / 2: the pass
  bool prune;
  uint64_t* seed;
  const double* thr;
  std::vector<NselfRowSeed> row_seeds;  // (row, span) partials of the whole table
  std::vector<uint32_t> counts;          // the chunk's (row, span) counts, row-major
  std::vector<uint64_t> offsets;
  uint32_t* pairs;
  uint64_t capacity;
  uint64_t stats[3];  // count pass: environment cells dropped by distance, environment cells looked at, pairs of the pass inside a dropped cell
};

// k_nenv_sweep<MODE, GROUPS>: the cell (row block g, span) of the chunk; emit: MODE emit, else MODE seed / count
void cell(Call& k, uint64_t g, uint32_t span, bool emit) {
  const uint32_t nm = k.geo.n_moving, n = nm + k.geo.n_env;
  uint64_t c;
  uint32_t i0, i1;
  pairs_block(k.rows, g, c, i0, i1);
  const double* boxes = k.moving + 6 * (c * nm);
  const uint64_t chunk_row = c * nm + i0 - k.row0;
  const uint64_t mask = k.group ? pairs_block_mask(k.group, k.collides, i0, i1) : ~uint64_t(0);
  const bool prune = k.mode != 0 && k.prune;
  NenvBlock block = NenvBlock();
  if (prune) block = nenv_block(boxes, i0, i1);
  const uint64_t seed = k.mode ? k.seed[c] : NSELF_NO_PAIR;
  const double thr = k.mode == 2 ? k.thr[c] : 0.0;
  uint32_t u0 = span * k.geo.span_len;
  const uint32_t u1 = k.geo.tiles - u0 > k.geo.span_len ? u0 + k.geo.span_len : k.geo.tiles;
  const uint32_t first = env_first_tile(i0, k.geo.tiles_moving);
  if (u0 < first) u0 = first;
  if (k.group && mask == 0) u0 = u1;
  std::vector<uint32_t> count(i1 - i0, 0);
  std::vector<NselfSeed> best(i1 - i0);
  for (NselfSeed& s : best) nself_seed_init(s);
  for (uint32_t u = u0; u < u1; ++u) {
    bool env;
    uint32_t base, j0, j_end;
    env_tile_columns(k.geo, u, env, base, j0, j_end);
    const double* table = env ? k.env : boxes;
    if (k.group && pairs_tile_skipped(k.tile_groups[u], mask)) continue;
    const uint32_t cols = j_end - j0 < PAIRS_TILE ? j_end - j0 : PAIRS_TILE;
    bool dropped = false;
    if (env && k.mode != 0 && !emit) ++k.stats[1];
    if (prune && env) {
      const uint32_t t = base / PAIRS_TILE;
      const double Lt = nenv_tile_bound(block, k.tile_boxes.data() + 6 * size_t(t), k.tile_terms.data() + 2 * size_t(t), k.r);
      dropped = nenv_tile_dropped(k.mode, Lt, seed, i0, i1, j0, cols, thr);
      if (dropped && !emit) ++k.stats[0];
    }
    for (uint32_t i = i0; i < i1; ++i) {
      const double* row_box = boxes + 6 * size_t(i);
      const NearestBoxTerms rt = nearest_box_terms(row_box);
      const NearestBoxTerms row_terms = nself_unpack(rt.diagonal, nself_pack_largest(rt));
      const uint64_t row_mask = k.group ? k.collides[k.group[i] & 63u] : 0;
      const uint64_t at = (chunk_row + (i - i0)) * k.geo.n_spans + span;
      for (uint32_t col = 0; col < cols; ++col) {
        const uint32_t j = j0 + col;
        if (!(j > i && j < j_end) || (k.group && !pairs_allowed(row_mask, k.group[j]))) continue;
        const double* col_box = table + 6 * size_t(base + col);
        NearestBoxTerms col_terms;
        if (env) {  // (what the tile stages: the set-time terms)
          col_terms = nself_unpack(k.env_terms[2 * size_t(base + col)], k.env_terms[2 * size_t(base + col) + 1]);
        } else {
          const NearestBoxTerms t = nearest_box_terms(col_box);
          col_terms = nself_unpack(t.diagonal, nself_pack_largest(t));
        }
        const double L = nearest_bound_terms(row_box, row_terms, col_box, col_terms, k.r);
        if (k.mode == 0) {
          if (L < best[i - i0].L) {
            best[i - i0].L = L;
            best[i - i0].key = j;
          }
          continue;
        }
        if (!nself_in_pass(k.mode, L, nself_key(i, j), seed, k.D, thr)) continue;
        if (dropped) {  // never drops a pair of the pass
          if (!emit) ++k.stats[2];
          continue;
        }
        if (emit) {
          const uint64_t p = k.offsets[at] + count[i - i0];
          if (p < k.capacity) {
            k.pairs[2 * p] = i;
            k.pairs[2 * p + 1] = j;
          }
        }
        ++count[i - i0];
      }
    }
  }
  for (uint32_t i = i0; i < i1; ++i) {
    if (k.mode == 0) {
      const NselfSeed& s = best[i - i0];
      k.row_seeds[(c * nm + i) * k.geo.n_spans + span] = NselfRowSeed{s.L, s.key == NSELF_NO_PAIR ? SCENE_NONE : uint32_t(s.key), 0};
    } else if (!emit) {
      k.counts[(chunk_row + (i - i0)) * k.geo.n_spans + span] = count[i - i0];
    }
  }
  (void)n;
}

}  // namespace

extern "C" uint64_t neh_sizes(int what) {
  return what == 0 ? sizeof(hfcl_scene_clearance) : what == 1 ? sizeof(NselfRowSeed) : what == 2 ? PAIRS_TILE : PAIRS_ROWS;
}

// the set-time tables of n_env boxes: tile boxes (tiles x 6), box terms (n_env x 2), tile terms (tiles x 2), and -- for the comparison --
// nearest_box_terms of every member as three doubles (diagonal, largest, finite).  Returns the number of tiles.
extern "C" uint32_t neh_terms(const double* env_boxes, uint32_t n_env, double* tile_boxes, double* env_terms, double* tile_terms, double* plain) {
  const uint32_t n_tiles = env_tiles(n_env);
  for (uint32_t x = 0; x < 6 * n_tiles; ++x) tile_boxes[x] = env_tile_coord(env_boxes, n_env, x / 6, x % 6);
  for (uint32_t e = 0; e < n_env; ++e) {
    nenv_box_terms(env_boxes + 6 * size_t(e), env_terms + 2 * size_t(e));
    const NearestBoxTerms t = nearest_box_terms(env_boxes + 6 * size_t(e));
    plain[3 * size_t(e)] = t.diagonal;
    plain[3 * size_t(e) + 1] = t.largest;
    plain[3 * size_t(e) + 2] = t.finite ? 1.0 : 0.0;
  }
  for (uint32_t t = 0; t < n_tiles; ++t) nenv_tile_terms(env_terms, n_env, t, tile_terms + 2 * size_t(t));
  return n_tiles;
}

// n_cases cells: case k has the row boxes rows[row_begin[k] .. row_begin[k + 1]) (1 .. PAIRS_ROWS of them) and the member boxes
// members[member_begin[k] .. member_begin[k + 1]) (1 .. PAIRS_TILE).  Lt[k]: the cell's bound through the set-time tables; min_L[k]: the
// smallest nearest_bound over all (row, member); any_none[k]: some pair has L = -inf
extern "C" void neh_property(const double* rows, const uint64_t* row_begin, const double* members, const uint64_t* member_begin, uint64_t n_cases,
                             double r, double* Lt, double* min_L, uint8_t* any_none) {
  std::vector<double> terms(2 * PAIRS_TILE);
  for (uint64_t k = 0; k < n_cases; ++k) {
    const double* rb = rows + 6 * row_begin[k];
    const double* mb = members + 6 * member_begin[k];
    const uint32_t nr = uint32_t(row_begin[k + 1] - row_begin[k]), n_env = uint32_t(member_begin[k + 1] - member_begin[k]);
    double tile_box[6], tile_terms[2];
    for (uint32_t q = 0; q < 6; ++q) tile_box[q] = env_tile_coord(mb, n_env, 0, q);
    for (uint32_t e = 0; e < n_env; ++e) nenv_box_terms(mb + 6 * size_t(e), terms.data() + 2 * size_t(e));
    nenv_tile_terms(terms.data(), n_env, 0, tile_terms);
    const NenvBlock block = nenv_block(rb, 0, nr);
    Lt[k] = nenv_tile_bound(block, tile_box, tile_terms, r);
    double least = __builtin_inf();
    bool none = false;
    for (uint32_t i = 0; i < nr; ++i)
      for (uint32_t e = 0; e < n_env; ++e) {
        const double L = nearest_bound(rb + 6 * size_t(i), mb + 6 * size_t(e), r);
        if (L == -__builtin_inf()) none = true;
        if (L < least) least = L;
      }
    min_L[k] = least;
    any_none[k] = none ? 1 : 0;
  }
}

// One walk of the table.  mode 0: seed[n_conf] is written.  mode 1 / 2: the list of the pass (pairs: 2 * capacity words; capacity 0: the
// count alone), conf_begin; seed (and thr, mode 2) are read.  chunk_rows: option scene_cull_chunk; span: option scene_env_span (0:
// automatic for n_cus compute units); prune: option scene_nearest_env_prune; group: nullptr or the full scene's groups.  stats: nullptr
// or three words (Call::stats).  Returns the count.
extern "C" uint64_t neh_sweep(const double* moving, uint32_t n_moving, const double* env, uint32_t n_env, uint64_t n_conf, const uint8_t* group,
                              uint32_t n_groups, const uint64_t* collides, double r, double D, int mode, int prune, uint64_t chunk_rows,
                              uint32_t span, uint32_t n_cus, uint64_t* seed, const double* thr, uint32_t* pairs, uint64_t capacity,
                              uint64_t* conf_begin, uint64_t* stats) {
  Call k;
  k.moving = moving;
  k.env = env;
  k.rows = pairs_geometry(n_moving, false);
  const uint64_t n_blocks = n_conf * k.rows.blocks_per_conf;
  const uint32_t tiles = env_geometry(n_moving, n_env, 0).tiles;
  if (span == 0) span = env_auto_span(tiles, n_blocks, n_cus ? n_cus : 1, ENV_AUTO_PER_CU);
  k.geo = env_geometry(n_moving, n_env, span);
  const uint32_t n_tiles = env_tiles(n_env);
  k.tile_boxes.resize(6 * size_t(n_tiles) + 6);
  k.env_terms.resize(2 * size_t(n_env) + 2);
  k.tile_terms.resize(2 * size_t(n_tiles) + 2);
  std::vector<double> plain(3 * size_t(n_env) + 3);
  neh_terms(env, n_env, k.tile_boxes.data(), k.env_terms.data(), k.tile_terms.data(), plain.data());
  k.n_conf = n_conf;
  k.group = group;
  memset(k.collides, 0, sizeof(k.collides));
  if (group) memcpy(k.collides, collides, n_groups * sizeof(uint64_t));
  k.tile_groups.resize(k.geo.tiles);
  for (uint32_t u = 0; group && u < k.geo.tiles; ++u) k.tile_groups[u] = env_tile_word(k.geo, group, u);
  k.r = r;
  k.D = D;
  k.mode = mode;
  k.prune = prune != 0;
  k.seed = seed;
  k.thr = thr;
  k.pairs = pairs;
  k.capacity = pairs ? capacity : 0;
  memset(k.stats, 0, sizeof(k.stats));
  uint64_t n_listed = 0, running = 0;
  if (n_conf == 0 || n_moving == 0) {
    for (uint64_t c = 0; mode && c <= n_conf; ++c) conf_begin[c] = 0;
    for (uint64_t c = 0; !mode && c < n_conf; ++c) seed[c] = NSELF_NO_PAIR;
    return 0;
  }
  const uint64_t S = k.geo.n_spans;
  if (mode == 0) k.row_seeds.assign(n_conf * n_moving * S, NselfRowSeed{0.0, 0xABABABABu, 0});  // (every partial must be written)
  const uint64_t per = env_chunk_blocks(k.geo, n_blocks, chunk_rows);
  for (uint64_t g0 = 0; g0 < n_blocks; g0 += per) {
    const uint64_t nb = per < n_blocks - g0 ? per : n_blocks - g0;
    k.row0 = pairs_block_row(k.rows, g0);
    const uint64_t n_rows = (pairs_block_row(k.rows, g0 + nb) - k.row0) * S;  // the scan's rows
    k.counts.assign(n_rows, 0xABABABABu);  // (every count must be written, those of cells that walk no tile too)
    k.offsets.assign(n_rows, 0);
    for (uint64_t x = 0; x < nb * S; ++x) cell(k, g0 + x / S, uint32_t(x % S), false);
    if (mode == 0) continue;
    // k_pairs_scan_sums / _top / _rows with rows x spans as the rows: n_objects = n_moving * n_spans
    for (uint64_t row = 0; row < n_rows; ++row) {
      k.offsets[row] = running;
      pairs_row_marks(k.row0 * S + row, running, k.counts[row], uint32_t(n_moving * S), n_conf * n_moving * S, n_conf, conf_begin, &n_listed);
      running += k.counts[row];
    }
    if (k.capacity)
      for (uint64_t x = 0; x < nb * S; ++x) cell(k, g0 + x / S, uint32_t(x % S), true);
  }
  if (mode == 0)  // k_nenv_seed_combine
    for (uint64_t c = 0; c < n_conf; ++c) {
      NselfSeed s;
      nself_seed_init(s);
      const uint64_t per_conf = uint64_t(n_moving) * S;
      for (uint64_t x = per_conf; x-- > 0;) nenv_seed_fold(s, k.row_seeds.data() + c * per_conf, uint32_t(S), x);  // (any order)
      seed[c] = s.key;
    }
  if (stats) memcpy(stats, k.stats, sizeof(k.stats));
  return n_listed;
}

extern "C" void neh_threshold(const hfcl_scene_summary* summary, uint64_t n_conf, double D, double* thr) {
  for (uint64_t c = 0; c < n_conf; ++c) thr[c] = nearest_threshold(D, summary[c].min_distance);
}

// k_nself_combine<hfcl_result>; a null conf_begin: no list
extern "C" void neh_combine(uint64_t n_conf, const hfcl_scene_summary* sum1, const hfcl_scene_summary* sum2, const uint32_t* pairs1,
                            const uint32_t* pairs2, const uint64_t* cb1, const uint64_t* cb2, const hfcl_result* rec1, const hfcl_result* rec2,
                            hfcl_scene_clearance* out, hfcl_result* min_out) {
  const hfcl_scene_summary* sum[2] = {sum1, sum2};
  const uint32_t* pairs[2] = {pairs1, pairs2};
  const uint64_t* cb[2] = {cb1, cb2};
  const hfcl_result* rec[2] = {rec1, rec2};
  for (uint64_t c = 0; c < n_conf; ++c) nself_combine<hfcl_result>(c, sum, pairs, cb, rec, out[c], min_out ? min_out + c : nullptr);
}
