// TEST INFRASTRUCTURE: host build of the environment header (hpp-fcl_amd/csrc/hfcl_env.hpp) with g++, built by tests/test_scene_env_cpu.py
// into a temporary directory -- as a shared library for the comparisons with the numpy model (tests/env_model.py) and as a program of its
// own (main below: the random property check and the order check, which need no model).  eh_env_pairs runs the cells of k_env_sweep /
// k_env_sweep_groups (count), the three scan kernels over the (row, span) counts and the emit, chunk by chunk, as hfcl_host_scene.hip cuts
// the call -- with the tile boxes, the block's union and mask and the skipping of hfcl_env.hpp -- and counts what it skipped.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_env.hpp"

using namespace hfcl;

namespace {

struct Call {
  const double* moving;  // n_conf x n_moving world boxes
  const double* env;     // n_env world boxes
  std::vector<double> tile_boxes;
  EnvGeometry geo;
  PairsGeometry rows;
  uint64_t n_conf, row0;  // row0: the chunk's first moving row
  double inflate;
  const uint8_t* group;  // nullptr: no groups; else of the full scene
  uint64_t collides[PAIRS_MAX_GROUPS];
  std::vector<uint64_t> tile_groups;
  std::vector<uint32_t> counts;   // the chunk's (row, span) counts, row-major
  std::vector<uint64_t> offsets;
  uint32_t* pairs;
  uint64_t capacity;
  uint64_t stats[4];  // count pass: environment cells skipped by box, environment cells, cells skipped by groups, listed pairs inside a skipped cell
};

// k_env_sweep<EMIT> / k_env_sweep_groups<EMIT>: the cell (row block g, span) of the chunk
void cell(Call& k, uint64_t g, uint32_t span, bool emit) {
  const uint32_t nm = k.geo.n_moving;
  uint64_t c;
  uint32_t i0, i1;
  pairs_block(k.rows, g, c, i0, i1);
  const double* boxes = k.moving + 6 * (c * nm);
  const uint64_t chunk_row = c * nm + i0 - k.row0;
  const uint64_t mask = k.group ? pairs_block_mask(k.group, k.collides, i0, i1) : ~uint64_t(0);
  double uni[6];
  env_union(boxes, i0, i1, k.inflate, uni);
  uint32_t u0 = span * k.geo.span_len;
  const uint32_t u1 = k.geo.tiles - u0 > k.geo.span_len ? u0 + k.geo.span_len : k.geo.tiles;
  const uint32_t first = env_first_tile(i0, k.geo.tiles_moving);
  if (u0 < first) u0 = first;
  if (k.group && mask == 0) u0 = u1;
  std::vector<uint32_t> count(i1 - i0, 0);
  for (uint32_t u = u0; u < u1; ++u) {
    bool env;
    uint32_t base, j0, j_end;
    env_tile_columns(k.geo, u, env, base, j0, j_end);
    const double* table = env ? k.env : boxes;
    if (k.group && pairs_tile_skipped(k.tile_groups[u], mask)) {
      if (!emit) ++k.stats[2];
      continue;
    }
    if (env && !emit) ++k.stats[1];
    if (env && env_tile_skipped(k.tile_boxes.data() + 6 * size_t(base / PAIRS_TILE), k.inflate, uni)) {
      if (!emit) {
        ++k.stats[0];
        for (uint32_t i = i0; i < i1; ++i)  // never skips a listed pair: the rule of the list on every (row, member) of the cell
          for (uint32_t col = 0; col < PAIRS_TILE && j0 + col < j_end; ++col)
            if (cull_keep(boxes + 6 * size_t(i), table + 6 * size_t(base + col), k.inflate)) ++k.stats[3];
      }
      continue;
    }
    for (uint32_t i = i0; i < i1; ++i) {
      double row_box[6];
      pairs_grow(boxes + 6 * size_t(i), k.inflate, row_box);
      const uint64_t row_mask = k.group ? k.collides[k.group[i] & 63u] : 0;
      const uint64_t at = (chunk_row + (i - i0)) * k.geo.n_spans + span;
      for (uint32_t col = 0; col < PAIRS_TILE; ++col) {
        const uint32_t j = j0 + col;
        if (j >= j_end) break;
        double col_box[6];
        pairs_grow(table + 6 * size_t(base + col), k.inflate, col_box);
        if (!pairs_keep(i, j, j_end, row_box, col_box) || (k.group && !pairs_allowed(row_mask, k.group[j]))) continue;
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
  if (!emit)
    for (uint32_t i = i0; i < i1; ++i) k.counts[(chunk_row + (i - i0)) * k.geo.n_spans + span] = count[i - i0];
}

// the rule of the list, straight: c, then i, then j ascending, i < n_moving, i < j, the boxes touch, the groups may pair
uint64_t brute(const double* moving, uint32_t nm, const double* env, uint32_t ne, uint64_t n_conf, double inflate, const uint8_t* group,
               const uint64_t* collides, std::vector<uint32_t>& pairs, std::vector<uint64_t>& conf_begin) {
  pairs.clear();
  conf_begin.assign(n_conf + 1, 0);
  for (uint64_t c = 0; c < n_conf; ++c) {
    conf_begin[c] = pairs.size() / 2;
    for (uint32_t i = 0; i < nm; ++i)
      for (uint32_t j = i + 1; j < nm + ne; ++j) {
        const double* bj = j < nm ? moving + 6 * (c * nm + j) : env + 6 * size_t(j - nm);
        if (!cull_keep(moving + 6 * (c * nm + i), bj, inflate)) continue;
        if (group && !pairs_allowed(collides[group[i] & 63u], group[j])) continue;
        pairs.push_back(i);
        pairs.push_back(j);
      }
  }
  conf_begin[n_conf] = pairs.size() / 2;
  return pairs.size() / 2;
}

}  // namespace

// the tile boxes of n_env boxes as hfcl_scene_set_environment computes them: out[env_tiles(n_env) x 6]; returns their number
extern "C" uint32_t eh_tile_boxes(const double* env_boxes, uint32_t n_env, double* out) {
  const uint32_t n_tiles = env_tiles(n_env);
  for (uint32_t x = 0; x < 6 * n_tiles; ++x) out[x] = env_tile_coord(env_boxes, n_env, x / 6, x % 6);
  return n_tiles;
}

// the whole call.  chunk_rows: option scene_cull_chunk; span: option scene_env_span (0: automatic for n_cus compute units; n_cus == 0:
// every tile in one span); group: nullptr or the full scene's groups.  Returns the count.  pairs: nullptr or 2 * capacity words;
// conf_begin: n_conf + 1; stats: nullptr or four words (Call::stats) summed over the count passes; geometry: nullptr or {span_len, n_spans}
extern "C" uint64_t eh_env_pairs(const double* moving, uint32_t n_moving, const double* env, uint32_t n_env, uint64_t n_conf, double inflate,
                                 uint64_t chunk_rows, uint32_t span, uint32_t n_cus, const uint8_t* group, uint32_t n_groups,
                                 const uint64_t* collides, uint32_t* pairs, uint64_t capacity, uint64_t* conf_begin, uint64_t* stats,
                                 uint32_t* geometry) {
  Call k;
  k.moving = moving;
  k.env = env;
  k.rows = pairs_geometry(n_moving, false);
  const uint64_t n_blocks = n_conf * k.rows.blocks_per_conf;
  const uint32_t tiles = env_geometry(n_moving, n_env, 0).tiles;
  if (span == 0 && n_cus) span = env_auto_span(tiles, n_blocks, n_cus, ENV_AUTO_PER_CU);
  k.geo = env_geometry(n_moving, n_env, span);
  if (geometry) {
    geometry[0] = k.geo.span_len;
    geometry[1] = k.geo.n_spans;
  }
  k.tile_boxes.resize(6 * size_t(env_tiles(n_env)) + 6);
  eh_tile_boxes(env, n_env, k.tile_boxes.data());
  k.n_conf = n_conf;
  k.inflate = inflate;
  k.group = group;
  memset(k.collides, 0, sizeof(k.collides));
  if (group) memcpy(k.collides, collides, n_groups * sizeof(uint64_t));
  k.tile_groups.resize(k.geo.tiles);
  for (uint32_t u = 0; group && u < k.geo.tiles; ++u) k.tile_groups[u] = env_tile_word(k.geo, group, u);
  k.pairs = pairs;
  k.capacity = pairs ? capacity : 0;
  memset(k.stats, 0, sizeof(k.stats));
  uint64_t n_listed = 0, running = 0;
  if (n_conf == 0 || n_moving == 0) {
    for (uint64_t c = 0; c <= n_conf; ++c) conf_begin[c] = 0;
    return 0;
  }
  const uint64_t per = env_chunk_blocks(k.geo, n_blocks, chunk_rows);
  const uint64_t S = k.geo.n_spans;
  for (uint64_t g0 = 0; g0 < n_blocks; g0 += per) {
    const uint64_t nb = per < n_blocks - g0 ? per : n_blocks - g0;
    k.row0 = pairs_block_row(k.rows, g0);
    const uint64_t n_rows = (pairs_block_row(k.rows, g0 + nb) - k.row0) * S;  // the scan's rows
    k.counts.assign(n_rows, 0xABABABABu);  // (every count must be written, those of cells that walk no tile too)
    k.offsets.assign(n_rows, 0);
    for (uint64_t x = 0; x < nb * S; ++x) cell(k, g0 + x / S, uint32_t(x % S), false);
    // k_pairs_scan_sums / _top / _rows with rows x spans as the rows: n_objects = n_moving * n_spans
    for (uint64_t r = 0; r < n_rows; ++r) {
      k.offsets[r] = running;
      pairs_row_marks(k.row0 * S + r, running, k.counts[r], uint32_t(n_moving * S), n_conf * n_moving * S, n_conf, conf_begin, &n_listed);
      running += k.counts[r];
    }
    if (k.capacity)
      for (uint64_t x = 0; x < nb * S; ++x) cell(k, g0 + x / S, uint32_t(x % S), true);
  }
  if (stats) memcpy(stats, k.stats, sizeof(k.stats));
  return n_listed;
}

// ---- the program: what needs no model ---------------------------------------------------------------------------------------------------
namespace {

int failures = 0;
#define EXPECT(cond, ...)                    \
  do {                                       \
    if (!(cond)) {                           \
      ++failures;                            \
      printf("FAILED %s: ", #cond);          \
      printf(__VA_ARGS__);                   \
      printf("\n");                          \
    }                                        \
  } while (0)

// a box with now and then a NaN, an infinity or an unbounded side
void random_box(std::mt19937_64& rng, double spread, double* b) {
  std::uniform_real_distribution<double> at(-spread, spread), half(0.05, 1.5);
  std::uniform_int_distribution<int> odd(0, 99);
  for (int q = 0; q < 3; ++q) {
    const double mid = at(rng), h = half(rng);
    b[q] = mid - h;
    b[3 + q] = mid + h;
  }
  const int what = odd(rng);
  const int q = odd(rng) % 6;
  const double inf = __builtin_inf(), big = 1.7976931348623157e308;
  if (what == 0) b[q] = __builtin_nan("");
  else if (what == 1) b[q] = q < 3 ? -inf : inf;
  else if (what == 2) b[q] = q < 3 ? inf : -inf;  // (an empty side: nothing touches it)
  else if (what == 3) b[q] = q < 3 ? -big : big;
}

// never skips a listed pair: 10^4 random boxes -- 625 cells of up to 16 rows against tiles of up to 256 members, both inflates
void property_check() {
  std::mt19937_64 rng(20240611);
  uint64_t boxes = 0, skipped = 0, looked = 0, nan_skipped = 0;
  for (int trial = 0; boxes < 10000; ++trial) {
    const uint32_t n_rows = 1 + uint32_t(rng() % PAIRS_ROWS), n_members = 1 + uint32_t(rng() % (trial % 8 == 0 ? PAIRS_TILE : 24));
    const double spread = trial % 3 == 0 ? 2.0 : 12.0;
    std::vector<double> rows(6 * n_rows), members(6 * n_members);
    for (uint32_t i = 0; i < n_rows; ++i) random_box(rng, spread, &rows[6 * i]);
    const double shift = (trial % 2) * 3.0 * spread;  // (half of the tiles far from the rows, so that both outcomes occur)
    for (uint32_t j = 0; j < n_members; ++j) {
      random_box(rng, spread, &members[6 * j]);
      if (members[6 * j] == members[6 * j]) members[6 * j] += shift, members[6 * j + 3] += shift;
    }
    boxes += n_rows + n_members;
    double tile[6];
    for (uint32_t q = 0; q < 6; ++q) tile[q] = env_tile_coord(members.data(), n_members, 0, q);
    for (const double inflate : {0.0, 0.25}) {
      double uni[6];
      env_union(rows.data(), 0, n_rows, inflate, uni);
      const bool skip = env_tile_skipped(tile, inflate, uni);
      skip ? ++skipped : ++looked;
      if (!skip) continue;
      bool has_nan = false;
      for (double v : rows) has_nan |= v != v;
      for (double v : members) has_nan |= v != v;
      nan_skipped += has_nan;
      for (uint32_t i = 0; i < n_rows; ++i)
        for (uint32_t j = 0; j < n_members; ++j)
          EXPECT(!cull_keep(&rows[6 * i], &members[6 * j], inflate), "trial %d inflate %g row %u member %u", trial, inflate, i, j);
    }
  }
  EXPECT(skipped > 100 && looked > 100, "skipped %llu looked at %llu", (unsigned long long)skipped, (unsigned long long)looked);
  printf("property check: %llu boxes, %llu cells skipped (%llu with a NaN about), %llu looked at\n", (unsigned long long)boxes,
         (unsigned long long)skipped, (unsigned long long)nan_skipped, (unsigned long long)looked);
}

// cell geometry and the row-major scan reproduce (c, i, j) order: span lengths 1, 2 and "all", whole and in chunks, with and without groups
void order_check() {
  std::mt19937_64 rng(7);
  const uint32_t sizes[][2] = {{37, 600}, {16, 256}, {17, 257}, {1, 1}, {2, 0}, {300, 40}, {5, 0}};
  for (const auto& sz : sizes) {
    const uint32_t nm = sz[0], ne = sz[1];
    const uint64_t n_conf = 3;
    std::vector<double> moving(6 * n_conf * nm), env(6 * size_t(ne) + 6);
    for (size_t i = 0; i < n_conf * nm; ++i) random_box(rng, 6.0, &moving[6 * i]);
    for (uint32_t j = 0; j < ne; ++j) {
      random_box(rng, 6.0, &env[6 * size_t(j)]);
      if (env[6 * size_t(j)] == env[6 * size_t(j)]) env[6 * size_t(j)] += 14.0 * (j / PAIRS_TILE), env[6 * size_t(j) + 3] += 14.0 * (j / PAIRS_TILE);
    }
    std::vector<uint8_t> group(nm + ne);
    for (auto& g : group) g = uint8_t(rng() % 5);
    uint64_t collides[5] = {0x0E, 0x15, 0x0B, 0x15, 0x0A};  // (symmetric)
    for (int with_groups = 0; with_groups < 2; ++with_groups)
      for (const double inflate : {0.0, 0.25}) {
        std::vector<uint32_t> want;
        std::vector<uint64_t> want_begin;
        const uint64_t n = brute(moving.data(), nm, env.data(), ne, n_conf, inflate, with_groups ? group.data() : nullptr, collides, want, want_begin);
        for (const uint32_t span : {1u, 2u, 0u})
          for (const uint64_t chunk : {uint64_t(0), uint64_t(7), uint64_t(64)}) {
            std::vector<uint32_t> got(2 * (n + 4), 0x5A5A5A5Au);
            std::vector<uint64_t> begin(n_conf + 1, 0x5A5A5A5A5A5A5A5Aull);
            uint64_t stats[4];
            const uint64_t m = eh_env_pairs(moving.data(), nm, env.data(), ne, n_conf, inflate, chunk, span, 0, with_groups ? group.data() : nullptr, 5,
                                            collides, got.data(), n, begin.data(), stats, nullptr);
            EXPECT(m == n, "%u + %u: count %llu, expected %llu (span %u chunk %llu groups %d)", nm, ne, (unsigned long long)m, (unsigned long long)n, span,
                   (unsigned long long)chunk, with_groups);
            EXPECT(m != n || !n || !memcmp(got.data(), want.data(), 8 * n), "%u + %u: the list (span %u chunk %llu groups %d)", nm, ne, span,
                   (unsigned long long)chunk, with_groups);
            EXPECT(begin == want_begin, "%u + %u: conf_begin (span %u chunk %llu groups %d)", nm, ne, span, (unsigned long long)chunk, with_groups);
            EXPECT(stats[3] == 0, "%u + %u: a skipped cell holds a listed pair", nm, ne);
            for (size_t x = 2 * n; x < got.size(); ++x) EXPECT(got[x] == 0x5A5A5A5Au, "written past the capacity");
          }
      }
  }
  printf("order check: done\n");
}

}  // namespace

int main() {
  property_check();
  order_check();
  if (failures) printf("env_harness: %d FAILED\n", failures);
  else printf("env_harness: ok\n");
  return failures ? 1 : 0;
}
