// TEST INFRASTRUCTURE: host build of the pruned-minimum header (hpp-fcl_amd/csrc/hfcl_nearest.hpp) with g++, built by
// tests/test_scene_nearest_cpu.py into a temporary directory.  nh_bound runs nearest_bound; nh_select runs the waves and lanes of
// k_nearest_seed / k_nearest_seed_combine, the workgroups of k_nearest_mark with k_cull_scan / k_cull_emit chunk by chunk, the fold of
// pass 1 over the records it is given, k_nearest_threshold, and pass 2; nh_gather runs k_nearest_gather's lanes.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_nearest.hpp"

using namespace hfcl;

extern "C" void nh_bound(const double* a, const double* b, uint64_t n, double r, double* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = nearest_bound(a + 6 * i, b + 6 * i, r);
}

static double query_bound(const double* boxes, const uint32_t* pairs, uint64_t n_objects, uint64_t c, uint32_t p, double r) {
  const double* base = boxes + 6 * (c * n_objects);
  return nearest_bound(base + 6 * size_t(pairs[2 * size_t(p)]), base + 6 * size_t(pairs[2 * size_t(p) + 1]), r);
}

static void seed_wave_reduce(NearestSeed* lanes) {  // the xor butterfly: every lane ends with the wave's seed
  for (int off = 32; off > 0; off >>= 1) {
    NearestSeed next[64];
    for (int l = 0; l < 64; ++l) {
      next[l] = lanes[l];
      nearest_seed_merge(next[l], lanes[l ^ off].L, lanes[l ^ off].p);
    }
    memcpy(lanes, next, sizeof(next));
  }
}

struct Select {
  const double* boxes;
  const uint32_t* pairs;
  uint32_t n_pairs;
  uint64_t n_objects, n_conf;
  double upper, r;
  const uint32_t* seed;
  const double* thr;
};

// mark, scan, emit of one pass over the chunks of the flat range; returns the count
static uint64_t compact(const Select& s, int pass, uint64_t chunk, uint64_t* ids, uint64_t* conf_begin) {
  const uint64_t total = s.n_conf * s.n_pairs;
  uint64_t running = 0, n_listed = 0;
  for (uint64_t q0 = 0; q0 < total; q0 += chunk) {
    const uint32_t m = uint32_t(q0 + chunk < total ? chunk : total - q0);
    uint64_t c0;
    uint32_t p0;
    scene_query(q0, s.n_pairs, c0, p0);
    const uint32_t n_blocks = (m + CULL_BLOCK - 1) / CULL_BLOCK;
    std::vector<uint64_t> words((m + 63) / 64), offsets(n_blocks);
    std::vector<uint32_t> counts(n_blocks);
    for (uint32_t b = 0; b < n_blocks; ++b) {  // k_nearest_mark
      uint32_t n = 0;
      for (uint32_t wave = 0; wave < CULL_WAVES; ++wave) {
        uint64_t ballot = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint32_t row = b * CULL_BLOCK + wave * 64 + lane;
          if (row >= m) continue;
          uint64_t c;
          uint32_t p;
          scene_query_from(c0, p0, row, s.n_pairs, c, p);
          const double L = query_bound(s.boxes, s.pairs, s.n_objects, c, p, s.r);
          const bool keep = pass == 1 ? nearest_in_pass1(L, p, s.seed[c], s.upper) : nearest_in_pass2(L, p, s.seed[c], s.upper, s.thr[c]);
          if (keep) ballot |= uint64_t(1) << lane;
        }
        if (b * CULL_BLOCK + wave * 64 < m) words[(b * CULL_BLOCK + wave * 64) >> 6] = ballot;
        n += cull_popcount(ballot);
      }
      counts[b] = n;
    }
    for (uint32_t b = 0; b < n_blocks; ++b) {  // k_cull_scan
      offsets[b] = running;
      running += counts[b];
    }
    for (uint32_t row = 0; row < m; ++row) {  // k_cull_emit
      const uint32_t b = row / CULL_BLOCK, wave = (row % CULL_BLOCK) >> 6, lane = row & 63u;
      uint64_t pos = offsets[b];
      for (uint32_t w = 0; w < wave; ++w) pos += cull_popcount(words[size_t(b) * CULL_WAVES + w]);
      const uint64_t ballot = words[size_t(b) * CULL_WAVES + wave];
      pos += cull_rank(ballot, lane);
      const bool keep = (ballot >> lane) & 1u;
      const uint64_t q = q0 + row;
      if (keep) ids[pos] = q;
      uint64_t c;
      uint32_t p;
      scene_query_from(c0, p0, row, s.n_pairs, c, p);
      if (p == 0u) conf_begin[c] = pos;
      if (q == total - 1) conf_begin[s.n_conf] = n_listed = pos + (keep ? 1u : 0u);
    }
  }
  return n_listed;
}

// ids1 / ids2: room for every query; conf_begin1 / conf_begin2: n_conf + 1; records: those of ALL n_conf * n_pairs queries (what the
// narrow phase would compute); n_out: the two counts
extern "C" void nh_select(const double* boxes, const uint32_t* pairs, uint32_t n_pairs, uint64_t n_objects, uint64_t n_conf, double upper,
                          double r, const hfcl_result* records, uint64_t chunk, uint32_t* seed, uint64_t* ids1, uint64_t* conf_begin1,
                          double* thr, uint64_t* ids2, uint64_t* conf_begin2, hfcl_scene_summary* summary, uint64_t* n_out) {
  const uint32_t shares = scene_shares(n_pairs);
  std::vector<NearestSeed> partials(n_conf * shares);
  for (uint64_t w = 0; w < n_conf * shares; ++w) {  // k_nearest_seed
    const uint64_t c = w / shares;
    const uint32_t piece = uint32_t(w - c * shares);
    const uint32_t lo = piece * SCENE_FOLD_SHARE;
    const uint32_t hi = n_pairs - lo > SCENE_FOLD_SHARE ? lo + SCENE_FOLD_SHARE : n_pairs;
    NearestSeed lanes[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
      nearest_seed_init(lanes[lane]);
      for (uint32_t p = lo + lane; p < hi; p += 64u) nearest_seed_merge(lanes[lane], query_bound(boxes, pairs, n_objects, c, p, r), p);
    }
    seed_wave_reduce(lanes);
    partials[w] = lanes[0];
  }
  for (uint64_t c = 0; c < n_conf; ++c) {  // k_nearest_seed_combine
    NearestSeed lanes[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
      nearest_seed_init(lanes[lane]);
      for (uint32_t g = lane; g < shares; g += 64u) nearest_seed_merge(lanes[lane], partials[c * shares + g].L, partials[c * shares + g].p);
    }
    seed_wave_reduce(lanes);
    seed[c] = lanes[0].p;
  }
  Select s{boxes, pairs, n_pairs, n_objects, n_conf, upper, r, seed, thr};
  n_out[0] = compact(s, 1, chunk, ids1, conf_begin1);
  for (uint64_t c = 0; c < n_conf; ++c) {  // the fold of pass 1, k_nearest_threshold
    scene_summary_init(summary[c]);
    for (uint64_t k = conf_begin1[c]; k < conf_begin1[c + 1]; ++k)
      scene_fold_record(summary[c], scene_value(records[ids1[k]].distance, 0.0, false), records[ids1[k]].status, uint32_t(ids1[k] - c * n_pairs));
    thr[c] = nearest_threshold(upper, summary[c].min_distance);
  }
  n_out[1] = compact(s, 2, chunk, ids2, conf_begin2);
  for (uint64_t c = 0; c < n_conf; ++c) {  // the fold of pass 2, merged
    hfcl_scene_summary part;
    scene_summary_init(part);
    for (uint64_t k = conf_begin2[c]; k < conf_begin2[c + 1]; ++k)
      scene_fold_record(part, scene_value(records[ids2[k]].distance, 0.0, false), records[ids2[k]].status, uint32_t(ids2[k] - c * n_pairs));
    scene_fold_merge(summary[c], part);
  }
}

// k_nearest_gather: position of c * n_pairs + min_pair in the two lists (list << 63 | position), or ~0 for a configuration without a min_pair
extern "C" void nh_gather(const hfcl_scene_summary* summary, uint64_t n_conf, uint32_t n_pairs, const uint64_t* ids1, const uint64_t* conf_begin1,
                          const uint64_t* ids2, const uint64_t* conf_begin2, uint64_t* where) {
  const uint64_t* ids[2] = {ids1, ids2};
  const uint64_t* cb[2] = {conf_begin1, conf_begin2};
  for (uint64_t c = 0; c < n_conf; ++c) {
    where[c] = ~uint64_t(0);
    if (summary[c].min_pair == SCENE_NONE) continue;
    const uint64_t q = c * n_pairs + summary[c].min_pair;
    for (int l = 0; l < 2; ++l) {
      const uint64_t k = nearest_find(ids[l], cb[l][c], cb[l][c + 1], q);
      if (k < cb[l][c + 1]) {
        where[c] = (uint64_t(l) << 63) | k;
        break;
      }
    }
  }
}

extern "C" void nh_no_record(hfcl_result* r, hfcl_result_f32* r32) {
  nearest_no_record(*r);
  nearest_no_record(*r32);
}
extern "C" double nh_r(int f32) { return f32 ? NEAREST_R32 : NEAREST_R64; }
