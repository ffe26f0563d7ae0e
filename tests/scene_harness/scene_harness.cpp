// TEST INFRASTRUCTURE: host build of the scene header (hpp-fcl_amd/csrc/hfcl_scene.hpp) with g++, built by
// tests/test_scene_cpu.py into a temporary directory.  sh_fold / sh_fold_f32 run the chunks, pieces, lanes, butterfly and
// stores of k_scene_fold / k_scene_fold_combine one after the other; sh_expand runs k_scene_expand64's lanes.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_scene.hpp"

using namespace hfcl;

static void wave_reduce(hfcl_scene_summary* lanes) {  // the xor butterfly: every lane ends with the wave's summary
  for (int off = 32; off > 0; off >>= 1) {
    hfcl_scene_summary next[64];
    for (int l = 0; l < 64; ++l) {
      next[l] = lanes[l];
      scene_fold_merge(next[l], lanes[l ^ off]);
    }
    memcpy(lanes, next, sizeof(next));
  }
}
static void store(hfcl_scene_summary* summary, uint64_t c, uint32_t n_pairs, uint64_t q0, const hfcl_scene_summary& part) {
  hfcl_scene_summary s = part;
  if (!scene_chunk_starts(c, n_pairs, q0)) {
    s = summary[c];
    scene_fold_merge(s, part);
  }
  summary[c] = s;
}

template <typename R, typename M>
static void fold(const R* rec, uint64_t total, uint32_t n_pairs, M margin, int collide, uint64_t chunk, hfcl_scene_summary* summary) {
  const uint32_t shares = scene_shares(n_pairs);
  for (uint64_t q0 = 0; q0 < total; q0 += chunk) {
    const uint64_t q1 = q0 + chunk < total ? q0 + chunk : total;
    const uint64_t g0 = scene_piece_of(q0, n_pairs), n_pieces = scene_piece_of(q1 - 1, n_pairs) - g0 + 1;
    std::vector<hfcl_scene_summary> partials(n_pieces);
    for (uint64_t w = 0; w < n_pieces; ++w) {
      uint64_t c, lo, hi;
      scene_piece_range(g0 + w, n_pairs, q0, q1, c, lo, hi);
      hfcl_scene_summary lanes[64];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        scene_summary_init(lanes[lane]);
        for (uint64_t q = lo + lane; q < hi; q += 64u)
          scene_fold_record(lanes[lane], scene_value(rec[q].distance, margin, collide != 0), rec[q].status, uint32_t(q - c * n_pairs));
      }
      wave_reduce(lanes);
      if (shares > 1u)
        partials[w] = lanes[0];
      else
        store(summary, c, n_pairs, q0, lanes[0]);
    }
    if (shares <= 1u) continue;
    const uint64_t c0 = g0 / shares, g_last = g0 + n_pieces - 1;
    for (uint64_t c = c0; c <= g_last / shares; ++c) {
      const uint64_t lo = c * shares > g0 ? c * shares : g0, hi = c * shares + shares - 1 < g_last ? c * shares + shares - 1 : g_last;
      hfcl_scene_summary lanes[64];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        scene_summary_init(lanes[lane]);
        for (uint64_t g = lo + lane; g <= hi; g += 64u) scene_fold_merge(lanes[lane], partials[g - g0]);
      }
      wave_reduce(lanes);
      store(summary, c, n_pairs, q0, lanes[0]);
    }
  }
}

// scene_query_from against the plain division, for chunk starts and rows on either side of 2^32
extern "C" int sh_query_from_agrees(uint64_t q0, uint32_t row, uint32_t n_pairs) {
  uint64_t c0, c, ce;
  uint32_t p0, p, pe;
  scene_query(q0, n_pairs, c0, p0);
  scene_query_from(c0, p0, row, n_pairs, c, p);
  scene_query(q0 + row, n_pairs, ce, pe);
  return c == ce && p == pe;
}
extern "C" size_t sh_summary_size() { return sizeof(hfcl_scene_summary); }
extern "C" uint32_t sh_fold_share() { return SCENE_FOLD_SHARE; }
extern "C" void sh_fold(const hfcl_result* rec, uint64_t total, uint32_t n_pairs, double margin, int collide, uint64_t chunk,
                        hfcl_scene_summary* summary) {
  fold(rec, total, n_pairs, margin, collide, chunk, summary);
}
extern "C" void sh_fold_f32(const hfcl_result_f32* rec, uint64_t total, uint32_t n_pairs, double margin, int collide, uint64_t chunk,
                            hfcl_scene_summary* summary) {
  fold(rec, total, n_pairs, float(margin), collide, chunk, summary);
}
// the lanes of k_scene_expand64 for the chunk [q0, q0 + m): one per 16-byte vector of a 96-byte row
extern "C" void sh_expand(const uint32_t* pairs, const uint32_t* object_shape, const double* table, uint64_t n_objects, uint32_t n_pairs,
                          uint64_t q0, uint32_t m, uint32_t* s1, uint32_t* s2, double* tf1, double* tf2) {
  for (uint64_t t = 0; t < uint64_t(m) * 6u; ++t) {
    const uint32_t row = uint32_t(t / 6u), part = uint32_t(t - uint64_t(row) * 6u);
    uint64_t c;
    uint32_t p;
    uint64_t c0;
    uint32_t p0;
    scene_query(q0, n_pairs, c0, p0);
    scene_query_from(c0, p0, row, n_pairs, c, p);
    const uint32_t i = pairs[2 * size_t(p)], j = pairs[2 * size_t(p) + 1];
    const double* r1 = table + scene_pose_row(c, n_objects, i, 12u) + 2u * part;
    const double* r2 = table + scene_pose_row(c, n_objects, j, 12u) + 2u * part;
    tf1[2 * t] = r1[0]; tf1[2 * t + 1] = r1[1];
    tf2[2 * t] = r2[0]; tf2[2 * t + 1] = r2[1];
    if (part == 0u) {
      s1[row] = object_shape[i];
      s2[row] = object_shape[j];
    }
  }
}
