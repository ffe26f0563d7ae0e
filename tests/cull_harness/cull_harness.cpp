// TEST INFRASTRUCTURE: host build of the cull header (hpp-fcl_amd/csrc/hfcl_cull.hpp) with g++, built by tests/test_scene_cull_cpu.py
// into a temporary directory.  ch_world_boxes* run k_cull_aabbs' lanes; ch_cull runs the workgroups, waves and lanes of k_cull_mark,
// k_cull_scan and k_cull_emit chunk by chunk; ch_fold_listed* run k_scene_fold_listed / k_scene_fold_listed_combine.
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_cull.hpp"

using namespace hfcl;

static void local_boxes(const hfcl_shape* shapes, size_t n_shapes, const double* verts, std::vector<double>& out) {
  out.resize(6 * n_shapes);
  for (size_t i = 0; i < n_shapes; ++i) {
    const Box3 b = shape_local_box(shapes[i], verts);
    for (int k = 0; k < 3; ++k) {
      out[6 * i + k] = b.lo[k];
      out[6 * i + 3 + k] = b.hi[k];
    }
  }
}

extern "C" void ch_world_boxes(const hfcl_shape* shapes, size_t n_shapes, const double* verts, const uint32_t* object_shape,
                               const double* tf, uint64_t n_objects, uint64_t n_rows, double* out) {
  std::vector<double> L;
  local_boxes(shapes, n_shapes, verts, L);
  for (uint64_t r = 0; r < n_rows; ++r)
    cull_world_box(tf + 12 * r, tf + 12 * r + 9, L.data() + 6 * size_t(object_shape[r % n_objects]), out + 6 * r);
}
extern "C" void ch_world_boxes_f32(const hfcl_shape* shapes, size_t n_shapes, const double* verts, const uint32_t* object_shape,
                                   const float* pose, uint64_t n_objects, uint64_t n_rows, double* out) {
  std::vector<double> L;
  local_boxes(shapes, n_shapes, verts, L);
  for (uint64_t r = 0; r < n_rows; ++r) cull_world_box_quat(pose + 7 * r, L.data() + 6 * size_t(object_shape[r % n_objects]), out + 6 * r);
}
extern "C" void ch_mesh_box(const double* verts, size_t n, double* out) {
  const Box3 b = mesh_local_box(verts, n);
  for (int k = 0; k < 3; ++k) {
    out[k] = b.lo[k];
    out[3 + k] = b.hi[k];
  }
}
extern "C" int ch_is_identity(const double* R) { return cull_rotation_is_identity(R) ? 1 : 0; }

// mark, scan, emit over the chunks of the flat range; returns the count
extern "C" uint64_t ch_cull(const double* boxes, const uint32_t* pairs, uint32_t n_pairs, uint64_t n_objects, uint64_t n_conf, double inflate,
                            uint64_t chunk, uint64_t* ids, uint64_t capacity, uint64_t* conf_begin) {
  const uint64_t total = n_conf * n_pairs;
  uint64_t running = 0, n_listed = 0;
  for (uint64_t q0 = 0; q0 < total; q0 += chunk) {
    const uint32_t m = uint32_t(q0 + chunk < total ? chunk : total - q0);
    uint64_t c0;
    uint32_t p0;
    scene_query(q0, n_pairs, c0, p0);
    const uint32_t n_blocks = (m + CULL_BLOCK - 1) / CULL_BLOCK;
    std::vector<uint64_t> words((m + 63) / 64), offsets(n_blocks);
    std::vector<uint32_t> counts(n_blocks);
    for (uint32_t b = 0; b < n_blocks; ++b) {  // k_cull_mark
      uint32_t n = 0;
      for (uint32_t wave = 0; wave < CULL_WAVES; ++wave) {
        uint64_t ballot = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint32_t row = b * CULL_BLOCK + wave * 64 + lane;
          if (row >= m) continue;
          uint64_t c;
          uint32_t p;
          scene_query_from(c0, p0, row, n_pairs, c, p);
          const double* base = boxes + 6 * (c * n_objects);
          if (cull_keep(base + 6 * size_t(pairs[2 * size_t(p)]), base + 6 * size_t(pairs[2 * size_t(p) + 1]), inflate)) ballot |= uint64_t(1) << lane;
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
      if (keep && ids && pos < capacity) ids[pos] = q;
      uint64_t c;
      uint32_t p;
      scene_query_from(c0, p0, row, n_pairs, c, p);
      if (conf_begin && p == 0u) conf_begin[c] = pos;
      if (q == total - 1) {
        n_listed = pos + (keep ? 1u : 0u);
        if (conf_begin) conf_begin[n_conf] = n_listed;
      }
    }
  }
  return n_listed;
}

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
static void store(hfcl_scene_summary* summary, uint64_t c, const hfcl_scene_summary& part) {
  hfcl_scene_summary s = summary[c];
  scene_fold_merge(s, part);
  summary[c] = s;
}

template <typename R, typename M>
static void fold_listed(const R* rec, const uint64_t* ids, const uint64_t* conf_begin, uint64_t n_listed, uint64_t n_conf, uint32_t n_pairs,
                        M margin, int collide, uint64_t chunk, hfcl_scene_summary* summary) {
  for (uint64_t c = 0; c < n_conf; ++c) scene_summary_init(summary[c]);
  const uint32_t shares = scene_shares(n_pairs);
  for (uint64_t k0 = 0; k0 < n_listed; k0 += chunk) {
    const uint64_t k1 = k0 + chunk < n_listed ? k0 + chunk : n_listed;
    uint64_t c_lo, confs;
    scene_listed_span(ids[k0], ids[k1 - 1], n_pairs, n_conf, c_lo, confs);
    std::vector<hfcl_scene_summary> partials(confs * shares);
    for (uint64_t w = 0; w < confs * shares; ++w) {
      const uint64_t c = c_lo + w / shares;
      uint64_t lo, hi;
      scene_listed_piece(conf_begin[c], conf_begin[c + 1], uint32_t(w % shares), k0, k1, lo, hi);
      hfcl_scene_summary lanes[64];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        scene_summary_init(lanes[lane]);
        for (uint64_t k = lo + lane; k < hi; k += 64u)
          scene_fold_record(lanes[lane], scene_value(rec[k].distance, margin, collide != 0), rec[k].status, uint32_t(ids[k] - c * n_pairs));
      }
      wave_reduce(lanes);
      if (shares > 1u)
        partials[w] = lanes[0];
      else if (hi > lo)
        store(summary, c, lanes[0]);
    }
    if (shares <= 1u) continue;
    for (uint64_t w = 0; w < confs; ++w) {
      hfcl_scene_summary lanes[64];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        scene_summary_init(lanes[lane]);
        for (uint32_t g = lane; g < shares; g += 64u) scene_fold_merge(lanes[lane], partials[w * shares + g]);
      }
      wave_reduce(lanes);
      store(summary, c_lo + w, lanes[0]);
    }
  }
}
extern "C" void ch_fold_listed(const hfcl_result* rec, const uint64_t* ids, const uint64_t* conf_begin, uint64_t n_listed, uint64_t n_conf,
                               uint32_t n_pairs, double margin, int collide, uint64_t chunk, hfcl_scene_summary* summary) {
  fold_listed(rec, ids, conf_begin, n_listed, n_conf, n_pairs, margin, collide, chunk, summary);
}
extern "C" void ch_fold_listed_f32(const hfcl_result_f32* rec, const uint64_t* ids, const uint64_t* conf_begin, uint64_t n_listed,
                                   uint64_t n_conf, uint32_t n_pairs, double margin, int collide, uint64_t chunk, hfcl_scene_summary* summary) {
  fold_listed(rec, ids, conf_begin, n_listed, n_conf, n_pairs, float(margin), collide, chunk, summary);
}
