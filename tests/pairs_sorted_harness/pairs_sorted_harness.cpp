// TEST INFRASTRUCTURE: host build of the sort-and-sweep header (hpp-fcl_amd/csrc/hfcl_pairs_sorted.hpp) and of its chunk plan
// (hfcl_plan.hpp: sorted_sweep_plan) with g++, built by tests/test_scene_pairs_sorted_cpu.py into a temporary directory.  psh_keys runs the
// key functions; psh_self_pairs the whole pipeline chunk by chunk as hfcl_host_scene.hip cuts the call -- axis, keys, std::stable_sort,
// gather and window ends, the sweep over the windows (count, then the emitted words), the sort of the words, the list -- with the
// header's functions where the kernels of hfcl_k_pairs_sorted.hip use them; psh_plan the plan.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_plan.hpp"

using namespace hfcl;

// per value: the key, the fp32 number it stands for, the window-end key
extern "C" void psh_keys(const double* x, uint64_t n, uint32_t* key, float* rounded, uint32_t* end) {
  for (uint64_t k = 0; k < n; ++k) {
    key[k] = psort_key(x[k]);
    rounded[k] = psort_orderable_inverse(key[k]);
    end[k] = psort_end(x[k]);
  }
}
extern "C" uint32_t psh_orderable(float f) { return psort_orderable(f); }

extern "C" void psh_plan(uint32_t n, uint64_t n_conf, uint64_t chunk_option, uint64_t* out) {
  const SortedSweepPlan p = sorted_sweep_plan(n, size_t(n_conf), chunk_option);
  out[0] = p.conf_per_chunk;
  out[1] = p.n_chunks;
  out[2] = p.chunk_rows;
  out[3] = p.blocks_per_conf;
  out[4] = p.conf_bits;
  out[5] = p.obj_bits;
}

// the whole call.  axis: 0, 1, 2 or PSORT_AXIS_AUTO; group / collides: nullptr or the groups; pairs: nullptr (count only) or 2 * capacity
// words; axes_out: nullptr or the axis of every configuration.  Returns the count.
extern "C" uint64_t psh_self_pairs(const double* boxes, uint32_t n, uint64_t n_conf, double inflate, uint64_t chunk_rows, uint32_t axis_option,
                                   const uint8_t* group, const uint64_t* collides, uint32_t* pairs, uint64_t capacity, uint64_t* conf_begin,
                                   uint64_t* n_chunks_out, uint32_t* axes_out) {
  uint64_t listed = 0, n_chunks = 0;
  if (conf_begin) memset(conf_begin, 0, (n_conf + 1) * sizeof(uint64_t));
  if (n_conf == 0 || n < 2) {
    if (n_chunks_out) *n_chunks_out = 0;
    return 0;
  }
  const SortedSweepPlan plan = sorted_sweep_plan(n, size_t(n_conf), chunk_rows);
  for (uint64_t c0 = 0; c0 < n_conf; c0 += plan.conf_per_chunk, ++n_chunks) {
    const uint64_t confs = std::min<uint64_t>(plan.conf_per_chunk, n_conf - c0);
    const uint64_t rows = confs * n;
    const double* chunk = boxes + 6 * c0 * n;
    // the axis of every configuration of the chunk
    std::vector<uint32_t> conf_axis(confs, axis_option);
    for (uint64_t c = 0; c < confs && axis_option >= PSORT_AXIS_AUTO; ++c) {
      const double inf = __builtin_inf();
      double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
      for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
          double centre;
          if (psort_centre(chunk + 6 * (c * n + i), k, centre)) {
            lo[k] = centre < lo[k] ? centre : lo[k];
            hi[k] = centre > hi[k] ? centre : hi[k];
          }
        }
      conf_axis[c] = psort_pick_axis(lo, hi);
    }
    for (uint64_t c = 0; axes_out && c < confs; ++c) axes_out[c0 + c] = conf_axis[c];
    // keys, the stable sort
    std::vector<uint64_t> order(rows), words(rows);
    for (uint64_t r = 0; r < rows; ++r) {
      const uint32_t c = uint32_t(r / n);
      words[r] = psort_word(c, psort_key(chunk[6 * r + conf_axis[c]] - inflate));
      order[r] = r;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return words[x] < words[y]; });
    std::vector<uint64_t> keys(rows);
    std::vector<uint32_t> ids(rows), ends(rows);
    std::vector<double> grown(6 * rows);
    for (uint64_t p = 0; p < rows; ++p) {
      keys[p] = words[order[p]];
      ids[p] = uint32_t(order[p] % n);
    }
    // gather, window ends
    for (uint64_t p = 0; p < rows; ++p) {
      const uint64_t c = p / n;
      pairs_grow(chunk + 6 * (c * n + ids[p]), inflate, &grown[6 * p]);
      ends[p] = psort_upper_bound(keys.data() + c * n, n, psort_end(grown[6 * p + 3 + conf_axis[c]]));
    }
    // the sweep over the windows: every pair once, by its earlier position
    std::vector<uint64_t> emitted;
    for (uint64_t c = 0; c < confs; ++c) {
      const uint64_t first = c * n;
      for (uint32_t p = 0; p < n; ++p)
        for (uint32_t q = p + 1; q < ends[first + p]; ++q) {
          const uint32_t a = ids[first + p], b = ids[first + q];
          if (!cull_boxes_touch(&grown[6 * (first + p)], &grown[6 * (first + q)])) continue;
          if (group && !psort_allowed(a, group[a], b, group[b], collides)) continue;
          emitted.push_back(psort_pair_word(uint32_t(c), a, b, plan.obj_bits));
        }
    }
    std::sort(emitted.begin(), emitted.end());
    for (uint64_t e = 0; e < emitted.size(); ++e) {
      const uint64_t c = emitted[e] >> (2 * plan.obj_bits);
      if (conf_begin) ++conf_begin[c0 + c + 1];
      if (pairs && listed + e < capacity) psort_pair_of(emitted[e], plan.obj_bits, pairs[2 * (listed + e)], pairs[2 * (listed + e) + 1]);
    }
    listed += emitted.size();
  }
  for (uint64_t c = 0; conf_begin && c < n_conf; ++c) conf_begin[c + 1] += conf_begin[c];
  if (n_chunks_out) *n_chunks_out = n_chunks;
  return listed;
}
