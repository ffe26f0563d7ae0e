// hfcl_plan.hpp -- the planning arithmetic of the host units: the chunk plan of the host pipeline (hfcl_host.hip: host_batch), and the chunk
// sizes, fold-partial bounds, list capacities and sweep plans of the scene calls (hfcl_host_scene.hip).  Plain C++, no HIP header:
// tests/plan_harness builds it with the host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "hfcl_env.hpp"
#include "hfcl_pairs_sorted.hpp"
#include "hfcl_scene.hpp"

// Chunk bounds of a host batch of n > 0 pairs: chunk k = [bounds[k], bounds[k + 1]), bounds[0] = 0, bounds.back() = n.
// Chunks: large enough that a chunk's fixed costs (a dozen launches, ~0.1 ms) vanish, small enough that the pipeline
// has several chunks to overlap.  The link is busy from the first byte to the last only if the first chunk is small
// (nothing computes until it has arrived) and the last one too (nothing overlaps its way back): the sizes ramp up
// geometrically from 16k pairs to the steady size and down again (1M pairs: 6.4 -> see profiles/r03_c).
// pipe_chunk: option pipe_chunk (pairs per chunk; 0 = automatic); pipelined = false: one chunk.
inline std::vector<size_t> plan_chunks(size_t n, size_t pipe_chunk, bool pipelined, bool f32) {
  std::vector<size_t> bounds;
  bounds.push_back(0);
  if (pipelined && pipe_chunk) {
    for (size_t lo = 0; lo < n; lo += pipe_chunk) bounds.push_back(std::min(n, lo + pipe_chunk));
  } else if (pipelined && f32 && n > (size_t(1) << 16)) {
    // fp32: 108 B per pair cross the link -- a quarter of the time the kernels take -- and those kernels live on latency, so a chunk a quarter the
    // size takes 0.44 of the time, not 0.25: few, large chunks (1M convex32 pairs: three chunks 3.7 ms, the fp64 policy's ten 6.4 ms, one chunk 4.1 ms)
    const size_t c = std::min<size_t>(std::max<size_t>((n + 2) / 3, size_t(1) << 16), size_t(1) << 19);
    for (size_t lo = 0; lo < n; lo += c) bounds.push_back(std::min(n, lo + c));
  } else if (pipelined && n > (size_t(1) << 16)) {
    const size_t steady = std::min<size_t>(std::max<size_t>(n / 6, size_t(1) << 16), size_t(1) << 18);
    std::vector<size_t> up;    // 16k, 32k, ... below the steady size
    for (size_t c = size_t(1) << 14; c < steady; c *= 2) up.push_back(c);
    size_t ramp = 0;
    for (size_t c : up) ramp += c;
    while (!up.empty() && 2 * ramp + steady > n) {  // a batch too small for the whole ramp: shorten it from the top
      ramp -= up.back();
      up.pop_back();
    }
    size_t lo = 0;
    for (size_t c : up) bounds.push_back(lo += c);
    const size_t mid_end = n - ramp;
    while (mid_end - lo > steady + steady / 2) bounds.push_back(lo += steady);
    if (mid_end > lo) bounds.push_back(lo = mid_end);
    for (size_t k = up.size(); k-- > 0;) bounds.push_back(lo += up[k]);
  } else {
    bounds.push_back(n);
  }
  return bounds;
}

// ---- scene calls (hfcl_host_scene.hip) ------------------------------------------------------------------------------------
// queries per chunk of a call of `total` > 0 queries: the option as given, or (0) equal chunks of at most auto_max
inline size_t equal_chunks(size_t total, size_t option, size_t auto_max) {
  if (option) return std::min(option, total);
  const size_t n_chunks = (total + auto_max - 1) / auto_max;
  return (total + n_chunks - 1) / n_chunks;
}
// ... of a scene call (option scene_chunk; a chunk's size goes to the kernels in 32 bits), of the cull (option scene_cull_chunk)
inline size_t scene_chunk_size(size_t total, size_t option) { return std::min<size_t>(equal_chunks(total, option, size_t(1) << 21), 0xFFFFFFF0ull); }
inline size_t cull_chunk_size(size_t total, size_t option) { return equal_chunks(total, option, size_t(1) << 22); }

// fold partials a chunk of m queries of the flat range can need: none when a pair list is one piece
inline size_t scene_pieces_bound(size_t n_pairs, size_t m) {
  if (hfcl::scene_shares(uint32_t(n_pairs)) <= 1u) return 0;
  // whole pieces inside the chunk, a cut one at either end, and one more cut per configuration boundary inside it
  return m / hfcl::SCENE_FOLD_SHARE + 2 + 2 * (m / n_pairs + 2);
}
// ... a chunk of a list can need: a slot per piece of every configuration it can span -- any number of them, whatever its length, since
// configurations without an entry lie in between (none when a pair list is one piece)
inline size_t scene_listed_pieces_bound(size_t n_pairs, size_t n_conf) {
  const uint32_t shares = hfcl::scene_shares(uint32_t(n_pairs));
  return shares <= 1u ? 0 : n_conf * shares;
}
// entries a list of the survivors of `total` queries is first given room for (a longer one is made again in a buffer of its size)
inline size_t list_capacity_guess(size_t total) { return std::min<size_t>(total, std::max<size_t>(total / 8, 4096)); }

// ---- the sweeps that make a list of pairs (hfcl_host_scene.hip: SelfSweep, EnvSweep) ---------------------------------------------
// (a sweep has rows: n_conf > 0 and n > 0 / nm > 0 -- the callers answer an empty table before they plan)
// configurations whose boxes a chunk of `per` row blocks can touch: the whole ones inside it and a cut one at either end
inline size_t sweep_conf_per_chunk(size_t n_conf, uint64_t per, uint32_t blocks_per_conf) {
  return std::min<size_t>(n_conf, size_t(per / blocks_per_conf) + 2);
}
// The all-pairs sweep over n_conf configurations of n objects (hfcl_pairs.hpp): small -- a wave per configuration -- up to the option
// scene_pairs_small_max (at most PAIRS_SMALL_MAX); `per` row blocks a chunk (chunk_option: option scene_cull_chunk, rows); chunk_rows:
// table rows a chunk's row arrays hold
struct SelfSweepPlan {
  bool small;
  hfcl::PairsGeometry geo;
  uint64_t n_blocks, per;
  size_t conf_per_chunk;
  uint64_t chunk_rows;
};
inline SelfSweepPlan self_sweep_plan(uint32_t n, size_t n_conf, uint32_t small_max_option, uint64_t chunk_option) {
  SelfSweepPlan p;
  p.small = n <= std::min(small_max_option, hfcl::PAIRS_SMALL_MAX);
  p.geo = hfcl::pairs_geometry(n, p.small);
  p.n_blocks = uint64_t(n_conf) * p.geo.blocks_per_conf;
  p.per = hfcl::pairs_chunk_blocks(p.geo, p.n_blocks, chunk_option);
  p.conf_per_chunk = sweep_conf_per_chunk(n_conf, p.per, p.geo.blocks_per_conf);
  p.chunk_rows = std::min<uint64_t>(p.per * p.geo.rows_per_block, uint64_t(n_conf) * n);
  return p;
}
// The sort-and-sweep form of the same list (hfcl_pairs_sorted.hpp; option scene_pairs_sorted) over n_conf configurations of n >= 2 objects:
// chunks of whole configurations -- chunk_option rows (option scene_cull_chunk; 0: PAIRS_CHUNK_ROWS, the call in equal chunks), at least
// one configuration.  conf_bits: bits of a configuration's index in its chunk, obj_bits: of an object's index -- the sorted words have
// 32 + conf_bits and conf_bits + 2 obj_bits bits in use; blocks_per_conf: workgroups of PAIRS_ROWS sorted positions
struct SortedSweepPlan {
  size_t conf_per_chunk, n_chunks;
  uint64_t chunk_rows;
  uint32_t blocks_per_conf, conf_bits, obj_bits;
};
inline SortedSweepPlan sorted_sweep_plan(uint32_t n, size_t n_conf, uint64_t chunk_option) {
  SortedSweepPlan p;
  const uint64_t rows = chunk_option ? chunk_option : hfcl::PAIRS_CHUNK_ROWS;
  p.conf_per_chunk = std::min<size_t>(n_conf, std::max<size_t>(size_t(rows / n), 1));
  p.n_chunks = (n_conf + p.conf_per_chunk - 1) / p.conf_per_chunk;
  if (!chunk_option) p.conf_per_chunk = (n_conf + p.n_chunks - 1) / p.n_chunks;
  p.chunk_rows = uint64_t(p.conf_per_chunk) * n;
  p.blocks_per_conf = (n + hfcl::PAIRS_ROWS - 1u) / hfcl::PAIRS_ROWS;
  p.conf_bits = hfcl::psort_bits(p.conf_per_chunk);
  p.obj_bits = hfcl::psort_bits(n);
  return p;
}
// tiles per span of the environment sweep: the option scene_env_span as given, or (0) env_auto_span for the call's row blocks
inline uint32_t env_sweep_span(uint32_t span_option, uint32_t tiles, uint64_t n_blocks, int n_cus) {
  return span_option ? span_option : hfcl::env_auto_span(tiles, n_blocks, uint32_t(std::max(n_cus, 1)), hfcl::ENV_AUTO_PER_CU);
}
// The sweep of nm moving rows against their own and ne environment columns (hfcl_env.hpp): rows -- the row blocks, never small --, geo --
// the column tiles in spans --, `per` row blocks a chunk; chunk_rows: moving rows of a chunk, scan_rows: its (row, span) counts
struct EnvSweepPlan {
  hfcl::PairsGeometry rows;
  hfcl::EnvGeometry geo;
  uint64_t n_blocks, per;
  size_t conf_per_chunk;
  uint64_t chunk_rows, scan_rows;
};
inline EnvSweepPlan env_sweep_plan(uint32_t nm, uint32_t ne, size_t n_conf, uint32_t span_option, int n_cus, uint64_t chunk_option) {
  EnvSweepPlan p;
  p.rows = hfcl::pairs_geometry(nm, false);
  p.n_blocks = uint64_t(n_conf) * p.rows.blocks_per_conf;
  p.geo = hfcl::env_geometry(nm, ne, env_sweep_span(span_option, hfcl::env_geometry(nm, ne, 0u).tiles, p.n_blocks, n_cus));
  p.per = hfcl::env_chunk_blocks(p.geo, p.n_blocks, chunk_option);
  p.conf_per_chunk = sweep_conf_per_chunk(n_conf, p.per, p.rows.blocks_per_conf);
  p.chunk_rows = std::min<uint64_t>(p.per * p.rows.rows_per_block, uint64_t(n_conf) * nm);
  p.scan_rows = p.chunk_rows * p.geo.n_spans;
  return p;
}
