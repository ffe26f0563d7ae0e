// TEST INFRASTRUCTURE: host build of the host units' planning arithmetic (hpp-fcl_amd/csrc/hfcl_plan.hpp) with g++, built by
// tests/test_host_plan_cpu.py into a temporary directory.  ph_plan_chunks writes up to `cap` bounds and returns how many the plan has; the
// others are the header's functions of the scene calls as they stand.
#include <cstdint>

#include "../../hpp-fcl_amd/csrc/hfcl_plan.hpp"

extern "C" uint64_t ph_plan_chunks(uint64_t n, uint64_t pipe_chunk, int pipelined, int f32, uint64_t* out, uint64_t cap) {
  const std::vector<size_t> b = plan_chunks(size_t(n), size_t(pipe_chunk), pipelined != 0, f32 != 0);
  for (size_t k = 0; k < b.size() && k < cap; ++k) out[k] = b[k];
  return b.size();
}

extern "C" uint64_t ph_equal_chunks(uint64_t total, uint64_t option, uint64_t auto_max) { return equal_chunks(size_t(total), size_t(option), size_t(auto_max)); }
extern "C" uint64_t ph_scene_chunk_size(uint64_t total, uint64_t option) { return scene_chunk_size(size_t(total), size_t(option)); }
extern "C" uint64_t ph_cull_chunk_size(uint64_t total, uint64_t option) { return cull_chunk_size(size_t(total), size_t(option)); }
extern "C" uint64_t ph_scene_pieces_bound(uint64_t n_pairs, uint64_t m) { return scene_pieces_bound(size_t(n_pairs), size_t(m)); }
extern "C" uint64_t ph_scene_listed_pieces_bound(uint64_t n_pairs, uint64_t n_conf) { return scene_listed_pieces_bound(size_t(n_pairs), size_t(n_conf)); }
extern "C" uint64_t ph_list_capacity_guess(uint64_t total) { return list_capacity_guess(size_t(total)); }
extern "C" uint64_t ph_scene_piece_of(uint64_t q, uint32_t n_pairs) { return hfcl::scene_piece_of(q, n_pairs); }

// the sweep plans: the members in the order of the header's structs, `small` / the geometry flattened
extern "C" uint64_t ph_sweep_conf_per_chunk(uint64_t n_conf, uint64_t per, uint32_t blocks_per_conf) { return sweep_conf_per_chunk(size_t(n_conf), per, blocks_per_conf); }
extern "C" uint64_t ph_env_sweep_span(uint32_t span_option, uint32_t tiles, uint64_t n_blocks, int n_cus) { return env_sweep_span(span_option, tiles, n_blocks, n_cus); }
// out: small, rows_per_block, blocks_per_conf, n_blocks, per, conf_per_chunk, chunk_rows
extern "C" void ph_self_sweep_plan(uint32_t n, uint64_t n_conf, uint32_t small_max_option, uint64_t chunk_option, uint64_t* out) {
  const SelfSweepPlan p = self_sweep_plan(n, size_t(n_conf), small_max_option, chunk_option);
  const uint64_t v[7] = {p.small, p.geo.rows_per_block, p.geo.blocks_per_conf, p.n_blocks, p.per, p.conf_per_chunk, p.chunk_rows};
  for (int k = 0; k < 7; ++k) out[k] = v[k];
}
// out: blocks_per_conf, tiles_moving, tiles, span_len, n_spans, n_blocks, per, conf_per_chunk, chunk_rows, scan_rows
extern "C" void ph_env_sweep_plan(uint32_t nm, uint32_t ne, uint64_t n_conf, uint32_t span_option, int n_cus, uint64_t chunk_option, uint64_t* out) {
  const EnvSweepPlan p = env_sweep_plan(nm, ne, size_t(n_conf), span_option, n_cus, chunk_option);
  const uint64_t v[10] = {p.rows.blocks_per_conf, p.geo.tiles_moving, p.geo.tiles, p.geo.span_len, p.geo.n_spans, p.n_blocks, p.per, p.conf_per_chunk, p.chunk_rows, p.scan_rows};
  for (int k = 0; k < 10; ++k) out[k] = v[k];
}
