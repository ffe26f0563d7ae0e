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
