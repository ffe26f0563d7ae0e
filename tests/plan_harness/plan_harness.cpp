// TEST INFRASTRUCTURE: host build of the host pipeline's chunk plan (hpp-fcl_amd/csrc/hfcl_plan.hpp) with g++, built by
// tests/test_host_plan_cpu.py into a temporary directory.  ph_plan_chunks writes up to `cap` bounds and returns how many the plan has.
#include <cstdint>

#include "../../hpp-fcl_amd/csrc/hfcl_plan.hpp"

extern "C" uint64_t ph_plan_chunks(uint64_t n, uint64_t pipe_chunk, int pipelined, int f32, uint64_t* out, uint64_t cap) {
  const std::vector<size_t> b = plan_chunks(size_t(n), size_t(pipe_chunk), pipelined != 0, f32 != 0);
  for (size_t k = 0; k < b.size() && k < cap; ++k) out[k] = b[k];
  return b.size();
}
