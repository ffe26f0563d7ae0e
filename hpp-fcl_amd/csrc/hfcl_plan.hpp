// hfcl_plan.hpp -- the chunk plan of the host pipeline (hfcl_host.hip: host_batch).  Plain C++, no HIP header: tests/plan_harness builds it
// with the host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

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
