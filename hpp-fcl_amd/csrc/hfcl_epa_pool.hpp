// hfcl_epa_pool.hpp -- how k_epa_loop<float, 8, 17> (hfcl_k_epa.hip) hands out the blocks of a batch's cnt polytopes: the arithmetic alone.
// Blocks [0, S) are strided over the grid's waves (wave w: w, w + grid, ...), fixed before any iteration count is known; the kernel lasts as
// long as its unluckiest wave.  Blocks [S, cnt) -- the pool -- are drawn by ticket as waves run out of their own: K ranges of equal length,
// a counter each (zeroed with the batch's counters), a ticket = atomicAdd(counter, blocks wanted).  Counters only grow, so a counter at or
// past its range's length means "dry for good": no wave ever waits for another, and a wave makes at most K draws that return nothing.
// Plain C++ behind HFCL_HD, no HIP header: tests/epa_pool_harness builds it with the host compiler and replays simulated waves;
// tools/sched_model.py: model_epa is the same arithmetic on the oracle's iteration counts.
#pragma once
#include <cstdint>

#include "hfcl_math.hpp"

namespace hfcl {

constexpr int EPA_POOL_K = 16;            // ranges (and counters) of the kernel; the functions below take any k <= 32
constexpr int EPA_POOL_STRIDE_WORDS = 32; // a counter alone in a 128-byte line

struct EpaPoolPlan {
  uint32_t S;    // blocks [0, S) are strided; S is a multiple of the grid, or cnt (no pool)
  uint32_t len;  // length of a range (the last ones may be shorter or empty); 0: no pool
};

// share_pct: percent of the blocks that go to the pool (0: none -- the static schedule).  A batch with fewer than min_refills full refills
// per wave (grid * groups * min_refills blocks) keeps the static schedule too.
HFCL_HD EpaPoolPlan epa_pool_plan(uint32_t cnt, uint32_t grid, uint32_t groups, uint32_t share_pct, uint32_t min_refills, uint32_t k) {
  EpaPoolPlan p{cnt, 0u};
  if (share_pct == 0u || grid == 0u || k == 0u) return p;
  if (uint64_t(cnt) < uint64_t(grid) * groups * min_refills) return p;
  const uint32_t pool = uint32_t(uint64_t(cnt) * share_pct / 100u);
  p.S = (cnt - pool) / grid * grid;
  p.len = uint32_t((uint64_t(cnt - p.S) + k - 1u) / k);
  return p;
}
// range j = [epa_pool_range_base, + epa_pool_range_len)
HFCL_HD uint32_t epa_pool_range_base(const EpaPoolPlan& p, uint32_t j) { return p.S + j * p.len; }
HFCL_HD uint32_t epa_pool_range_len(const EpaPoolPlan& p, uint32_t cnt, uint32_t j) {
  const uint64_t lo = uint64_t(p.S) + uint64_t(j) * p.len;
  if (lo >= cnt) return 0u;
  const uint64_t left = cnt - lo;
  return left < p.len ? uint32_t(left) : p.len;
}
// The take of ticket t for `want` blocks in a range of length len: the blocks [t, t + result) of the range; 0: nothing left, for good.
HFCL_HD uint32_t epa_pool_take(uint32_t t, uint32_t want, uint32_t len) {
  if (t >= len) return 0u;
  const uint32_t left = len - t;
  return want < left ? want : left;
}
// ... and whether that ticket was the range's last (the wave that drew it marks the range dry)
HFCL_HD bool epa_pool_drained(uint32_t t, uint32_t want, uint32_t len) { return uint64_t(t) + want >= len; }
// the first range at or after `at` (cyclically) whose bit in `dry` is clear; dry must not be full
HFCL_HD uint32_t epa_pool_pick(uint32_t dry, uint32_t at, uint32_t k) {
  for (uint32_t s = 0; s < k; ++s) {
    const uint32_t j = at + s < k ? at + s : at + s - k;
    if (!((dry >> j) & 1u)) return j;
  }
  return k;
}
HFCL_HD uint32_t epa_pool_full_mask(uint32_t k) { return k >= 32u ? 0xFFFFFFFFu : (1u << k) - 1u; }

}  // namespace hfcl
