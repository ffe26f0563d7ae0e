// Host build of hpp-fcl_amd/csrc/hfcl_epa_pool.hpp: simulated waves of k_epa_loop<float, 8, 17> hand out the blocks of a batch with the
// header's arithmetic, in a seeded random interleaving of their refills and atomics.  A stand-alone program (tests/test_epa_pool_cpu.py
// builds and runs it, once more under -fsanitize=address,undefined): one line per case,
//   cnt grid share k min_refills S len ok taken_twice never_taken out_of_range max_empty_draws atomics
// usage: epa_pool_harness <seed> <k> <share> <min_refills> <grid> <cnt> [<cnt> ...]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_epa_pool.hpp"

using namespace hfcl;

namespace {
constexpr uint32_t G = 8;           // groups of a wave
constexpr uint32_t REFILL_MIN = 2;  // HFCL_EPA_LOOP_REFILL_MIN

struct Wave {
  uint32_t id = 0, next = 0, dry = 0, at = 0, n_live = 0;
  // a refill from the pool in progress: 0 none, 2 an atomic is due
  int phase = 0;
  uint32_t want = 0, empty_draws = 0;
  bool done = false;
};

struct Sim {
  uint32_t cnt, grid, k;
  EpaPoolPlan pool;
  std::vector<uint32_t> counters, taken;
  uint64_t out_of_range = 0, atomics = 0;
  std::mt19937 rng;

  void take(uint32_t block) {
    if (block < cnt) ++taken[block];
    else ++out_of_range;
  }
  // one event of wave w: the kernel's loop, cut where it touches memory other waves write
  void step(Wave& w) {
    const uint32_t full = epa_pool_full_mask(k);
    if (w.phase == 0) {
      const bool strided = w.next < pool.S;
      const bool more = strided || w.dry != full;
      if (!(w.n_live == 0 || (more && G - w.n_live >= REFILL_MIN))) {
        // trips: some of the live groups end (all of them once nothing is left to take)
        const uint32_t need = more ? (G - w.n_live >= REFILL_MIN ? 0u : REFILL_MIN - (G - w.n_live)) : w.n_live;
        const uint32_t ending = need + (w.n_live > need ? uint32_t(rng() % (w.n_live - need + 1)) : 0u);
        w.n_live -= ending ? ending : 1u;
        return;
      }
      if (w.n_live == 0 && !more) {
        w.done = true;
        return;
      }
      w.want = G - w.n_live;
      if (strided) {
        for (uint32_t rank = 0; rank < w.want; ++rank) {
          const uint32_t it = w.next + rank * grid;
          if (it < pool.S) {
            take(it);
            ++w.n_live;
          }
        }
        w.next += w.want * grid;
        return;
      }
      if (w.dry != full) w.phase = 2;
      else if (w.n_live == 0) w.done = true;
      return;
    }
    // one atomicAdd on the first range that is not known to be dry
    w.at = epa_pool_pick(w.dry, w.at, k);
    const uint32_t t = counters[w.at];
    counters[w.at] += w.want;
    ++atomics;
    const uint32_t len_at = epa_pool_range_len(pool, cnt, w.at);
    const uint32_t n = epa_pool_take(t, w.want, len_at);
    if (epa_pool_drained(t, w.want, len_at)) w.dry |= 1u << w.at;
    if (n) {
      for (uint32_t rank = 0; rank < n; ++rank) take(epa_pool_range_base(pool, w.at) + t + rank);
      w.n_live += n;
      w.phase = 0;
    } else {
      ++w.empty_draws;
      if (w.dry == full) w.phase = 0;
    }
  }
};

int run_case(uint32_t seed, uint32_t k, uint32_t share, uint32_t min_refills, uint32_t grid_max, uint32_t cnt) {
  // (the launcher's grid: a wave per G blocks of the batch at most -- here of the polytopes, which is what matters to the hand-out)
  const uint32_t grid = grid_max;
  Sim s;
  s.cnt = cnt;
  s.grid = grid;
  s.k = k;
  s.pool = epa_pool_plan(cnt, grid, G, share, min_refills, k);
  s.counters.assign(k, 0u);
  s.taken.assign(cnt, 0u);
  s.rng.seed(seed ^ (cnt * 2654435761u) ^ (grid << 7) ^ (share << 3) ^ k);
  std::vector<Wave> waves(grid);
  std::vector<uint32_t> running(grid);
  for (uint32_t i = 0; i < grid; ++i) {
    waves[i].id = i;
    waves[i].next = i;
    waves[i].at = i % k;
    waves[i].dry = s.pool.len ? 0u : epa_pool_full_mask(k);
    running[i] = i;
  }
  while (!running.empty()) {
    const size_t pick = s.rng() % running.size();
    Wave& w = waves[running[pick]];
    s.step(w);
    if (w.done) {
      running[pick] = running.back();
      running.pop_back();
    }
  }
  uint64_t twice = 0, never = 0;
  for (uint32_t b = 0; b < cnt; ++b) {
    twice += s.taken[b] > 1u;
    never += s.taken[b] == 0u;
  }
  uint32_t max_empty = 0;
  for (const Wave& w : waves) max_empty = w.empty_draws > max_empty ? w.empty_draws : max_empty;
  const bool ok = twice == 0 && never == 0 && s.out_of_range == 0;
  printf("%u %u %u %u %u %u %u %d %llu %llu %llu %u %llu\n", cnt, grid, share, k, min_refills, s.pool.S, s.pool.len, ok ? 1 : 0,
         (unsigned long long)twice, (unsigned long long)never, (unsigned long long)s.out_of_range, max_empty, (unsigned long long)s.atomics);
  return ok ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: %s <seed> <k> <share> <min_refills> <grid> <cnt> [<cnt> ...]\n", argv[0]);
    return 2;
  }
  const uint32_t seed = uint32_t(strtoul(argv[1], nullptr, 10)), k = uint32_t(strtoul(argv[2], nullptr, 10));
  const uint32_t share = uint32_t(strtoul(argv[3], nullptr, 10)), min_refills = uint32_t(strtoul(argv[4], nullptr, 10));
  const uint32_t grid = uint32_t(strtoul(argv[5], nullptr, 10));
  if (k == 0 || k > 32 || grid == 0) return 2;
  int bad = 0;
  for (int a = 6; a < argc; ++a) bad += run_case(seed, k, share, min_refills, grid, uint32_t(strtoul(argv[a], nullptr, 10)));
  return bad ? 1 : 0;
}
