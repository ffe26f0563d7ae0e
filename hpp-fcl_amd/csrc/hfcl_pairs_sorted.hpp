// hfcl_pairs_sorted.hpp -- the self-collision pairs of a scene per configuration by sort and sweep along one axis (option
// scene_pairs_sorted): the arithmetic shared by the kernels of hfcl_k_pairs_sorted.hip, the host unit and the host build of the tests
// (tests/pairs_sorted_harness).  The list is the one of hfcl_pairs.hpp, byte for byte; only the way to it differs.  Builds with hipcc and
// with g++.
//
// The method.  Per (configuration, object) a key: the box's grown min along the sweep axis, rounded DOWN to fp32 and mapped to a uint32
// whose order is the floats' (psort_key).  The keys of a chunk of whole configurations are sorted, the configuration's index in the chunk
// above the key.  Sorted position p of a configuration pairs with the positions q > p whose key is at most p's grown max, rounded down the
// same way (psort_end): a window [p + 1, end(p)) found by binary search.  Every pair whose boxes touch on the axis is inside the window of
// its earlier position: key(q) <= min(q) <= max(p), and key(q) is an fp32 number, so key(q) <= the largest fp32 number below max(p).  The
// exact test on the doubles (cull_boxes_touch) decides, the sweep only skips what that test would reject on the axis.
// A NaN follows the predicate, which keeps a pair unless a comparison separates it: a NaN min sorts first (nothing before it can skip
// it), a NaN max has the whole configuration as its window.  -0.0 and +0.0 are one key (the +0.0 one).
// The hits leave as 64-bit words (configuration in the chunk, min(i, j), max(i, j)) in the order the sweep meets them and are sorted
// once more: c, then i, then j ascending -- the list's order.
// Worst case: boxes that all overlap on the sweep axis (a stack of plates swept along their normal's plane) have whole configurations as
// windows -- the all-pairs test again, with two sorts on top.
#pragma once
#include "hfcl_pairs.hpp"

namespace hfcl {

// rows of the sweep: as the tiled form, a wave holds PAIRS_WAVE_ROWS consecutive sorted positions, a workgroup of four waves PAIRS_ROWS;
// the columns of their joint window come through LDS in tiles of PAIRS_TILE
constexpr uint32_t PSORT_AXIS_AUTO = 3u;
// objects a workgroup of the centre-spread kernel reads (automatic axis)
constexpr uint32_t PSORT_SPREAD_BLOCK = 4096u;

// ---- keys ------------------------------------------------------------------------------------------------------------------------
HFCL_HD uint32_t psort_float_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, sizeof(u));
  return u;
}
HFCL_HD float psort_bits_float(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, sizeof(f));
  return f;
}
// the largest fp32 number <= x (x not a NaN): +-inf stay, x > FLT_MAX gives FLT_MAX, x < -FLT_MAX gives -inf; a zero result is +0.0
HFCL_HD float psort_round_down(double x) {
  float f = float(x);  // to nearest
  if (double(f) > x) {  // one step down: the float below f
    const uint32_t u = psort_float_bits(f);
    f = psort_bits_float((u << 1) == 0u ? 0x80000001u : ((u >> 31) ? u + 1u : u - 1u));
  }
  return f == 0.0f ? 0.0f : f;  // (-0.0 == 0.0f: one zero)
}
// uint32 in the order of the floats (no NaN comes here): negative numbers with all bits flipped, the others with the sign bit set
HFCL_HD uint32_t psort_orderable(float f) {
  const uint32_t u = psort_float_bits(f);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
HFCL_HD float psort_orderable_inverse(uint32_t k) { return psort_bits_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }
constexpr uint32_t PSORT_KEY_NEG_INF = 0x007FFFFFu, PSORT_KEY_POS_INF = 0xFF800000u;
// the sort key of a box whose grown min on the sweep axis is `lo`: never above lo; a NaN: -inf
HFCL_HD uint32_t psort_key(double lo) { return lo != lo ? PSORT_KEY_NEG_INF : psort_orderable(psort_round_down(lo)); }
// the last key inside the window of a box whose grown max on the sweep axis is `hi`: the keys k with float(k) <= hi are those <= this; a NaN: +inf
HFCL_HD uint32_t psort_end(double hi) { return hi != hi ? PSORT_KEY_POS_INF : psort_orderable(psort_round_down(hi)); }
// bits an index below `count` needs (count <= 1: 0)
HFCL_HD uint32_t psort_bits(uint64_t count) {
  uint32_t b = 0;
  while (b < 64u && (count - (count ? 1u : 0u)) >> b) ++b;
  return b;
}
// the word a chunk's keys are sorted by: the configuration's index in the chunk above the key
HFCL_HD uint64_t psort_word(uint32_t c_local, uint32_t key) { return (uint64_t(c_local) << 32) | key; }

// ---- windows -----------------------------------------------------------------------------------------------------------------------
// upper_bound of `end_key` in the low words of the sorted keys[0, n) of one configuration: the number of keys <= end_key
HFCL_HD uint32_t psort_upper_bound(const uint64_t* keys, uint32_t n, uint32_t end_key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (uint32_t(keys[mid]) <= end_key) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// ---- the emitted words -----------------------------------------------------------------------------------------------------------
// (c_local, min(i, j), max(i, j)) with obj_bits = psort_bits(n_objects) bits an index: ascending words are the list's order
HFCL_HD uint64_t psort_pair_word(uint32_t c_local, uint32_t a, uint32_t b, uint32_t obj_bits) {
  const uint32_t i = a < b ? a : b, j = a < b ? b : a;
  return (((uint64_t(c_local) << obj_bits) | i) << obj_bits) | j;
}
HFCL_HD void psort_pair_of(uint64_t word, uint32_t obj_bits, uint32_t& i, uint32_t& j) {
  const uint64_t mask = (uint64_t(1) << obj_bits) - 1u;
  j = uint32_t(word & mask);
  i = uint32_t((word >> obj_bits) & mask);
}
// may (a, b) pair under the groups?  The rule of the list is about i < j: collides[group[i]] against group[j]
HFCL_HD bool psort_allowed(uint32_t a, uint32_t group_a, uint32_t b, uint32_t group_b, const uint64_t* collides) {
  return a < b ? pairs_allowed(collides[group_a & 63u], group_b) : pairs_allowed(collides[group_b & 63u], group_a);
}

// ---- the axis ----------------------------------------------------------------------------------------------------------------------
// a box's centre on axis k for the spread of an automatic axis; boxes without a finite centre there (unbounded, NaN) do not count
HFCL_HD bool psort_centre(const double* box, int k, double& centre) {
  centre = 0.5 * box[k] + 0.5 * box[3 + k];
  return centre - centre == 0.0;  // finite
}
// the axis on which the centres spread widest (lo > hi on an axis: no finite centre, spread 0); ties to the lowest axis
HFCL_HD uint32_t psort_pick_axis(const double* lo, const double* hi) {
  uint32_t axis = 0;
  double best = -1.0;
  for (uint32_t k = 0; k < 3u; ++k) {
    const double spread = lo[k] <= hi[k] ? hi[k] - lo[k] : 0.0;
    if (spread > best) {
      best = spread;
      axis = k;
    }
  }
  return axis;
}

}  // namespace hfcl
