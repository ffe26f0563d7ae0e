// hfcl_nearest.hpp -- the per-configuration minimum distance of a scene with box-bound pruning (hfcl_scene_nearest*): the arithmetic
// shared by the kernels of hfcl_k_nearest.hip and the host build of the tests (tests/nearest_harness).  What
// DynamicAABBTreeCollisionManager::distance with DistanceCallBackDefault does with its shrinking bound, restated on the flat pair list:
// a lower bound L of a query's distance from its two world boxes, a first list (the queries without a bound, and per configuration the
// one with the smallest bound), the threshold its minimum gives, a second list (every other query whose bound is not above the threshold).
// nearest_bound (and nearest_diagonal) must be compiled without contraction of a*b+c for the bounds to be the same bits everywhere:
// hfcl_k_nearest.hip and the tests' harness are.  The host unit uses the constants, NearestSeed and nearest_no_record only.
// Builds with hipcc and with g++.
#pragma once
#include "hfcl_cull.hpp"

namespace hfcl {

// ---- the bound ------------------------------------------------------------------------------------------------------------------
// Box, Cone and Cylinder supports are inflated by 1 + 1e-10 (hfcl_shapes.hpp: box_inflate): a computed distance may fall below the true one
// by 1e-10 x the shapes' half extents.  Four times that, on the sum of the two boxes' diagonals.
constexpr double NEAREST_INFLATION_SLACK = 2e-10;
// rounding of the narrow phase, relative to the largest coordinate of the two boxes.  fp64: 2^-40 (seen: about one ulp).
constexpr double NEAREST_R64 = 0x1p-40;
// fp32 records: 16 x the largest (lb - d_f32) / M measured on the device against the unculled fp32 call, rounded up to a power of two,
// with a floor of 2^-18.  Measured where the bound is tight (tests/test_scene_nearest_gpu.py prints them): 1.03e-7 = 2^-23.2 on 504 axis-aligned
// face-to-face pairs of every solid kind at coordinate offsets 0 .. 4000, 7.5e-9 on the grid of spheres and boxes; negative under random
// rotations (-2.7e-3 .. -7.3e-6 on the planner scenes).  16 x 2^-23.2 rounds up to 2^-19: the floor holds (profiles/r10_a_scene_nearest.md)
constexpr double NEAREST_R32 = 0x1p-18;

HFCL_HD bool nearest_finite(double x) { return habs(x) <= 1.7976931348623157e308; }  // (false for a NaN)
HFCL_HD double nearest_diagonal(const double* a) {
  const double x = a[3] - a[0], y = a[4] - a[1], z = a[5] - a[2];
  return hsqrt((x * x + y * y) + z * z);
}
// L(q) of the world boxes a, b (min xyz, max xyz) of the query's two objects: -inf (no bound: the query is always evaluated) when the boxes
// touch (closed intervals, as cull_boxes_touch), when a coordinate is not finite (NaN poses, the +-DBL_MAX boxes of Plane and Halfspace)
// or when the arithmetic overflows; the distance between the boxes less the slack otherwise
HFCL_HD double nearest_bound(const double* a, const double* b, double r) {
  const double none = -__builtin_inf();
  double M = 0.0;
  for (int k = 0; k < 6; ++k) {
    if (!nearest_finite(a[k]) || !nearest_finite(b[k])) return none;
    const double x = habs(a[k]), y = habs(b[k]);
    if (x > M) M = x;
    if (y > M) M = y;
  }
  double g[3];
  bool apart = false;
  for (int k = 0; k < 3; ++k) {
    const double g1 = a[k] - b[3 + k], g2 = b[k] - a[3 + k];
    g[k] = g1 > g2 ? g1 : g2;
    if (g[k] > 0.0) apart = true;
    else g[k] = 0.0;
  }
  if (!apart) return none;
  const double lb = hsqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  const double e = nearest_diagonal(a) + nearest_diagonal(b);
  const double L = lb - (NEAREST_INFLATION_SLACK * e + r * M);
  return nearest_finite(L) ? L : none;
}

// ---- the selection ----------------------------------------------------------------------------------------------------------------
// seed[c]: the lowest p attaining the smallest L of configuration c
struct NearestSeed {
  double L;
  uint32_t p;
  uint32_t pad;
};
HFCL_HD void nearest_seed_init(NearestSeed& s) {
  s.L = __builtin_inf();
  s.p = SCENE_NONE;
  s.pad = 0u;
}
HFCL_HD void nearest_seed_merge(NearestSeed& s, double L, uint32_t p) {
  if (L < s.L || (L == s.L && p < s.p)) {
    s.L = L;
    s.p = p;
  }
}
// pass 1: the queries without a bound and each configuration's seed, unless the bound is already above the caller's upper bound D
HFCL_HD bool nearest_in_pass1(double L, uint32_t p, uint32_t seed, double D) { return (L == -__builtin_inf() || p == seed) && L <= D; }
// thr[c]: what pass 1 found, capped by D
HFCL_HD double nearest_threshold(double D, double min_distance) { return min_distance < D ? min_distance : D; }
// pass 2: the other queries whose bound is not above the threshold
HFCL_HD bool nearest_in_pass2(double L, uint32_t p, uint32_t seed, double D, double thr) { return !nearest_in_pass1(L, p, seed, D) && L <= thr; }

// the min record of a configuration without an evaluated, computed record: status bit 31, distance = +inf
HFCL_HD void nearest_no_record(hfcl_result& r) {
  const double x = __builtin_nan("");
  r.distance = __builtin_inf();
  for (int k = 0; k < 3; ++k) r.normal[k] = r.p1[k] = r.p2[k] = x;
  r.b1 = r.b2 = -1;
  r.status = 0x80000000u;
  r.num_contacts = 0;
}
HFCL_HD void nearest_no_record(hfcl_result_f32& r) {
  r.distance = __builtin_inff();
  for (int k = 0; k < 3; ++k) r.normal[k] = r.p1[k] = r.p2[k] = 0.0f;
  r.status = 0x80000000u;
}

// position of the id q in the ascending ids[lo, hi), or hi
HFCL_HD uint64_t nearest_find(const uint64_t* ids, uint64_t lo, uint64_t hi, uint64_t q) {
  const uint64_t end = hi;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    if (ids[mid] < q) lo = mid + 1u;
    else hi = mid;
  }
  return (lo < end && ids[lo] == q) ? lo : end;
}

}  // namespace hfcl
