// hfcl_scene.hpp -- scene queries (hfcl_scene_*): the arithmetic shared by the kernels of hfcl_k_scene.hip and the host
// build of the tests (tests/scene_harness): which (configuration, pair) a flat query is, how a chunk of the flat query
// range is cut into fold segments, and the fold of records into a hfcl_scene_summary.  Plain integer / comparison code:
// builds with hipcc and with g++.
#pragma once
#include "hfcl_math.hpp"
#include "../../include/hppfcl_amd.h"

namespace hfcl {

constexpr uint32_t SCENE_NONE = 0xFFFFFFFFu;
// records one wave folds: a configuration's pair list is cut at multiples of this many pairs (4 records per lane).  Measured with 2048: a
// chunk of 262144 records is then 128 waves on 256 CUs and the fold reads at 0.9 TB/s (profiles/r08_a_scene.md)
constexpr uint32_t SCENE_FOLD_SHARE = 256u;

// ---- flat query range: q = c * n_pairs + p ------------------------------------------------------------------------------
HFCL_HD void scene_query(uint64_t q, uint32_t n_pairs, uint64_t& c, uint32_t& p) {
  c = q / n_pairs;
  p = uint32_t(q - c * n_pairs);
}
// ... of query q0 + row, given (c0, p0) = scene_query(q0): one 32-bit division per lane (p0 + row fits 32 bits for every chunk that
// does not span 2^32 pair slots; the 64-bit form otherwise -- the branch is uniform over all but one wave of a launch)
HFCL_HD void scene_query_from(uint64_t c0, uint32_t p0, uint32_t row, uint32_t n_pairs, uint64_t& c, uint32_t& p) {
  const uint64_t pp = uint64_t(p0) + row;
  if (pp <= 0xFFFFFFFFull) {
    const uint32_t k = uint32_t(pp) / n_pairs;
    c = c0 + k;
    p = uint32_t(pp) - k * n_pairs;
  } else {
    const uint64_t k = pp / n_pairs;
    c = c0 + k;
    p = uint32_t(pp - k * n_pairs);
  }
}
// first element of object o's pose row in configuration c (width: 12 doubles or 7 floats)
HFCL_HD uint64_t scene_pose_row(uint64_t c, uint64_t n_objects, uint32_t o, uint32_t width) { return (c * n_objects + o) * width; }

// ---- fold segments of a chunk [q0, q1) -----------------------------------------------------------------------------------
// A configuration's pair list is cut into `shares` = ceil(n_pairs / SCENE_FOLD_SHARE) pieces at fixed pair indices, whatever the
// chunk: piece g = c * shares + k holds the pairs [k * SHARE, min((k + 1) * SHARE, n_pairs)) of configuration c.  A chunk touches
// the pieces [scene_piece_of(q0), scene_piece_of(q1 - 1)] and folds, of each, the part inside [q0, q1).
HFCL_HD uint32_t scene_shares(uint32_t n_pairs) { return (n_pairs + SCENE_FOLD_SHARE - 1u) / SCENE_FOLD_SHARE; }
HFCL_HD uint64_t scene_piece_of(uint64_t q, uint32_t n_pairs) {
  uint64_t c;
  uint32_t p;
  scene_query(q, n_pairs, c, p);
  return c * scene_shares(n_pairs) + p / SCENE_FOLD_SHARE;
}
// piece g, cut to the chunk: configuration c, flat queries [lo, hi) (hi <= lo: nothing)
HFCL_HD void scene_piece_range(uint64_t g, uint32_t n_pairs, uint64_t q0, uint64_t q1, uint64_t& c, uint64_t& lo, uint64_t& hi) {
  const uint32_t shares = scene_shares(n_pairs);
  c = g / shares;
  const uint64_t k = g - c * shares;
  const uint64_t p_lo = k * SCENE_FOLD_SHARE;
  const uint64_t p_hi = (p_lo + SCENE_FOLD_SHARE < uint64_t(n_pairs)) ? p_lo + SCENE_FOLD_SHARE : uint64_t(n_pairs);
  lo = c * n_pairs + p_lo;
  hi = c * n_pairs + p_hi;
  if (lo < q0) lo = q0;
  if (hi > q1) hi = q1;
}
// is the first query of configuration c inside the chunk?  (then the chunk starts c's summary, else it continues the stored one)
HFCL_HD bool scene_chunk_starts(uint64_t c, uint32_t n_pairs, uint64_t q0) { return c * n_pairs >= q0; }

// ---- the fold -------------------------------------------------------------------------------------------------------------
HFCL_HD void scene_summary_init(hfcl_scene_summary& s) {
  s.min_distance = __builtin_inf();
  s.min_pair = SCENE_NONE;
  s.first_contact = SCENE_NONE;
  s.n_contacts = 0u;
  s.n_skipped = 0u;
}
// Does (d, p) replace (best, bp)?  Smaller value, then smaller pair index.  A NaN never does (both comparisons are false), and a
// stored value is never NaN, so a NaN neither wins nor poisons.
HFCL_HD bool scene_better(double d, uint32_t p, double best, uint32_t bp) { return d < best || (d == best && p < bp); }
// What a record contributes to min_distance: collide() -- CollisionResult::distance_lower_bound = distance - security_margin;
// distance() -- min_distance itself.  fp32 records: the subtraction in float, the result widened exactly.
HFCL_HD double scene_value(double distance, double margin, bool collide) { return collide ? distance - margin : distance; }
HFCL_HD double scene_value(float distance, float margin, bool collide) { return double(collide ? distance - margin : distance); }
// one record (value as scene_value gives it) of pair p into s
HFCL_HD void scene_fold_record(hfcl_scene_summary& s, double value, uint32_t status, uint32_t p) {
  if (HFCL_STATUS_SKIPPED(status)) {
    ++s.n_skipped;
    return;
  }
  if (scene_better(value, p, s.min_distance, s.min_pair)) {
    s.min_distance = value;
    s.min_pair = p;
  }
  if (HFCL_STATUS_CONTACT(status)) {
    ++s.n_contacts;
    if (p < s.first_contact) s.first_contact = p;
  }
}
// two partial summaries of one configuration (disjoint sets of pairs) into a
HFCL_HD void scene_fold_merge(hfcl_scene_summary& a, const hfcl_scene_summary& b) {
  if (scene_better(b.min_distance, b.min_pair, a.min_distance, a.min_pair)) {
    a.min_distance = b.min_distance;
    a.min_pair = b.min_pair;
  }
  if (b.first_contact < a.first_contact) a.first_contact = b.first_contact;
  a.n_contacts += b.n_contacts;
  a.n_skipped += b.n_skipped;
}

#if defined(__HIPCC__)
// the wave's lanes' partial summaries -> the same summary in every lane
HFCL_D void scene_wave_reduce(hfcl_scene_summary& s) {
  for (int off = 32; off > 0; off >>= 1) {
    hfcl_scene_summary o;
    o.min_distance = __shfl_xor(s.min_distance, off, 64);
    o.min_pair = __shfl_xor(s.min_pair, off, 64);
    o.first_contact = __shfl_xor(s.first_contact, off, 64);
    o.n_contacts = __shfl_xor(s.n_contacts, off, 64);
    o.n_skipped = __shfl_xor(s.n_skipped, off, 64);
    scene_fold_merge(s, o);
  }
}
#endif

}  // namespace hfcl
