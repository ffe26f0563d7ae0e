// hfcl_nearest_self.hpp -- the clearance of a scene per configuration on device-made pairs (hfcl_scene_nearest_self*): the arithmetic
// shared by the kernels of hfcl_k_nearest_self.hip, the host unit and the host build of the tests (tests/nearest_self_harness).  The two
// passes of hfcl_nearest.hpp on the candidates of hfcl_pairs.hpp: every (i, j), i < j, the groups allow; the seed is a pair, the lists
// are lists of pairs in (c, i, j) order, and the two passes' summaries -- ranks in two different lists -- are combined per configuration.
// nearest_box_terms / nearest_bound_terms must be compiled without contraction of a*b+c, as nearest_bound (hfcl_k_nearest_self.hip and
// the tests' harness are).  Builds with hipcc and with g++.
#pragma once
#include "hfcl_nearest.hpp"
#include "hfcl_pairs.hpp"

namespace hfcl {

// ---- the bound in per-box parts ----------------------------------------------------------------------------------------------------
// what nearest_bound computes of ONE box: a sweep computes it once per box, when the box is loaded, not once per test
struct NearestBoxTerms {
  double diagonal;  // nearest_diagonal
  double largest;   // the largest |coordinate| (of the finite ones)
  bool finite;      // every coordinate is
};
HFCL_HD NearestBoxTerms nearest_box_terms(const double* a) {
  NearestBoxTerms t;
  t.finite = true;
  t.largest = 0.0;
  for (int k = 0; k < 6; ++k) {
    if (!nearest_finite(a[k])) t.finite = false;
    const double x = habs(a[k]);
    if (x > t.largest) t.largest = x;
  }
  t.diagonal = nearest_diagonal(a);
  return t;
}
// the bits of nearest_bound(a, b, r) for every input: max is exact and order-free, e is the same sum of the same two square roots
HFCL_HD double nearest_bound_terms(const double* a, const NearestBoxTerms& ta, const double* b, const NearestBoxTerms& tb, double r) {
  const double none = -__builtin_inf();
  if (!ta.finite || !tb.finite) return none;
  const double M = ta.largest > tb.largest ? ta.largest : tb.largest;
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
  const double e = ta.diagonal + tb.diagonal;
  const double L = lb - (NEAREST_INFLATION_SLACK * e + r * M);
  return nearest_finite(L) ? L : none;
}
// two doubles a box where the terms are staged: `finite` rides in the sign of the second (a largest |coordinate| is never negative)
HFCL_HD double nself_pack_largest(const NearestBoxTerms& t) { return t.finite ? t.largest : -1.0; }
HFCL_HD NearestBoxTerms nself_unpack(double diagonal, double packed) {
  NearestBoxTerms t;
  t.diagonal = diagonal;
  t.largest = packed;
  t.finite = packed >= 0.0;
  return t;
}

// ---- the selection -------------------------------------------------------------------------------------------------------------------
// a pair as one word: the order of the words is the lexicographic order of the pairs
constexpr uint64_t NSELF_NO_PAIR = ~uint64_t(0);
HFCL_HD uint64_t nself_key(uint32_t i, uint32_t j) { return (uint64_t(i) << 32) | j; }
// the smallest L of a row of the table and the lowest column attaining it (L = +inf, j = SCENE_NONE: a row without a candidate)
struct NselfRowSeed {
  double L;
  uint32_t j;
  uint32_t pad;
};
static_assert(sizeof(NselfRowSeed) == 16, "a 16-byte partial per row");
// the smallest L so far and the lowest pair attaining it
struct NselfSeed {
  double L;
  uint64_t key;
};
HFCL_HD void nself_seed_init(NselfSeed& s) {
  s.L = __builtin_inf();
  s.key = NSELF_NO_PAIR;
}
HFCL_HD void nself_seed_merge(NselfSeed& s, double L, uint64_t key) {
  if (L < s.L || (L == s.L && key < s.key)) {
    s.L = L;
    s.key = key;
  }
}
// pass 1 / pass 2 of hfcl_nearest.hpp with the pair's word in the place of its index in a list
HFCL_HD bool nself_in_pass1(double L, uint64_t key, uint64_t seed, double D) { return (L == -__builtin_inf() || key == seed) && L <= D; }
HFCL_HD bool nself_in_pass(int pass, double L, uint64_t key, uint64_t seed, double D, double thr) {
  const bool first = nself_in_pass1(L, key, seed, D);
  return pass == 1 ? first : (!first && L <= thr);
}

// ---- the two passes' summaries into one clearance -----------------------------------------------------------------------------------------
// Configuration c: sum[l] the summaries of pass l + 1 (min_pair: a rank in the configuration's span of list l), pairs[l] / conf_begin[l]
// that list, rec[l] its records (nullptr: none).  The smaller min_distance, on a tie the lower (i, j); the counts add up.  A null
// conf_begin[l]: an empty list.
template <typename R>
HFCL_HD void nself_combine(uint64_t c, const hfcl_scene_summary* const* sum, const uint32_t* const* pairs, const uint64_t* const* conf_begin,
                           const R* const* rec, hfcl_scene_clearance& out, R* min_out) {
  out.min_distance = __builtin_inf();
  out.min_i = out.min_j = SCENE_NONE;
  out.n_evaluated = 0u;
  out.n_skipped = 0u;
  uint64_t best = NSELF_NO_PAIR, where = 0;
  int from = -1;
  for (int l = 0; l < 2; ++l) {
    if (!conf_begin[l]) continue;
    const uint64_t lo = conf_begin[l][c], hi = conf_begin[l][c + 1u];
    if (hi == lo) continue;
    const hfcl_scene_summary s = sum[l][c];
    out.n_evaluated += uint32_t(hi - lo);
    out.n_skipped += s.n_skipped;
    if (s.min_pair == SCENE_NONE) continue;
    const uint64_t k = lo + s.min_pair;
    const uint64_t key = nself_key(pairs[l][2u * k], pairs[l][2u * k + 1u]);
    if (from < 0 || s.min_distance < out.min_distance || (s.min_distance == out.min_distance && key < best)) {
      out.min_distance = s.min_distance;
      best = key;
      where = k;
      from = l;
    }
  }
  if (from >= 0) {
    out.min_i = uint32_t(best >> 32);
    out.min_j = uint32_t(best);
  }
  if (min_out) {
    if (from >= 0 && rec[from]) {
      *min_out = rec[from][where];
    } else {
      R none = R();
      nearest_no_record(none);
      *min_out = none;
    }
  }
}

}  // namespace hfcl
