// hfcl_nearest_env.hpp -- the clearance of the moving objects of a scene among an environment kept on the device
// (include/hppfcl_amd_nearest_env.h: hfcl_scene_nearest_env*): the arithmetic shared by the kernels of hfcl_k_nearest_env.hip, the host unit
// and the host build of the tests (tests/nearest_env_harness).  The two passes of hfcl_nearest_self.hpp over the cells of hfcl_env.hpp: the
// candidates are the pairs (i, j), i < n_moving, i < j < n_objects, the groups allow; bound, seed, predicate, threshold and combination are
// those of hfcl_nearest_self.hpp.  What is new here: the per-box terms of the bound kept with the environment (set time), per-tile terms,
// and a lower bound of the bound over a whole (row block, environment tile) cell, by which a pass drops the cell without loading it.
// Must be compiled without contraction of a*b+c, as hfcl_nearest_self.hpp (hfcl_k_nearest_env.hip and the tests' harness are).  Builds with
// hipcc and with g++.
#pragma once
#include "hfcl_nearest_self.hpp"
#include "hfcl_env.hpp"

namespace hfcl {

// ---- set-time tables ---------------------------------------------------------------------------------------------------------------
// per environment box two doubles: nearest_box_terms' diagonal, and nself_pack_largest of it -- what a sweep stages beside the box
HFCL_HD void nenv_box_terms(const double* box, double* terms) {
  const NearestBoxTerms t = nearest_box_terms(box);
  terms[0] = t.diagonal;
  terms[1] = nself_pack_largest(t);
}
// per tile two doubles, folded in member order from 0: the largest member diagonal, the largest member `largest`; "wild" -- some member
// coordinate is not finite -- packed as -1 in the second (a diagonal that is a NaN belongs to a wild tile and is never the larger)
HFCL_HD void nenv_tile_terms(const double* env_terms, uint32_t n_env, uint32_t t, double* terms) {
  const uint32_t e0 = t * PAIRS_TILE, e1 = n_env - e0 > PAIRS_TILE ? e0 + PAIRS_TILE : n_env;
  double diagonal = 0.0, largest = 0.0;
  bool wild = false;
  for (uint32_t e = e0; e < e1; ++e) {
    const double d = env_terms[2u * size_t(e)], big = env_terms[2u * size_t(e) + 1u];
    if (d > diagonal) diagonal = d;
    if (big < 0.0) wild = true;
    if (big > largest) largest = big;
  }
  terms[0] = diagonal;
  terms[1] = wild ? -1.0 : largest;
}

// ---- a row block as one box --------------------------------------------------------------------------------------------------------
// Beyond this largest |coordinate| the cell's bound is not computed: below it no step of it -- differences, squares, their sum, the
// diagonals, the slack -- can overflow, so a pair of such boxes that are apart has a finite L
constexpr double NENV_COORD_MAX = 0x1p500;
struct NenvBlock {
  double uni[6];    // the union of the rows' (ungrown) boxes: env_fold_min / env_fold_max in row order
  double diagonal;  // the largest row diagonal
  double largest;   // the largest row `largest`
  bool finite;      // every coordinate of every row is
};
// the block is folded row by row; min, max and "and" do not depend on the order or on a row that comes twice (the sign of a zero aside,
// which no step of the bound sees: a difference of zero is clamped to 0 or squared), so a kernel may fold its waves' rows apart and merge
HFCL_HD void nenv_block_init(NenvBlock& b) {
  for (int k = 0; k < 3; ++k) {
    b.uni[k] = __builtin_inf();
    b.uni[3 + k] = -__builtin_inf();
  }
  b.diagonal = 0.0;
  b.largest = 0.0;
  b.finite = true;
}
// a row: its box and its terms as they are staged (nself_pack_largest: negative = not finite)
HFCL_HD void nenv_block_add(NenvBlock& b, const double* a, double diagonal, double packed_largest) {
  for (int k = 0; k < 3; ++k) {
    b.uni[k] = env_fold_min(b.uni[k], a[k]);
    b.uni[3 + k] = env_fold_max(b.uni[3 + k], a[3 + k]);
  }
  if (packed_largest < 0.0) b.finite = false;
  if (diagonal > b.diagonal) b.diagonal = diagonal;
  if (packed_largest > b.largest) b.largest = packed_largest;
}
// a part of the block as 8 doubles (the union, the diagonal, the largest with "not finite" as -1), and a part into the block
HFCL_HD void nenv_block_pack(const NenvBlock& b, double* w) {
  for (int k = 0; k < 6; ++k) w[k] = b.uni[k];
  w[6] = b.diagonal;
  w[7] = b.finite ? b.largest : -1.0;
}
HFCL_HD void nenv_block_merge(NenvBlock& b, const double* w) { nenv_block_add(b, w, w[6], w[7]); }
// rows [i0, i1) of a configuration's moving boxes
HFCL_HD NenvBlock nenv_block(const double* boxes, uint32_t i0, uint32_t i1) {
  NenvBlock b;
  nenv_block_init(b);
  for (uint32_t i = i0; i < i1; ++i) {
    const double* a = boxes + 6u * size_t(i);
    const NearestBoxTerms t = nearest_box_terms(a);
    nenv_block_add(b, a, t.diagonal, nself_pack_largest(t));
  }
  return b;
}

// ---- the bound of a cell -------------------------------------------------------------------------------------------------------------
// Lt of a row block and an environment tile (its box: env_tile_coord's, its terms: nenv_tile_terms'): -inf when the tile is wild, a row
// coordinate is not finite, the tile's box touches the union (cull_boxes_touch: closed), or the largest |coordinate| of either exceeds
// NENV_COORD_MAX; otherwise the operations of nearest_bound_terms in their order on the union and the tile's box, with the largest
// diagonals and the largest `largest` of the two sides.  The union lies around every row's box and the tile's box around every member's,
// the diagonals and M are not below any pair's, and every operation -- a difference, max, a square, a sum, the square root, a product
// with a positive constant -- is monotone under rounding: Lt <= L(i, j) for every row i of the block and every member j of the tile, and
// a finite Lt means that no such pair has L = -inf (none touches, none is not finite, none overflows).
HFCL_HD double nenv_tile_bound(const NenvBlock& b, const double* tile_box, const double* tile_terms, double r) {
  const double none = -__builtin_inf();
  if (tile_terms[1] < 0.0 || !b.finite) return none;
  if (!(b.largest <= NENV_COORD_MAX) || !(tile_terms[1] <= NENV_COORD_MAX)) return none;
  if (cull_boxes_touch(b.uni, tile_box)) return none;
  const double M = b.largest > tile_terms[1] ? b.largest : tile_terms[1];
  double g[3];
  bool apart = false;
  for (int k = 0; k < 3; ++k) {
    const double g1 = b.uni[k] - tile_box[3 + k], g2 = tile_box[k] - b.uni[3 + k];
    g[k] = g1 > g2 ? g1 : g2;
    if (g[k] > 0.0) apart = true;
    else g[k] = 0.0;
  }
  if (!apart) return none;
  const double lb = hsqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  const double e = b.diagonal + tile_terms[0];
  const double L = lb - (NEAREST_INFLATION_SLACK * e + r * M);
  return nearest_finite(L) ? L : none;
}
// what a sweep does with it.  mode 0 (the seeds): nothing is dropped by distance.  Pass 1 holds the pairs with L = -inf and the seed: a
// cell with a finite Lt holds none of the first, and the seed only if it is (a row of this block, a column of this tile).  Pass 2 holds
// pairs with L <= thr only.
HFCL_HD bool nenv_tile_dropped(int mode, double Lt, uint64_t seed, uint32_t i0, uint32_t i1, uint32_t j0, uint32_t cols, double thr) {
  if (mode == 1) {
    const uint32_t si = uint32_t(seed >> 32), sj = uint32_t(seed);
    const bool seed_here = seed != NSELF_NO_PAIR && si >= i0 && si < i1 && sj >= j0 && sj - j0 < cols;
    return Lt > -__builtin_inf() && !seed_here;
  }
  return mode == 2 && Lt > thr;
}

// ---- the seeds -------------------------------------------------------------------------------------------------------------------------
// the partials of a configuration: one NselfRowSeed per (row, span), row-major; x = i * n_spans + span
HFCL_HD void nenv_seed_fold(NselfSeed& s, const NselfRowSeed* partials, uint32_t n_spans, uint64_t x) {
  const NselfRowSeed o = partials[x];
  if (o.j != SCENE_NONE) nself_seed_merge(s, o.L, nself_key(uint32_t(x / n_spans), o.j));
}

}  // namespace hfcl
