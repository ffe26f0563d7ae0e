// hfcl_octree.hpp -- OcTree x convex solid collide() (hppfcl_amd_octree.h): the arithmetic shared by the kernels of
// hfcl_k_octree.hip, the host unit (hfcl_host_octree.hip) and the host build of the tests (tests/octree_harness).
//   the tree         a flat node array; validator and makeOctree without octomap (host)
//   the boxes        getRootBV (include/hpp/fcl/octree.h:139-144), computeChildBV (:299-324): carried down the path, halving by halving
//   the box test     convertBV<AABB, OBB> (BV/BV.h:79-84) of the node's box under the tree's pose and of the solid's local box under the
//                    solid's pose, OBB::overlap(other, request, sqr) (src/BV/OBB.cpp:405-423) = obb_disjoint_lb (hfcl_bvh.hpp)
//   the walk         OcTreeShapeIntersectRecurse (internal/traversal_node_octree.h:299-369)
//   a leaf           constructBox (src/shape/geometric_shapes_utility.cpp:1052-1056), ShapeShapeDistance<Box, S>: the per-pair solver of
//                    hfcl_pair.hpp with the supports of hfcl_shapes.hpp (what a Box x solid pair of a batch runs)
//   the fold         ShapeShapeCollider::run (internal/shape_shape_func.h:132-164), the contact rebuilt by the walk (:337-349),
//                    updateDistanceLowerBoundFromBV / FromLeaf (collision_data.h:1177-1197)
// Every unit that includes this is built without contraction of a*b+c: device and host builds compute the same bits.
// Builds with hipcc and with g++.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/hppfcl_amd_octree.h"
#include "hfcl_bvh.hpp"
#include "hfcl_pair.hpp"
#include "hfcl_listed.hpp"

namespace hfcl {

constexpr int OCT_MAX_DEPTH = int(HFCL_OCTREE_MAX_DEPTH);
constexpr int OCT_STACK = OCT_MAX_DEPTH;  // walk stack entries: the inner nodes of a path, levels 0 .. depth - 1

// ---- the tree (host) ----------------------------------------------------------------------------------------------------
// HFCL_OK, or HFCL_ERR_INVALID_ARGUMENT with the rule that failed in *why
inline int oct_validate(const hfcl_octree_node* nodes, size_t n_nodes, uint32_t depth, std::string* why) {
  auto fail = [&](const std::string& s) {
    if (why) *why = s;
    return int(HFCL_ERR_INVALID_ARGUMENT);
  };
  if (depth < 1 || depth > HFCL_OCTREE_MAX_DEPTH) return fail("depth outside 1..16");
  if (n_nodes == 0) return HFCL_OK;  // the empty tree
  if (!nodes) return fail("null node array");
  if (n_nodes > 0x7FFFFFF0u) return fail("too many nodes (node ids are 32-bit)");
  std::vector<uint8_t> parents(n_nodes, 0);
  for (size_t i = 0; i < n_nodes; ++i) {
    if (nodes[i].occupancy != nodes[i].occupancy) return fail("NaN occupancy at node " + std::to_string(i));
    for (int k = 0; k < 8; ++k) {
      const uint32_t c = nodes[i].child[k];
      if (c == 0) continue;
      if (c >= n_nodes) return fail("child index outside (0, n_nodes) at node " + std::to_string(i));
      if (parents[c]) return fail("node " + std::to_string(c) + " has more than one parent");
      parents[c] = 1;
    }
  }
  for (size_t i = 1; i < n_nodes; ++i)
    if (!parents[i]) return fail("node " + std::to_string(i) + " has no parent");
  // every node has one parent and the root none: what the root reaches is a tree; a node it does not reach lies on a cycle
  std::vector<uint32_t> order(1, 0u);
  std::vector<uint8_t> level(n_nodes, 0);
  order.reserve(n_nodes);
  for (size_t at = 0; at < order.size(); ++at) {  // (a node enters the list once: one parent)
    const uint32_t i = order[at];
    for (int k = 0; k < 8; ++k) {
      const uint32_t c = nodes[i].child[k];
      if (c == 0) continue;
      if (uint32_t(level[i]) + 1u > depth) return fail("node " + std::to_string(c) + " lies deeper than depth");
      level[c] = uint8_t(level[i] + 1u);
      order.push_back(c);
    }
  }
  if (order.size() != n_nodes) return fail("a node is not reachable from the root (a cycle)");
  return HFCL_OK;
}

// occupancy of a leaf hit `hits` times: 0.7, raised in log-odds by every further hit, clamped at 0.97 (octomap's defaults as
// remembered; not checked against octomap)
inline double oct_hit_occupancy(uint64_t hits) {
  if (hits <= 1) return 0.7;
  double odds = 0.7 / 0.3;
  for (uint64_t k = 1; k < hits && k < 8; ++k) odds *= 0.7 / 0.3;  // (five hits are past the clamp already)
  const double p = odds / (1.0 + odds);
  return p < 0.97 ? p : 0.97;
}
struct OctBuilder {
  const uint64_t* codes;  // sorted path codes of the distinct keys: 3 bits a level, the root's child in the highest
  const uint32_t* hits;
  uint32_t depth;
  std::vector<hfcl_octree_node>* out;
  double rec(size_t lo, size_t hi, uint32_t level) {  // the node of the keys [lo, hi) at `level`; at most 17 levels
    const size_t id = out->size();
    out->push_back(hfcl_octree_node());
    for (int k = 0; k < 8; ++k) (*out)[id].child[k] = 0;
    double occ;
    if (level == depth) {
      occ = oct_hit_occupancy(hits[lo]);
    } else {
      occ = 0.0;
      const uint32_t shift = 3u * (depth - 1u - level);
      for (size_t a = lo; a < hi;) {
        const uint32_t ci = uint32_t((codes[a] >> shift) & 7u);
        size_t b = a + 1;
        while (b < hi && uint32_t((codes[b] >> shift) & 7u) == ci) ++b;
        (*out)[id].child[ci] = uint32_t(out->size());
        occ = std::max(occ, rec(a, b, level + 1u));
        a = b;
      }
    }
    (*out)[id].occupancy = occ;
    return occ;
  }
};
inline int oct_from_points(const double* xyz, size_t n, double resolution, uint32_t depth, std::vector<hfcl_octree_node>& out, std::string* why) {
  out.clear();
  if (depth < 1 || depth > HFCL_OCTREE_MAX_DEPTH || !(resolution > 0.0) || !std::isfinite(resolution) || (n && !xyz)) {
    if (why) *why = "depth outside 1..16, a resolution that is not positive and finite, or null points";
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  const double half = double(1u << (depth - 1u)), side = double(1u << depth);
  std::vector<uint64_t> codes;
  codes.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    uint32_t key[3];
    bool inside = true;
    for (int k = 0; k < 3; ++k) {
      const double kd = std::floor(xyz[3 * i + k] / resolution) + half;
      if (!(kd >= 0.0 && kd < side)) inside = false;  // (NaN too)
      else key[k] = uint32_t(kd);
    }
    if (!inside) continue;
    uint64_t code = 0;
    for (uint32_t l = 0; l < depth; ++l) {
      const uint32_t bit = depth - 1u - l;
      code = (code << 3) | uint64_t(((key[0] >> bit) & 1u) | (((key[1] >> bit) & 1u) << 1) | (((key[2] >> bit) & 1u) << 2));
    }
    codes.push_back(code);
  }
  if (codes.empty()) return HFCL_OK;  // the empty tree
  std::sort(codes.begin(), codes.end());
  std::vector<uint64_t> distinct;
  std::vector<uint32_t> hits;
  for (size_t i = 0; i < codes.size(); ++i) {
    if (i && codes[i] == codes[i - 1]) {
      if (hits.back() < 0xFFFFFFFFu) ++hits.back();
    } else {
      distinct.push_back(codes[i]);
      hits.push_back(1u);
    }
  }
  OctBuilder b;
  b.codes = distinct.data();
  b.hits = hits.data();
  b.depth = depth;
  b.out = &out;
  b.rec(0, distinct.size(), 0u);
  return HFCL_OK;
}

HFCL_HD bool oct_kind_supported(int k) {
  return k == K_BOX || k == K_SPHERE || k == K_CAPSULE || k == K_CONE || k == K_CYLINDER || k == K_ELLIPSOID || k == K_CONVEX;
}
// getRootBV: (1 << depth) * resolution / 2
HFCL_HD double oct_root_half(uint32_t depth, double resolution) { return double(1u << depth) * resolution / 2.0; }

// an octree registered on a library: where its nodes start in the library's array
struct DOctree {
  uint64_t node_off;
  uint32_t n_nodes, depth;
  double resolution, root_half;
  double occupancy_threshold, free_threshold;
};

// ---- the box test ----------------------------------------------------------------------------------------------------------
// the solid's OBB against the tree's pose: R = axes^T axes2 is the same for every node of a query (axes = the tree pose's rotation)
template <typename T>
struct OctQuery {
  M3<T> R;
  V3<T> To2, ext2;
};
// lb: the solid's local box (min xyz, max xyz)
template <typename T>
HFCL_HD OctQuery<T> oct_make_query(const Pose<T>& tft, const Pose<T>& tfs, const double* lb) {
  OctQuery<T> o;
  const V3<T> lo = mk<T>(T(lb[0]), T(lb[1]), T(lb[2])), hi = mk<T>(T(lb[3]), T(lb[4]), T(lb[5]));
  o.To2 = mul(tfs.R, (lo + hi) * T(0.5)) + tfs.t;
  o.ext2 = (hi - lo) * T(0.5);
  o.R = tmul(tft.R, tfs.R);
  return o;
}
// true: the node's box [lo, hi] under the tree's pose is disjoint from the solid's OBB, sq = the squared bound that said so
template <typename T>
HFCL_HD bool oct_node_disjoint(const OctQuery<T>& o, const Pose<T>& tft, const V3<T>& lo, const V3<T>& hi, T margin, T bd2, T& sq) {
  const V3<T> To1 = mul(tft.R, (lo + hi) * T(0.5)) + tft.t;
  const V3<T> ext1 = (hi - lo) * T(0.5);
  const V3<T> Tv = tmul(tft.R, o.To2 - To1);
  return obb_disjoint_lb(o.R, Tv, ext1, o.ext2, margin, bd2, sq);
}
// computeChildBV
template <typename T>
HFCL_HD void oct_child_box(const V3<T>& lo, const V3<T>& hi, uint32_t i, V3<T>& clo, V3<T>& chi) {
  clo = lo;
  chi = hi;
  if (i & 1u) clo.x = (lo.x + hi.x) * T(0.5); else chi.x = (lo.x + hi.x) * T(0.5);
  if (i & 2u) clo.y = (lo.y + hi.y) * T(0.5); else chi.y = (lo.y + hi.y) * T(0.5);
  if (i & 4u) clo.z = (lo.z + hi.z) * T(0.5); else chi.z = (lo.z + hi.z) * T(0.5);
}

// ---- the walk --------------------------------------------------------------------------------------------------------------
// OcTreeShapeIntersectRecurse flattened.  The box tests do not depend on the leaves, so the set and order of the reached leaves is
// fixed by the poses; on_leaf(node, lo, hi, m) gets the leaf's own box and the running minimum m of the box bounds met so far (a
// bound is a square root, >= 0, so the `<= 0` latch of updateDistanceLowerBoundFromBV never changes what the minimum takes).
// Returns the minimum over all boxes (DBL_MAX: none was disjoint); overflow: the stack was too small (cannot happen with a
// validated tree).  st_node / st_next[l * stride], st_box[(6 * l + k) * stride]: OCT_STACK levels.
template <typename T, class OnLeaf>
HFCL_HD T oct_walk(const hfcl_octree_node* nodes, const DOctree& tr, const Pose<T>& tft, const OctQuery<T>& oq, T margin, T bd2, uint32_t* st_node,
                   uint32_t* st_next, T* st_box, int stride, OnLeaf on_leaf, bool& overflow) {
  T m = Lim<T>::max();
  overflow = false;
  if (tr.n_nodes == 0) return m;  // `if (!root1) return false`
  int sp = 0;
  // true: an occupied inner node whose box overlaps -- its children are visited
  auto visit = [&](uint32_t node, const V3<T>& lo, const V3<T>& hi) {
    const double occ = nodes[node].occupancy;
    if (occ <= tr.free_threshold) return false;            // isNodeFree
    if (!(occ >= tr.occupancy_threshold)) return false;    // isNodeUncertain
    T sq;
    if (oct_node_disjoint(oq, tft, lo, hi, margin, bd2, sq)) {
      const T nd = hsqrt(sq);
      if (nd < m) m = nd;
      return false;
    }
    uint32_t any = 0;
    for (int k = 0; k < 8; ++k) any |= nodes[node].child[k];
    if (!any) {
      on_leaf(node, lo, hi, m);
      return false;
    }
    return true;
  };
  auto push = [&](uint32_t node, const V3<T>& lo, const V3<T>& hi) {
    st_node[sp * stride] = node;
    st_next[sp * stride] = 0u;
    T* b = st_box + size_t(6 * sp) * size_t(stride);
    b[0] = lo.x; b[stride] = lo.y; b[2 * stride] = lo.z;
    b[3 * stride] = hi.x; b[4 * stride] = hi.y; b[5 * stride] = hi.z;
    ++sp;
  };
  {
    const T d = T(tr.root_half);
    const V3<T> lo = mk<T>(-d, -d, -d), hi = mk<T>(d, d, d);
    if (visit(0u, lo, hi)) push(0u, lo, hi);
  }
  const uint64_t max_steps = 2u * uint64_t(tr.n_nodes) + 2u;  // (a node is visited once and popped once)
  for (uint64_t steps = 0; sp > 0 && steps < max_steps; ++steps) {
    const int top = sp - 1;
    const uint32_t node = st_node[top * stride];
    uint32_t i = st_next[top * stride];
    while (i < 8u && nodes[node].child[i] == 0u) ++i;
    if (i >= 8u) {
      --sp;
      continue;
    }
    st_next[top * stride] = i + 1u;
    const uint32_t child = nodes[node].child[i];
    if (child >= tr.n_nodes) continue;  // (refused by the validator)
    const T* b = st_box + size_t(6 * top) * size_t(stride);
    const V3<T> lo = mk<T>(b[0], b[stride], b[2 * stride]), hi = mk<T>(b[3 * stride], b[4 * stride], b[5 * stride]);
    V3<T> clo, chi;
    oct_child_box(lo, hi, i, clo, chi);
    if (visit(child, clo, chi)) {
      if (sp >= OCT_STACK) {
        overflow = true;
        break;
      }
      push(child, clo, chi);
    }
  }
  return m;
}

// ---- a leaf: ShapeShapeDistance<Box, S>(Box(max - min), tf_tree * Transform3f(center), solid, tf_solid) ---------------------------
template <typename T>
struct OctLeafOut {
  T distance;
  V3<T> p1, p2, normal;  // the solver's own
};
// MinkowskiDiff of (box, solid): hfcl_pair.hpp's SerialSupport with the solid's support plugged in
template <typename T, class Solid>
struct BoxSolidSupport {
  DShape<T> box;
  const Solid* solid;  // V3<T> (*solid)(dir): support of the solid in its own frame (NoSweptSphere)
  MDiff<T> md;
  HFCL_HD void operator()(const V3<T>& dir, V3<T>& w, V3<T>& w0) const {
    w0 = prim_support(box, dir);
    const V3<T> d1 = md.identity ? -dir : -tmul(md.oR1, dir);
    V3<T> s1 = (*solid)(d1);
    s1 = md.identity ? s1 : (mul(md.oR1, s1) + md.ot1);
    w = w0 - s1;
  }
};
// q: setup_collide of the request (mode 1, DefaultGuess, gjk.distance_upper_bound = DBL_MAX); verts: the library's vertex array
template <typename T, class Grp, class Solid>
HFCL_HD void oct_leaf(const V3<T>& lo, const V3<T>& hi, const Pose<T>& tft, const DShape<T>& s, const T* verts, const Pose<T>& tfs,
                      const Solid& solid, const QParams<T>& q, EpaScratch<T, EPA_MAX_ITER>* scratch, OctLeafOut<T>& out) {
  DShape<T> box;
  box.kind = K_BOX;
  box.num_points = 0;
  box.vertex_offset = 0;
  box.bvh_index = 0;
  box.p0 = (hi.x - lo.x) / T(2);  // Box(side): halfSide = side / 2
  box.p1 = (hi.y - lo.y) / T(2);
  box.p2 = (hi.z - lo.z) / T(2);
  box.p3 = T(0);
  box.ssr = T(0);
  Pose<T> tfb;
  tfb.R = tft.R;
  tfb.t = mul(tft.R, (lo + hi) * T(0.5)) + tft.t;
  if (pair_class(K_BOX, s.kind) == CLS_CLOSED) {  // Box x Sphere
    out.distance = closed_form_distance(box, tfb, s, tfs, verts, out.p1, out.p2, out.normal);
    return;
  }
  BoxSolidSupport<T, Solid> sup;
  sup.box = box;
  sup.solid = &solid;
  sup.md = make_mdiff(tfb, tfs);
  const V3<T> guess0 = mk<T>(T(1), T(0), T(0));  // DefaultGuess
  const T r0 = T(0), r1 = swept_radius(s);
  Gjk<T, PW0<T>> g;
  gjk_run(g, q.gjk, guess0, r0 + r1, false, sup);  // normalize_support_direction: both ConvexBase only -- a Box is none
  PairOut<T> o;
  EpaSeed<T> seed;
  if (gjk_finish(g, q, tfb, r0, r1, guess0, o, seed)) {
    Grp::sync();
    epa_run<T, Grp, EPA_MAX_ITER>(scratch, seed, q, tfb, r0, r1, sup, o);
    Grp::sync();
  }
  out.distance = o.distance;
  out.p1 = o.p1;
  out.p2 = o.p2;
  out.normal = o.normal;
}

// ---- the replay of one query ----------------------------------------------------------------------------------------------------
// A listed leaf of a query, in walk order: its node, its own box and the minimum of the box bounds met before it
template <typename T>
struct OctItem {
  uint32_t node, query;
  T lo[3], hi[3];
  T box_min;
};
// the contact as the walk rebuilds it: Contact(o1, o2, b1, b2, pos, normal, depth) with pos = (p1 + p2) / 2
template <typename T>
HFCL_HD void oct_rebuilt_points(const OctLeafOut<T>& lf, V3<T>& n1, V3<T>& n2) {
  const V3<T> pos = (lf.p1 + lf.p2) / T(2);
  const V3<T> h = (lf.distance * lf.normal) / T(2);
  n1 = pos - h;
  n2 = pos + h;
}
// The fold of a query's items in order: updateDistanceLowerBoundFromBV (the minimum logged with each leaf, the tail after the last
// one), updateDistanceLowerBoundFromLeaf and the contact decision of every leaf, the stop at num_max_contacts.  on_contact(k, node,
// leaf): contact k was added.  Writes the record (hppfcl_amd_octree.h) and the bound; returns numContacts().  swapped sets bit 23 only.
template <typename T, class OnContact>
HFCL_HD uint32_t oct_fold(const OctItem<T>* items, const OctLeafOut<T>* leaves, uint64_t n_items, T tail_box_min, T margin, T threshold,
                          uint32_t num_max_contacts, bool swapped, OnContact on_contact, hfcl_result* rec, double* dlb_out) {
  const T nanv = Lim<T>::nan();
  T dlb = Lim<T>::max();
  V3<T> np1 = mk<T>(nanv, nanv, nanv), np2 = np1, nn = np1;
  uint32_t nc = 0;
  int first_node = -1;
  OctLeafOut<T> first;
  first.distance = nanv;
  first.p1 = first.p2 = first.normal = np1;
  bool stopped = false;
  for (uint64_t i = 0; i < n_items; ++i) {
    const T box_min = items[i].box_min;
    const uint32_t node = items[i].node;
    const OctLeafOut<T> lf = leaves[i];
    if (!(dlb <= T(0)) && box_min < dlb) dlb = box_min;
    const T dtc = lf.distance - margin;
    if (dtc < dlb) {
      dlb = dtc;
      np1 = lf.p1;
      np2 = lf.p2;
      nn = lf.normal;
    }
    if (dtc <= threshold && nc < num_max_contacts) {
      if (nc == 0) {
        first = lf;
        first_node = int(node);
      }
      on_contact(nc, node, lf);
      ++nc;
    }
    if (nc >= num_max_contacts) {  // isSatisfied()
      stopped = true;
      break;
    }
  }
  if (!stopped && !(dlb <= T(0)) && tail_box_min < dlb) dlb = tail_box_min;
  if (dlb_out) *dlb_out = double(dlb);
  if (rec) {
    V3<T> p1 = np1, p2 = np2;
    if (nc) oct_rebuilt_points(first, p1, p2);
    const V3<T> n = nc ? first.normal : nn;
    rec->distance = double(nc ? first.distance : dlb);
    rec->normal[0] = n.x; rec->normal[1] = n.y; rec->normal[2] = n.z;
    rec->p1[0] = p1.x; rec->p1[1] = p1.y; rec->p1[2] = p1.z;
    rec->p2[0] = p2.x; rec->p2[1] = p2.y; rec->p2[2] = p2.z;
    rec->b1 = first_node;
    rec->b2 = -1;
    rec->status = (uint32_t(EPA_DID_NOT_RUN) << 3) | (nc ? 128u : 0u) | (swapped ? (1u << 23) : 0u);
    rec->num_contacts = int32_t(nc);
  }
  return nc;
}
template <typename T>
HFCL_HD void oct_fill_contact(hfcl_contact& c, uint32_t pair, uint32_t node, const OctLeafOut<T>& lf) {
  c.pair = pair;
  c.b1 = int32_t(node);
  c.b2 = -1;
  c._pad = 0;
  c.penetration_depth = double(lf.distance);
  V3<T> a1, a2;
  oct_rebuilt_points(lf, a1, a2);
  c.normal[0] = lf.normal.x; c.normal[1] = lf.normal.y; c.normal[2] = lf.normal.z;
  c.p1[0] = a1.x; c.p1[1] = a1.y; c.p1[2] = a1.z;
  c.p2[0] = a2.x; c.p2[1] = a2.y; c.p2[2] = a2.z;
}
HFCL_HD void oct_skipped_record(hfcl_result* rec, double* dlb_out, bool swapped) {
  if (rec) {
    rec->distance = 0;
    for (int k = 0; k < 3; ++k) rec->normal[k] = rec->p1[k] = rec->p2[k] = 0;
    rec->b1 = rec->b2 = 0;
    rec->status = 0x80000000u | (swapped ? (1u << 23) : 0u);
    rec->num_contacts = 0;
  }
  if (dlb_out) *dlb_out = Lim<double>::max();
}

// ---- the kernels' parameter block (hfcl_k_octree.hip) ---------------------------------------------------------------------------
// What a chunk of octree queries adds to the pipeline's block (hfcl_listed.hpp; tf_c: the trees' poses)
struct OctArgs : ListedArgs {
  const double* local_boxes;  // 6 doubles a shape of the library
  uint32_t n_trees;
  const DOctree* trees;
  const hfcl_octree_node* nodes;
  const uint32_t* octree;
  OctItem<double>* items;
  OctLeafOut<double>* leaves;
};

}  // namespace hfcl

#if defined(__HIPCC__)
// Launches of one chunk (hfcl_k_octree.hip: launch_listed_count / launch_listed_solve of hfcl_listed.hpp for this kind)
void launch_oct_count(hipStream_t st, const hfcl::OctArgs& a);
void launch_oct_solve(hipStream_t st, const hfcl::OctArgs& a, int max_blocks, bool want_contacts, const char** names, hipEvent_t* e0, hipEvent_t* e1);
#endif
