// hfcl_octree_distance.hpp -- OcTree x convex solid distance() (hppfcl_amd_octree_distance.h): the arithmetic shared by the kernel of
// hfcl_k_octree_distance.hip and the host build of the tests (tests/octree_distance_harness).
//   the entry        OcTreeSolver::OcTreeShapeDistance / ShapeOcTreeDistance (internal/traversal_node_octree.h:216-244)
//   the walk         OcTreeShapeDistanceRecurse (:246-297), flattened onto the collide walk's stack (hfcl_octree.hpp): OCT_STACK levels
//                    holding node, next child and box, plus the eight box distances of the level's children
//   the solid's box  computeBV<AABB, S>(solid, tf_solid) = hf_solid_world_box (hfcl_hfield.hpp): no swept-sphere radius; the Ellipsoid's
//                    R * radii WITHOUT absolute values, as the reference -- a box with min > max, whose distances over-estimate
//   a child's box    computeChildBV = oct_child_box; Converter<AABB, AABB>::convert(child_bv, tf_tree) (BV/BV.h:66-73): centre
//                    R * center + T, half side ||max - min|| * 0.5 on every axis; AABB::distance (src/BV/AABB.cpp:115-133)
//   a leaf           oct_leaf (hfcl_octree.hpp) with the QParams of setup_distance: ShapeShapeDistance<Box, S>, the per-pair distance()
//                    of this library for that box and pose; DistanceResult::update (collision_data.h:1111-1124): a strict
//                    min_distance > distance takes the distance, the solver's own points and normal, and the node
//   the end          DistanceRequest::isSatisfied: min_distance <= 0
// The descent into child i hangs on d < min_distance with the minimum AS IT STANDS at that moment: the answer is the result of the
// ordered walk, not the minimum over all occupied leaves (with the Ellipsoid's box the two differ).
// A choice: n_nodes == 0 (the reference dereferences a null root) answers with the untouched DistanceResult.
// Every unit that includes this is built without contraction of a*b+c; every sum of products is written left to right.
// Builds with hipcc and with g++.
#pragma once
#include "hfcl_hfield.hpp"
#include "hfcl_octree.hpp"

namespace hfcl {

// the walk's stack of one query (in LDS: one per lane group)
template <typename T>
struct OctDistStack {
  uint32_t node[OCT_STACK], next[OCT_STACK];
  T box[OCT_STACK][6];  // the node's own box: min xyz, max xyz
  T d[OCT_STACK][8];    // aabb1.distance(aabb2) of child i (0 where there is none)
};
struct OctDistWalk {
  int sp;
  uint64_t steps, max_steps;  // 2 * n_nodes + 2: a node is entered once and popped once
  bool started, overflow;
};
// DistanceResult
template <typename T>
struct OctDistResult {
  T min_distance;
  V3<T> p1, p2, normal;
  int32_t b1;
  uint32_t visited;  // leaves solved
};
template <typename T>
HFCL_HD void oct_dist_clear(OctDistResult<T>& r) {
  const T nanv = Lim<T>::nan();
  r.min_distance = Lim<T>::max();
  r.p1 = r.p2 = r.normal = mk<T>(nanv, nanv, nanv);
  r.b1 = -1;
  r.visited = 0;
}
template <typename T>
HFCL_HD void oct_dist_update(OctDistResult<T>& r, uint32_t node, const OctLeafOut<T>& lf) {
  ++r.visited;
  if (r.min_distance > lf.distance) {
    r.min_distance = lf.distance;
    r.p1 = lf.p1;
    r.p2 = lf.p2;
    r.normal = lf.normal;
    r.b1 = int32_t(node);
  }
}
// the record: GJK / EPA fields as the octree collide records write them (0 and EPA_DID_NOT_RUN), bit 7 = min_distance <= 0
template <typename T>
HFCL_HD void oct_dist_record(const OctDistResult<T>& r, bool swapped, hfcl_result* rec) {
  rec->distance = double(r.min_distance);
  rec->normal[0] = r.normal.x; rec->normal[1] = r.normal.y; rec->normal[2] = r.normal.z;
  rec->p1[0] = r.p1.x; rec->p1[1] = r.p1.y; rec->p1[2] = r.p1.z;
  rec->p2[0] = r.p2.x; rec->p2[1] = r.p2.y; rec->p2[2] = r.p2.z;
  rec->b1 = r.b1;
  rec->b2 = -1;
  rec->status = (uint32_t(EPA_DID_NOT_RUN) << 3) | (r.min_distance <= T(0) ? 128u : 0u) | (swapped ? (1u << 23) : 0u);
  rec->num_contacts = 0;
}

// Converter<AABB, AABB>::convert(child_bv, tf_tree), then aabb1.distance(aabb2)
template <typename T>
HFCL_HD T oct_child_box_distance(const Pose<T>& tft, const V3<T>& clo, const V3<T>& chi, const V3<T>& blo, const V3<T>& bhi) {
  const V3<T> c2 = mul(tft.R, (clo + chi) * T(0.5)) + tft.t;
  const T r = norm(chi - clo) * T(0.5);
  const T amin[3] = {c2.x - r, c2.y - r, c2.z - r}, amax[3] = {c2.x + r, c2.y + r, c2.z + r};
  const T bmin[3] = {blo.x, blo.y, blo.z}, bmax[3] = {bhi.x, bhi.y, bhi.z};
  T result = T(0);
  for (int k = 0; k < 3; ++k) {
    if (amin[k] > bmax[k]) {
      const T delta = bmax[k] - amin[k];
      result += delta * delta;
    } else if (bmin[k] > amax[k]) {
      const T delta = amax[k] - bmin[k];
      result += delta * delta;
    }
  }
  return hsqrt(result);
}

HFCL_HD void oct_dist_walk_init(OctDistWalk& w, const DOctree& tr) {
  w.sp = 0;
  w.steps = 0;
  w.max_steps = 2u * uint64_t(tr.n_nodes) + 2u;
  w.started = false;
  w.overflow = false;
}

// Advances the walk to the next leaf to solve (true: its node and box) or to its end (false).  min_distance: the minimum as it stands.
// Run by every lane of the group with the same arguments: lane 0 writes the stack, lanes 0..7 the eight box distances of a node that is
// pushed (they do not depend on the minimum; their comparisons, taken serially in index order, do).
template <typename T, class Grp>
HFCL_HD bool oct_dist_next(const hfcl_octree_node* nodes, const DOctree& tr, const Pose<T>& tft, const V3<T>& blo, const V3<T>& bhi, T min_distance,
                           OctDistStack<T>* st, OctDistWalk& w, uint32_t& leaf, V3<T>& llo, V3<T>& lhi) {
  const int lig = Grp::lane();
  // true: an occupied leaf -- to be solved; else the node ended its branch or its children are on the stack
  auto enter = [&](uint32_t node, const V3<T>& lo, const V3<T>& hi) {
    uint32_t any = 0;
    for (int k = 0; k < 8; ++k) any |= nodes[node].child[k];
    const bool occupied = nodes[node].occupancy >= tr.occupancy_threshold;  // isNodeOccupied: free and uncertain are the same here
    if (!any) {
      if (!occupied) return false;
      leaf = node;
      llo = lo;
      lhi = hi;
      return true;
    }
    if (!occupied) return false;
    if (w.sp >= OCT_STACK) {  // (cannot happen with a validated tree)
      w.overflow = true;
      return false;
    }
    const int at = w.sp;
    Grp::sync();
    if (lig == 0) {
      st->node[at] = node;
      st->next[at] = 0u;
      st->box[at][0] = lo.x; st->box[at][1] = lo.y; st->box[at][2] = lo.z;
      st->box[at][3] = hi.x; st->box[at][4] = hi.y; st->box[at][5] = hi.z;
    }
    for (int k = lig; k < 8; k += Grp::W) {  // (a 16-lane group: lanes 0..7, one child each)
      T d = T(0);
      if (nodes[node].child[k] != 0u) {
        V3<T> clo, chi;
        oct_child_box(lo, hi, uint32_t(k), clo, chi);
        d = oct_child_box_distance(tft, clo, chi, blo, bhi);
      }
      st->d[at][k] = d;
    }
    ++w.sp;
    Grp::sync();
    return false;
  };
  if (!w.started) {
    w.started = true;
    if (tr.n_nodes == 0) return false;  // the empty tree (a choice: the reference dereferences a null root)
    const T d = T(tr.root_half);
    if (enter(0u, mk<T>(-d, -d, -d), mk<T>(d, d, d))) return true;  // the root gets no box test
  }
  while (w.sp > 0 && w.steps < w.max_steps) {  // (bound: 2 * n_nodes + 2 steps over the whole walk)
    ++w.steps;
    const int top = w.sp - 1;
    const uint32_t node = st->node[top];
    uint32_t i = st->next[top];
    while (i < 8u && nodes[node].child[i] == 0u) ++i;  // (bound: 8)
    if (i >= 8u) {
      --w.sp;
      continue;
    }
    if (lig == 0) st->next[top] = i + 1u;
    Grp::sync();
    const uint32_t child = nodes[node].child[i];
    if (child >= tr.n_nodes) continue;               // (refused by the validator)
    if (!(st->d[top][i] < min_distance)) continue;  // `if (d < dresult->min_distance)`
    const V3<T> lo = mk<T>(st->box[top][0], st->box[top][1], st->box[top][2]), hi = mk<T>(st->box[top][3], st->box[top][4], st->box[top][5]);
    V3<T> clo, chi;
    oct_child_box(lo, hi, i, clo, chi);
    if (enter(child, clo, chi)) return true;
  }
  return false;
}

// One query: "advance the walk to the next leaf to solve, or to its end; then solve".  q: setup_distance of the request (DefaultGuess).
// The groups of a wave meet at the solve.  r is the same on every lane of the group.
template <typename T, class Grp, class Solid>
HFCL_HD void oct_distance_query(const hfcl_octree_node* nodes, const DOctree& tr, const Pose<T>& tft, const DShape<T>& s, const T* verts,
                                const Pose<T>& tfs, const Solid& solid, const QParams<T>& q, OctDistStack<T>* st,
                                EpaScratch<T, EPA_MAX_ITER>* scratch, OctDistResult<T>& r, bool& overflow) {
  oct_dist_clear(r);
  V3<T> blo, bhi;
  hf_solid_world_box(s, verts, tfs, blo, bhi);  // aabb2, once per query (a hull: its vertex count)
  OctDistWalk w;
  oct_dist_walk_init(w, tr);
  for (uint32_t pass = 0; pass < tr.n_nodes; ++pass) {  // (bound: a pass solves one leaf, a node is entered once)
    uint32_t leaf = 0;
    V3<T> llo, lhi;
    if (!oct_dist_next<T, Grp>(nodes, tr, tft, blo, bhi, r.min_distance, st, w, leaf, llo, lhi)) break;
    OctLeafOut<T> lf;
    oct_leaf<T, Grp>(llo, lhi, tft, s, verts, tfs, solid, q, scratch, lf);
    oct_dist_update(r, leaf, lf);
    if (r.min_distance <= T(0)) break;  // DistanceRequest::isSatisfied
  }
  overflow = w.overflow;
}

// ---- the kernel's parameter block (hfcl_k_octree_distance.hip): a chunk of m queries of a call -----------------------------------
struct OctDistArgs {
  const DShape<double>* shapes;
  const double* verts;
  uint32_t n_shapes, n_trees;
  const DOctree* trees;
  const hfcl_octree_node* nodes;
  const uint32_t* octree;
  const uint32_t* shape;
  const double* tf_t;
  const double* tf_s;
  const uint8_t* swapped;  // nullptr: none
  uint32_t m;
  QParams<double> q;
  hfcl_result* out;
  uint32_t* n_visited;     // nullptr or m
};

}  // namespace hfcl

#if defined(__HIPCC__)
void launch_oct_distance(hipStream_t st, const hfcl::OctDistArgs& a, int max_blocks);  // k_oct_distance
#endif
