// hfcl_octree_mesh.hpp -- OcTree x BVHModel<OBBRSS> collide() (hppfcl_amd_octree_mesh.h): the arithmetic shared by the kernels of
// hfcl_k_octree_mesh.hip and the host build of the tests (tests/octree_mesh_harness).
//   the boxes        getRootBV, computeChildBV: carried down the path, halving by halving (hfcl_octree.hpp)
//   the box test     convertBV<AABB, OBB> of the node's box under the tree's pose, convertBV<OBBRSS, OBB> (BV/BV.h:94-113) of the mesh node
//                    under the mesh's pose, OBB::overlap(other, request, sqr) (src/BV/OBB.cpp:405-423) = obb_disjoint_lb (hfcl_bvh.hpp)
//   the walk         OcTreeMeshIntersectRecurse (internal/traversal_node_octree.h:462-563) flattened over a PATH stack: a frame per level of
//                    the recursion, an octree frame where the octree side descended, a mesh frame where the mesh side did
//   a leaf           constructBox, ShapeShapeDistance<Box, TriangleP>: triangle_solid_distance (hfcl_bvh_shape.hpp) with the Box as the
//                    solid, its result kept in Box-first order
//   the fold         updateDistanceLowerBoundFromBV / FromLeaf (collision_data.h:1177-1197), the eight-argument Contact (:138-148)
// Every unit that includes this is built without contraction of a*b+c: device and host builds compute the same bits.
// Builds with hipcc and with g++.
#pragma once
#include <utility>

#include "../../include/hppfcl_amd_octree_mesh.h"
#include "hfcl_octree.hpp"
#include "hfcl_bvh_shape.hpp"

namespace hfcl {

constexpr int OCTM_MESH_DEPTH = int(HFCL_OCTREE_MESH_MAX_BVH_DEPTH);  // levels of a mesh's BVH the walk takes (the root is level 1)
constexpr int OCTM_MESH_STACK = OCTM_MESH_DEPTH;  // mesh frames: the inner nodes of a path, at most depth - 1

// Levels of a BVH given as a node array (the root is level 1), by an explicit stack; 0xFFFFFFFF where the child links revisit a node
// (more visits than nodes): such an array is as deep as one likes.  first_child(i): the link of node i (> 0: children at it and the next)
template <class FirstChild>
inline uint32_t octm_bvh_depth(size_t n_nodes, FirstChild first_child) {
  if (n_nodes == 0) return 0;
  std::vector<std::pair<uint32_t, uint32_t>> todo(1, std::make_pair(0u, 1u));
  uint32_t depth = 1;
  size_t visits = 0;
  while (!todo.empty()) {  // (at most n_nodes + 1 passes)
    const std::pair<uint32_t, uint32_t> e = todo.back();
    todo.pop_back();
    if (++visits > n_nodes) return 0xFFFFFFFFu;
    depth = std::max(depth, e.second);
    const int fc = first_child(e.first);
    if (fc > 0 && size_t(fc) + 1 < n_nodes) {
      todo.emplace_back(uint32_t(fc), e.second + 1u);
      todo.emplace_back(uint32_t(fc) + 1u, e.second + 1u);
    }
  }
  return depth;
}

// ---- the walk --------------------------------------------------------------------------------------------------------------
// true: the octree node's box [lo, hi] under the tree's pose is disjoint from the mesh node's OBB under the mesh's pose
template <typename T>
HFCL_HD bool octm_disjoint(const Pose<T>& tft, const V3<T>& lo, const V3<T>& hi, const Pose<T>& tfm, const DNode<T>& bn, T margin, T bd2, T& sq) {
  const V3<T> To1 = mul(tft.R, (lo + hi) * T(0.5)) + tft.t;  // Converter<AABB, OBB>
  const V3<T> ext1 = (hi - lo) * T(0.5);
  const V3<T> To2 = mul(tfm.R, bn.To) + tfm.t;  // Converter<OBBRSS, OBB>
  const M3<T> axes2 = mmul(tfm.R, bn.axes);
  const V3<T> Tv = tmul(tft.R, To2 - To1);  // OBB::overlap: axes^T (other.To - To), axes^T other.axes
  const M3<T> R = tmul(tft.R, axes2);
  return obb_disjoint_lb(R, Tv, ext1, bn.extent, margin, bd2, sq);
}

// OcTreeMeshIntersectRecurse without the leaves' solves.  The box tests do not depend on the leaves, so the set and order of the
// reached (octree leaf, triangle) pairs is fixed by the poses; on_leaf(node, lo, hi, prim, m) gets the leaf's own box, the triangle
// and the running minimum m of the box bounds met so far (a bound is a square root, > 0, so the `<= 0` latch of
// updateDistanceLowerBoundFromBV never changes what the minimum takes).  Returns the minimum over all boxes (DBL_MAX: none was
// disjoint).  overflow: a stack was too small -- the walk ends there; the host refuses meshes deeper than OCTM_MESH_DEPTH before any
// launch and the validator trees deeper than 16, so this is unreachable, and the guard stays.
// The state is the recursion's path.  An octree frame (st_node / st_next [l * stride], st_box[(6 * l + k) * stride]; OCT_STACK
// levels): a node whose children are being visited, the next child index, the node's box.  A mesh frame (st_m / st_mo [l * stride];
// OCTM_MESH_STACK levels): the first child of a mesh node whose children are being visited; st_mo = the number of octree frames
// below it (bits 0-4) and which child comes next (bits 5-6).  The mesh frame on top is the newest frame iff no octree frame was
// pushed since.  The current octree node of a mesh frame is the child the top octree frame went into last (the root: none); the current
// mesh node of an octree frame likewise.  Every pass of the loop is one entry of the recursion; a tree and a BVH of bounded depth end it.
template <typename T, class OnLeaf>
HFCL_HD T octm_walk(const hfcl_octree_node* nodes, const DOctree& tr, const Pose<T>& tft, const DNode<T>* mnodes, uint32_t n_mnodes,
                    const Pose<T>& tfm, T margin, T bd2, uint32_t* st_node, uint32_t* st_next, T* st_box, uint32_t* st_m, uint8_t* st_mo, int stride,
                    OnLeaf on_leaf, bool& overflow) {
  T m = Lim<T>::max();
  overflow = false;
  if (tr.n_nodes == 0 || n_mnodes == 0) return m;  // `if (!root1) return false`
  int osp = 0, msp = 0;
  const T d = T(tr.root_half);
  const V3<T> rlo = mk<T>(-d, -d, -d), rhi = mk<T>(d, d, d);
  uint32_t cur_o = 0u, cur_m = 0u;
  V3<T> lo = rlo, hi = rhi;
  for (;;) {
    // ---- one entry of the recursion: (cur_o with [lo, hi], cur_m)
    int act = 0;  // 1: the octree side descends, 2: the mesh side
    int mfc = 0;
    const double occ = nodes[cur_o].occupancy;
    if (!(occ <= tr.free_threshold) && occ >= tr.occupancy_threshold) {  // neither isNodeFree nor isNodeUncertain
      const DNode<T> bn = mnodes[cur_m];
      T sq;
      if (octm_disjoint(tft, lo, hi, tfm, bn, margin, bd2, sq)) {
        const T nd = hsqrt(sq);
        if (nd < m) m = nd;
      } else {
        uint32_t any = 0;
        for (int k = 0; k < 8; ++k) any |= nodes[cur_o].child[k];
        const bool mleaf = bn.first_child < 0;
        if (!any && mleaf) {
          on_leaf(cur_o, lo, hi, uint32_t(-(bn.first_child + 1)), m);
        } else if (mleaf || (any && sqnorm(hi - lo) > sqnorm(bn.extent))) {  // AABB::size(): the FULL diagonal squared; OBBRSS::size(): the HALF extents squared
          act = 1;
        } else {
          act = 2;
          mfc = bn.first_child;
        }
      }
    }
    if (act == 1) {
      if (osp >= OCT_STACK) {
        overflow = true;
        break;
      }
      st_node[osp * stride] = cur_o;
      st_next[osp * stride] = 0u;
      T* b = st_box + size_t(6 * osp) * size_t(stride);
      b[0] = lo.x; b[stride] = lo.y; b[2 * stride] = lo.z;
      b[3 * stride] = hi.x; b[4 * stride] = hi.y; b[5 * stride] = hi.z;
      ++osp;
    } else if (act == 2) {
      if (msp >= OCTM_MESH_STACK || mfc <= 0) {
        overflow = true;
        break;
      }
      st_m[msp * stride] = uint32_t(mfc);
      st_mo[msp * stride] = uint8_t(osp);
      ++msp;
    }
    // ---- the next entry: the newest frame's next child; a frame without one is dropped
    bool found = false;
    while (osp > 0 || msp > 0) {
      const bool mtop = msp > 0 && int(st_mo[(msp - 1) * stride] & 31u) == osp;
      if (mtop) {
        const uint32_t which = uint32_t(st_mo[(msp - 1) * stride]) >> 5;
        if (which >= 2u) {
          --msp;
          continue;
        }
        st_mo[(msp - 1) * stride] = uint8_t(uint32_t(osp) | ((which + 1u) << 5));
        cur_m = st_m[(msp - 1) * stride] + which;  // left, then right
        if (cur_m >= n_mnodes) continue;  // (refused at registration)
        if (osp == 0) {
          cur_o = 0u;
          lo = rlo;
          hi = rhi;
        } else {
          const int top = osp - 1;
          const uint32_t i = st_next[top * stride] - 1u;  // (a frame under a mesh frame has gone into a child)
          cur_o = nodes[st_node[top * stride]].child[i & 7u];
          const T* b = st_box + size_t(6 * top) * size_t(stride);
          oct_child_box(mk<T>(b[0], b[stride], b[2 * stride]), mk<T>(b[3 * stride], b[4 * stride], b[5 * stride]), i & 7u, lo, hi);
        }
        found = true;
        break;
      }
      const int top = osp - 1;
      const uint32_t node = st_node[top * stride];
      uint32_t i = st_next[top * stride];
      while (i < 8u && nodes[node].child[i] == 0u) ++i;
      if (i >= 8u) {
        --osp;
        continue;
      }
      st_next[top * stride] = i + 1u;
      const uint32_t child = nodes[node].child[i];
      if (child >= tr.n_nodes) continue;  // (refused by the validator)
      const T* b = st_box + size_t(6 * top) * size_t(stride);
      oct_child_box(mk<T>(b[0], b[stride], b[2 * stride]), mk<T>(b[3 * stride], b[4 * stride], b[5 * stride]), i, lo, hi);
      cur_o = child;
      cur_m = 0u;
      if (msp > 0) {
        const uint32_t which = uint32_t(st_mo[(msp - 1) * stride]) >> 5;  // (>= 1: a frame under an octree frame has gone into a child)
        cur_m = st_m[(msp - 1) * stride] + ((which - 1u) & 1u);
      }
      found = true;
      break;
    }
    if (!found) break;
  }
  return m;
}

// ---- a leaf: ShapeShapeDistance<Box, TriangleP>(Box(max - min), tf_tree * Transform3f(center), tri, tf_mesh) -------------------------
template <typename T>
struct OctMeshLeafOut {
  T distance;
  V3<T> p1, p2, normal;  // the solver's own, Box first
  uint32_t prim, pad_;   // the item's triangle (the fold reports it)
};
template <typename T>
struct OctMeshBoxSupport {
  DShape<T> box;
  HFCL_HD V3<T> operator()(const V3<T>& dir) const { return prim_support(box, dir); }
};
// q: setup_collide of the request (mode 1, DefaultGuess, gjk.distance_upper_bound = DBL_MAX); mverts: the mesh's vertices, t3: the
// triangle's three vertex ids
template <typename T, class Grp>
HFCL_HD void octm_leaf(const V3<T>& lo, const V3<T>& hi, const Pose<T>& tft, const T* mverts, const uint32_t* t3, const Pose<T>& tfm,
                       const QParams<T>& q, EpaScratch<T, EPA_MAX_ITER>* scratch, OctMeshLeafOut<T>& out) {
  OctMeshBoxSupport<T> bs;
  bs.box.kind = K_BOX;
  bs.box.num_points = 0;
  bs.box.vertex_offset = 0;
  bs.box.bvh_index = 0;
  bs.box.p0 = (hi.x - lo.x) / T(2);  // Box(side): halfSide = side / 2
  bs.box.p1 = (hi.y - lo.y) / T(2);
  bs.box.p2 = (hi.z - lo.z) / T(2);
  bs.box.p3 = T(0);
  bs.box.ssr = T(0);
  Pose<T> tfb;
  tfb.R = tft.R;
  tfb.t = mul(tft.R, (lo + hi) * T(0.5)) + tft.t;
  auto vtx = [&](uint32_t i) { return mk<T>(mverts[3 * size_t(i)], mverts[3 * size_t(i) + 1], mverts[3 * size_t(i) + 2]); };
  const V3<T> guess0 = mk<T>(T(1), T(0), T(0));  // DefaultGuess
  PairOut<T> o;
  V3<T> p_tri, p_box, n;  // (the exchanged form, which the mesh x solid leaf reports: not used)
  triangle_solid_distance<T, Grp>(vtx(t3[0]), vtx(t3[1]), vtx(t3[2]), tfm, tfb, bs, T(0), q, guess0, scratch, o, p_tri, p_box, n);
  out.distance = o.distance;
  out.p1 = o.p1;
  out.p2 = o.p2;
  out.normal = o.normal;
}

// ---- the replay of one query ----------------------------------------------------------------------------------------------------
// A listed (octree leaf, triangle) pair of a query, in walk order: the node, its own box, the triangle and the minimum of the box
// bounds met before it
template <typename T>
struct OctMeshItem {
  uint32_t node, query, prim, pad_;
  T lo[3], hi[3];
  T box_min;
};
// The fold of a query's items in order: updateDistanceLowerBoundFromBV (the minimum logged with each item, the tail after the last one
// when the walk was not stopped), updateDistanceLowerBoundFromLeaf and the contact decision of every item, the stop at
// num_max_contacts.  on_contact(k, node, leaf): contact k was added.  Writes the record (hppfcl_amd_octree_mesh.h) and the bound;
// returns numContacts().  swapped sets bit 23 only.
template <typename T, class OnContact>
HFCL_HD uint32_t octm_fold(const OctMeshItem<T>* items, const OctMeshLeafOut<T>* leaves, uint64_t n_items, T tail_box_min, T margin, T threshold,
                           uint32_t num_max_contacts, bool swapped, OnContact on_contact, hfcl_result* rec, double* dlb_out) {
  const T nanv = Lim<T>::nan();
  T dlb = Lim<T>::max();
  V3<T> np1 = mk<T>(nanv, nanv, nanv), np2 = np1, nn = np1;
  uint32_t nc = 0;
  int first_node = -1, first_prim = -1;
  OctMeshLeafOut<T> first;
  first.distance = nanv;
  first.p1 = first.p2 = first.normal = np1;
  bool stopped = false;
  for (uint64_t i = 0; i < n_items; ++i) {
    const T box_min = items[i].box_min;
    const uint32_t node = items[i].node;
    const OctMeshLeafOut<T> lf = leaves[i];
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
        first_prim = int(lf.prim);
      }
      on_contact(nc, node, lf);
      ++nc;
    }
    if (nc >= num_max_contacts) {  // isSatisfied(): the walk ends, what it has not reached does not count
      stopped = true;
      break;
    }
  }
  if (!stopped && !(dlb <= T(0)) && tail_box_min < dlb) dlb = tail_box_min;
  if (dlb_out) *dlb_out = double(dlb);
  if (rec) {
    const V3<T> p1 = nc ? first.p1 : np1, p2 = nc ? first.p2 : np2, n = nc ? first.normal : nn;
    rec->distance = double(nc ? first.distance : dlb);
    rec->normal[0] = n.x; rec->normal[1] = n.y; rec->normal[2] = n.z;
    rec->p1[0] = p1.x; rec->p1[1] = p1.y; rec->p1[2] = p1.z;
    rec->p2[0] = p2.x; rec->p2[1] = p2.y; rec->p2[2] = p2.z;
    rec->b1 = first_node;
    rec->b2 = first_prim;
    rec->status = (uint32_t(EPA_DID_NOT_RUN) << 3) | (nc ? 128u : 0u) | (swapped ? (1u << 23) : 0u);
    rec->num_contacts = int32_t(nc);
  }
  return nc;
}
template <typename T>
HFCL_HD void octm_fill_contact(hfcl_contact& c, uint32_t pair, uint32_t node, const OctMeshLeafOut<T>& lf) {
  c.pair = pair;
  c.b1 = int32_t(node);
  c.b2 = int32_t(lf.prim);
  c._pad = 0;
  c.penetration_depth = double(lf.distance);
  c.normal[0] = lf.normal.x; c.normal[1] = lf.normal.y; c.normal[2] = lf.normal.z;
  c.p1[0] = lf.p1.x; c.p1[1] = lf.p1.y; c.p1[2] = lf.p1.z;
  c.p2[0] = lf.p2.x; c.p2[1] = lf.p2.y; c.p2[2] = lf.p2.z;
}

}  // namespace hfcl

#if defined(__HIPCC__)
namespace hfcl {
// ---- the kernels' parameter block (hfcl_k_octree_mesh.hip) ------------------------------------------------------------------------
// What a chunk of octree x mesh queries adds to the pipeline's block (hfcl_listed.hpp; tf_c: the trees' poses, tf_s: the meshes';
// shape: HFCL_BV_OBBRSS rows of the shape table)
struct OctMeshArgs : ListedArgs {
  uint32_t n_trees, n_meshes;
  const DOctree* trees;
  const hfcl_octree_node* nodes;
  const uint32_t* octree;
  const DNode<double>* mnodes;  // the library's mesh tables (hfcl_lib_add_bvh)
  const double* mverts;
  const uint32_t* mtris;
  const DMesh* meshes;
  OctMeshItem<double>* items;
  OctMeshLeafOut<double>* leaves;
};
}  // namespace hfcl
// Launches of one chunk (hfcl_k_octree_mesh.hip), as launch_oct_count / launch_oct_solve
void launch_octm_count(hipStream_t st, const hfcl::OctMeshArgs& a);
void launch_octm_solve(hipStream_t st, const hfcl::OctMeshArgs& a, int max_blocks, bool want_contacts, const char** names, hipEvent_t* e0, hipEvent_t* e1);
#endif
