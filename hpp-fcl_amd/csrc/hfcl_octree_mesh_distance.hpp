// hfcl_octree_mesh_distance.hpp -- OcTree x BVHModel<OBBRSS> distance() (hppfcl_amd_octree_mesh_distance.h): the arithmetic shared by the
// kernel of hfcl_k_octree_mesh_distance.hip and the host build of the tests (tests/octree_mesh_distance_harness).
//   the entry        OcTreeSolver::OcTreeMeshDistance (internal/traversal_node_octree.h:113-124); MeshOcTreeDistanceTraversalNode calls it
//                    with the operands exchanged (:1307-1353), so both orders run the octree-first recursion
//   the walk         OcTreeMeshDistanceRecurse (:371-458), flattened over the PATH stack of the collide walk (hfcl_octree_mesh.hpp): an
//                    octree frame where the octree side descended (node, next child, box, plus the eight box distances of its children
//                    against the current mesh node), a mesh frame where the mesh side did (first child, a byte of bookkeeping, plus the
//                    two box distances of its children against the current octree box)
//   the boxes        aabb1 = Converter<AABB, AABB>::convert(bv, tf_tree) (BV/BV.h:66-73) = oct_child_box_distance's first half
//                    (hfcl_octree_distance.hpp); aabb2 = Converter<OBBRSS, AABB>::convert(bv(m), tf_mesh) (BV/BV.h:132-140, BV/OBB.h:110-122):
//                    centre R * To + T, half side ||(2 e0, 2 e1, 2 e2)|| * 0.5 on every axis -- the RSS half is not read;
//                    AABB::distance (src/BV/AABB.cpp:115-133)
//   the size rule    bv1.size() > bv(m).size(): the squared FULL diagonal against the squared norm of the HALF extents, as the collide walk
//   a leaf pair      octm_leaf (hfcl_octree_mesh.hpp) with the QParams of setup_distance: ShapeShapeDistance<Box, TriangleP>
//                    (narrowphase.h:319-336); DistanceResult::update (collision_data.h:1111-1124): a strict min_distance > distance takes the
//                    distance, the solver's own points and normal, the node and the triangle
//   the end          DistanceRequest::isSatisfied: min_distance <= 0
// A descent hangs on d < min_distance with the minimum AS IT STANDS at that moment; the distances themselves do not depend on it and are
// computed once, when a frame is pushed.  Both converted boxes enclose their bounding volumes, so d is a true lower bound: the ordered
// walk's distance is the minimum over all reachable occupied leaves x triangles whenever that minimum is positive.
// A choice: n_nodes == 0 (the reference dereferences a null root) answers with the untouched DistanceResult.
// Every unit that includes this is built without contraction of a*b+c; every sum of products is written left to right.
// Builds with hipcc and with g++.
#pragma once
#include "../../include/hppfcl_amd_octree_mesh_distance.h"
#include "hfcl_octree_distance.hpp"
#include "hfcl_octree_mesh.hpp"

namespace hfcl {

// the walk's path stack of one query (in LDS: one per lane group)
template <typename T>
struct OctMeshDistStack {
  uint32_t node[OCT_STACK], next[OCT_STACK];
  T box[OCT_STACK][6];  // the node's own box: min xyz, max xyz
  T d[OCT_STACK][8];    // aabb1(child i).distance(aabb2(the frame's mesh node)) (0 where there is no child)
  uint32_t m[OCTM_MESH_STACK];  // the first child of the mesh node
  uint8_t mo[OCTM_MESH_STACK];  // bits 0-4: the octree frames below; bits 5-6: which child comes next
  T md[OCTM_MESH_STACK][2];     // aabb1(the frame's octree box).distance(aabb2(left / right child))
};
struct OctMeshDistWalk {
  int osp, msp;
  uint64_t steps, max_steps;  // 2 * n_nodes * n_mesh_nodes + 2: a pair of nodes is entered once, and tested once as a child
  bool started, overflow;
};
// DistanceResult
template <typename T>
struct OctMeshDistResult {
  T min_distance;
  V3<T> p1, p2, normal;
  int32_t b1, b2;
  uint32_t visited;  // (leaf, triangle) pairs solved
};
template <typename T>
HFCL_HD void octmd_clear(OctMeshDistResult<T>& r) {
  const T nanv = Lim<T>::nan();
  r.min_distance = Lim<T>::max();
  r.p1 = r.p2 = r.normal = mk<T>(nanv, nanv, nanv);
  r.b1 = r.b2 = -1;
  r.visited = 0;
}
template <typename T>
HFCL_HD void octmd_update(OctMeshDistResult<T>& r, uint32_t node, uint32_t prim, const OctMeshLeafOut<T>& lf) {
  ++r.visited;
  if (r.min_distance > lf.distance) {
    r.min_distance = lf.distance;
    r.p1 = lf.p1;
    r.p2 = lf.p2;
    r.normal = lf.normal;
    r.b1 = int32_t(node);
    r.b2 = int32_t(prim);
  }
}
// the record: the layout of oct_dist_record with the triangle in b2
template <typename T>
HFCL_HD void octmd_record(const OctMeshDistResult<T>& r, bool swapped, hfcl_result* rec) {
  rec->distance = double(r.min_distance);
  rec->normal[0] = r.normal.x; rec->normal[1] = r.normal.y; rec->normal[2] = r.normal.z;
  rec->p1[0] = r.p1.x; rec->p1[1] = r.p1.y; rec->p1[2] = r.p1.z;
  rec->p2[0] = r.p2.x; rec->p2[1] = r.p2.y; rec->p2[2] = r.p2.z;
  rec->b1 = r.b1;
  rec->b2 = r.b2;
  rec->status = (uint32_t(EPA_DID_NOT_RUN) << 3) | (r.min_distance <= T(0) ? 128u : 0u) | (swapped ? (1u << 23) : 0u);
  rec->num_contacts = 0;
}

// Converter<OBBRSS, AABB>::convert(bv, tf_mesh): the OBB half alone
template <typename T>
HFCL_HD void octm_node_aabb(const Pose<T>& tfm, const V3<T>& To, const V3<T>& extent, V3<T>& blo, V3<T>& bhi) {
  const V3<T> c2 = mul(tfm.R, To) + tfm.t;
  const T r = norm(mk<T>(T(2) * extent.x, T(2) * extent.y, T(2) * extent.z)) * T(0.5);  // width(), height(), depth()
  blo = mk<T>(c2.x - r, c2.y - r, c2.z - r);
  bhi = mk<T>(c2.x + r, c2.y + r, c2.z + r);
}

HFCL_HD void octmd_walk_init(OctMeshDistWalk& w, const DOctree& tr, uint32_t n_mnodes) {
  w.osp = w.msp = 0;
  w.steps = 0;
  w.max_steps = 2u * uint64_t(tr.n_nodes) * uint64_t(n_mnodes) + 2u;
  w.started = false;
  w.overflow = false;
}

// Advances the walk to the next (leaf, triangle) pair to solve (true: the node, its box, the triangle) or to its end (false).
// min_distance: the minimum as it stands.  Run by every lane of the group with the same arguments: lane 0 writes the frames, lanes 0..7
// the eight box distances of an octree frame that is pushed, lanes 0..1 the two of a mesh frame (they do not depend on the minimum;
// their comparisons, taken serially in order when a child comes up, do).  The state is the recursion's path, as octm_walk keeps it: the
// mesh frame on top is the newest frame iff no octree frame was pushed since; the current octree node of a mesh frame is the child the
// top octree frame went into last (none: the root), the current mesh node of an octree frame likewise -- neither changes while the
// frame lives.  overflow: a stack was too small -- the walk ends there; the host refuses meshes deeper than OCTM_MESH_DEPTH before any
// launch and the validator trees deeper than 16, so this is unreachable, and the guard stays.
template <typename T, class Grp>
HFCL_HD bool octmd_next(const hfcl_octree_node* nodes, const DOctree& tr, const Pose<T>& tft, const DNode<T>* mnodes, uint32_t n_mnodes,
                        const Pose<T>& tfm, T min_distance, OctMeshDistStack<T>* st, OctMeshDistWalk& w, uint32_t& leaf, V3<T>& llo, V3<T>& lhi,
                        uint32_t& prim) {
  const int lig = Grp::lane();
  // one entry of the recursion; true: an occupied leaf against a triangle -- to be solved; else the pair ended its branch or a frame
  // with its children is on the stack
  auto enter = [&](uint32_t o, const V3<T>& lo, const V3<T>& hi, uint32_t m) {
    uint32_t any = 0;
    for (int k = 0; k < 8; ++k) any |= nodes[o].child[k];
    const int fc = mnodes[m].first_child;
    const bool mleaf = fc < 0;
    const bool occupied = nodes[o].occupancy >= tr.occupancy_threshold;  // isNodeOccupied: free and uncertain are the same here
    if (!any && mleaf) {
      if (!occupied) return false;
      leaf = o;
      llo = lo;
      lhi = hi;
      prim = uint32_t(-(fc + 1));
      return true;
    }
    if (!occupied) return false;
    if (mleaf || (any && sqnorm(hi - lo) > sqnorm(mnodes[m].extent))) {  // AABB::size(): the FULL diagonal squared; OBBRSS::size(): the HALF extents squared
      if (w.osp >= OCT_STACK) {  // (cannot happen with a validated tree)
        w.overflow = true;
        return false;
      }
      const int at = w.osp;
      Grp::sync();
      if (lig == 0) {
        st->node[at] = o;
        st->next[at] = 0u;
        st->box[at][0] = lo.x; st->box[at][1] = lo.y; st->box[at][2] = lo.z;
        st->box[at][3] = hi.x; st->box[at][4] = hi.y; st->box[at][5] = hi.z;
      }
      V3<T> blo, bhi;
      octm_node_aabb(tfm, mnodes[m].To, mnodes[m].extent, blo, bhi);  // aabb2
      for (int k = lig; k < 8; k += Grp::W) {  // (a 16-lane group: lanes 0..7, one child each)
        T d = T(0);
        if (nodes[o].child[k] != 0u) {
          V3<T> clo, chi;
          oct_child_box(lo, hi, uint32_t(k), clo, chi);
          d = oct_child_box_distance(tft, clo, chi, blo, bhi);
        }
        st->d[at][k] = d;
      }
      ++w.osp;
      Grp::sync();
      return false;
    }
    if (w.msp >= OCTM_MESH_STACK || fc <= 0 || uint32_t(fc) + 1u >= n_mnodes) {  // (refused before any launch / at registration)
      w.overflow = true;
      return false;
    }
    const int at = w.msp;
    Grp::sync();
    if (lig == 0) {
      st->m[at] = uint32_t(fc);
      st->mo[at] = uint8_t(w.osp);
    }
    for (int k = lig; k < 2; k += Grp::W) {  // (lanes 0..1: the left and the right child)
      V3<T> blo, bhi;
      octm_node_aabb(tfm, mnodes[fc + k].To, mnodes[fc + k].extent, blo, bhi);
      st->md[at][k] = oct_child_box_distance(tft, lo, hi, blo, bhi);  // aabb1 of the current bv1
    }
    ++w.msp;
    Grp::sync();
    return false;
  };
  const T rh = T(tr.root_half);
  const V3<T> rlo = mk<T>(-rh, -rh, -rh), rhi = mk<T>(rh, rh, rh);
  if (!w.started) {
    w.started = true;
    if (tr.n_nodes == 0 || n_mnodes == 0) return false;  // the empty tree (a choice: the reference dereferences a null root)
    if (enter(0u, rlo, rhi, 0u)) return true;             // the root pair gets no box test
  }
  while ((w.osp > 0 || w.msp > 0) && !w.overflow && w.steps < w.max_steps) {  // (bound: 2 * n_nodes * n_mesh_nodes + 2 steps over the whole walk)
    ++w.steps;
    if (w.msp > 0 && int(st->mo[w.msp - 1] & 31u) == w.osp) {  // a mesh frame is the newest: its left child, then its right
      const int top = w.msp - 1;
      const uint32_t which = uint32_t(st->mo[top]) >> 5;
      if (which >= 2u) {
        --w.msp;
        continue;
      }
      Grp::sync();
      if (lig == 0) st->mo[top] = uint8_t(uint32_t(w.osp) | ((which + 1u) << 5));
      Grp::sync();
      const uint32_t cm = st->m[top] + which;
      if (!(st->md[top][which] < min_distance)) continue;  // `if (d < dresult->min_distance)`
      if (w.osp == 0) {
        if (enter(0u, rlo, rhi, cm)) return true;
        continue;
      }
      const int otop = w.osp - 1;
      const uint32_t i = (st->next[otop] - 1u) & 7u;  // (a frame under a mesh frame has gone into a child)
      const V3<T> lo = mk<T>(st->box[otop][0], st->box[otop][1], st->box[otop][2]), hi = mk<T>(st->box[otop][3], st->box[otop][4], st->box[otop][5]);
      V3<T> clo, chi;
      oct_child_box(lo, hi, i, clo, chi);
      if (enter(nodes[st->node[otop]].child[i], clo, chi, cm)) return true;
      continue;
    }
    const int top = w.osp - 1;  // an octree frame is the newest: its existing children in index order
    const uint32_t node = st->node[top];
    uint32_t i = st->next[top];
    while (i < 8u && nodes[node].child[i] == 0u) ++i;  // (bound: 8)
    if (i >= 8u) {
      --w.osp;
      continue;
    }
    Grp::sync();
    if (lig == 0) st->next[top] = i + 1u;
    Grp::sync();
    const uint32_t child = nodes[node].child[i];
    if (child >= tr.n_nodes) continue;               // (refused by the validator)
    if (!(st->d[top][i] < min_distance)) continue;  // `if (d < dresult->min_distance)`
    const V3<T> lo = mk<T>(st->box[top][0], st->box[top][1], st->box[top][2]), hi = mk<T>(st->box[top][3], st->box[top][4], st->box[top][5]);
    V3<T> clo, chi;
    oct_child_box(lo, hi, i, clo, chi);
    uint32_t cm = 0u;
    if (w.msp > 0) {
      const uint32_t which = uint32_t(st->mo[w.msp - 1]) >> 5;  // (>= 1: a frame under an octree frame has gone into a child)
      cm = st->m[w.msp - 1] + ((which - 1u) & 1u);
    }
    if (enter(child, clo, chi, cm)) return true;
  }
  return false;
}

// One query: "advance the walk to the next pair to solve, or to its end; then solve".  q: setup_distance of the request (DefaultGuess).
// The groups of a wave meet at the solve.  r is the same on every lane of the group.  on_pair(node, triangle): a pair is about to be
// solved (the tests' host build lists them; the kernel passes nothing).  mverts / mtris: the mesh's own vertices and triangles
template <typename T, class Grp, class OnPair>
HFCL_HD void octm_distance_query(const hfcl_octree_node* nodes, const DOctree& tr, const Pose<T>& tft, const DNode<T>* mnodes, uint32_t n_mnodes,
                                 const T* mverts, const uint32_t* mtris, const Pose<T>& tfm, const QParams<T>& q, OctMeshDistStack<T>* st,
                                 EpaScratch<T, EPA_MAX_ITER>* scratch, OctMeshDistResult<T>& r, bool& overflow, OnPair on_pair) {
  octmd_clear(r);
  OctMeshDistWalk w;
  octmd_walk_init(w, tr, n_mnodes);
  for (uint64_t pass = 0; pass < w.max_steps; ++pass) {  // (bound: a pass solves one pair, and a pair of nodes is entered once)
    uint32_t leaf = 0, prim = 0;
    V3<T> llo, lhi;
    if (!octmd_next<T, Grp>(nodes, tr, tft, mnodes, n_mnodes, tfm, r.min_distance, st, w, leaf, llo, lhi, prim)) break;
    on_pair(leaf, prim);
    OctMeshLeafOut<T> lf;
    octm_leaf<T, Grp>(llo, lhi, tft, mverts, mtris + 3 * size_t(prim), tfm, q, scratch, lf);
    octmd_update(r, leaf, prim, lf);
    if (r.min_distance <= T(0)) break;  // DistanceRequest::isSatisfied
  }
  overflow = w.overflow;
}
struct OctMeshDistNoList {
  HFCL_HD void operator()(uint32_t, uint32_t) const {}
};

}  // namespace hfcl

#if defined(__HIPCC__)
namespace hfcl {
// ---- the kernel's parameter block (hfcl_k_octree_mesh_distance.hip): a chunk of m queries of a call ----------------------------------
struct OctMeshDistArgs {
  const DShape<double>* shapes;  // HFCL_BV_OBBRSS rows of the shape table name the meshes (bvh_index)
  uint32_t n_shapes, n_trees, n_meshes;
  const DOctree* trees;
  const hfcl_octree_node* nodes;
  const DNode<double>* mnodes;  // the library's mesh tables (hfcl_lib_add_bvh)
  const double* mverts;
  const uint32_t* mtris;
  const DMesh* meshes;
  const uint32_t* octree;
  const uint32_t* shape;
  const double* tf_t;
  const double* tf_m;
  const uint8_t* swapped;  // nullptr: none
  uint32_t m;
  QParams<double> q;
  hfcl_result* out;
  uint32_t* n_visited;     // nullptr or m
};
}  // namespace hfcl
void launch_octm_distance(hipStream_t st, const hfcl::OctMeshDistArgs& a, int max_blocks);  // k_octm_distance
#endif
