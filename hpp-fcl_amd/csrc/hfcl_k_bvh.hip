// hfcl_k_bvh.hip -- BVHModel<OBBRSS> x BVHModel<OBBRSS> collide() and top-level TriangleP pairs (hfcl_k_bvh.o), with hipcc's default
// contraction (Makefile).  The lanes' walk, its task levels and the walk in rounds are templates this object shares with mesh x solid
// collide() (hfcl_mesh_collide.hpp, which also says what keeps the mesh objects' kernels apart); here: the waves' continuation, the listed
// triangle pairs, k_triangle and the launchers.
#include "hfcl_mesh_collide.hpp"

constexpr int MESH_UNIT_PART = 1;  // what this object's copy of a kernel two mesh objects launch carries (hfcl_mesh_collide.hpp); named once, passed explicitly below

// ---------------------------------------------------------------------------------------
// k_bvh_coop: the continuation of k_bvh_shape_coop (hfcl_k_bvhc.hip, where it is described) for mesh x mesh walks (BvhSplit::coop
// on the plain form of k_bvh_collide): a query that used up its step budget is taken over by a lane group that walks COOP_W entries of its (ordered) stack per trip.  An entry
// is a pair of nodes; a box pair that overlaps is replaced by its two successors (firstOverSecond decides which node is
// split), a disjoint one by its bound, a pair of leaves by its triangles' distance -- applied in stack order exactly as in
// k_bvh_shape_coop (same scans, hfcl_mesh_collide.hpp), so the record is the sequential walk's.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 8)))
k_bvh_coop(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q, BvhParams bp, T break_distance2, BvhSplit split) {
  constexpr int W = COOP_W, G = 64 / W;
  typedef BvhEntry<false> EN;
  __shared__ uint32_t stacks[G][COOP_CAP + COOP_SLACK];
  __shared__ T w0_slab[W0Lds<T, 64>::WORDS];
  const W0Lds<T, 64> leaf_ps{w0_slab + threadIdx.x};
  const int lane = threadIdx.x, grp = lane / W, lig = lane & (W - 1);
  uint32_t* const stack = stacks[grp];
  const uint64_t gbits = W == 64 ? ~uint64_t(0) : ((uint64_t(1) << (W & 63)) - 1);
  auto gballot = [&](bool x) -> uint64_t { return (__ballot(x) >> (grp * W)) & gbits; };
  // the units of this launch: the suspended queries (level 0), or the chunks the launch before cut its long walks into (see above)
  const uint32_t level = split.level;
  uint32_t unit0 = level ? min(split.ctr[BVH_CTR_LEVEL0 + level - 1], split.cap) : 0u;
  uint32_t n_units = level ? min(split.ctr[BVH_CTR_LEVEL0 + level], split.cap) - unit0 : 0u;
  uint32_t* ticket = &wk.counts[B_COUNT + 2];  // (k_bvh_collide is through with it; k_bvh_level_mark has reset it)
  if (!level) {
    const uint32_t cr = split.coop_range;
    if (cr && cr < 0x100u) {  // what round cr - 1 of the walk handed over; the later rounds append to the list meanwhile
      const uint32_t r = cr - 1u;
      unit0 = r ? min(split.walk.ctr[8u * (r - 1u) + WALK_CTR_SNAP], split.n_queries) : 0u;
      n_units = min(split.walk.ctr[8u * r + WALK_CTR_SNAP], split.n_queries) - unit0;
      ticket = &split.walk.ctr[8u * r + WALK_CTR_TICKET_EARLY];
    } else {
      const uint32_t tot = min(split.ctr[BVH_CTR_SUSPENDED], split.n_queries);
      if (cr) unit0 = min(split.walk.ctr[8u * (cr - 0x100u) + WALK_CTR_SNAP], tot);
      n_units = tot - unit0;
    }
  }
  if (n_units == 0u) return;  // (nothing suspended: no wave draws a ticket)
  const unsigned long long cut_ticks = split.can_suspend ? split.cut_ticks : 0u;
  const T big = Lim<T>::max();
  bool have = false, overflow = false, exhausted = false;
  uint32_t pair = 0, ncontacts = 0;
  uint32_t unit = 0, my_parent = 0xFFFFFFFFu, my_order = 0;
  unsigned long long t_begin = 0, t_wave = __builtin_readcyclecounter();
  unsigned n_walks = 0, trip_no = 0;
  (void)t_wave; (void)n_walks;
  DMesh m1 = {0, 0, 0, 0}, m2 = {0, 0, 0, 0};
  M3<T> RT_R;
  V3<T> RT_T = mk<T>(T(0), T(0), T(0));
  RT_R.r0 = RT_R.r1 = RT_R.r2 = RT_T;
  int sp = 0, fb1 = -1, fb2 = -1;
  T dlb = big, rec_dist = big, cand_val = big;
  V3<T> np1 = RT_T, np2 = RT_T, nn = RT_T;
  for (;;) {
    if (!have && !exhausted) {
      const CoopUnit u = coop_draw<T, W>(split, ticket, level, unit0, n_units, lig, grp);
      exhausted = u.exhausted;
      if (u.take) {
      BvhSum<T> s;
      if (level) {  // a chunk starts from an empty state
        s.dlb = s.rec_dist = s.cand_val = big;
        s.np1 = s.np2 = s.nn = mk<T>(Lim<T>::nan(), Lim<T>::nan(), Lim<T>::nan());
        s.flags = 0u;
        s.first_child = u.first;
        s.n_child = u.count;
      } else {
        s = *bvh_sum<T>(split, u.index);
      }
      pair = u.pair;
      unit = u.index;
      my_parent = u.parent;
      my_order = u.order;
      m1 = bv.meshes[lib.shapes[wk.shape1[pair]].bvh_index];
      m2 = bv.meshes[lib.shapes[wk.shape2[pair]].bvh_index];
      {
        const Pose<T> tf1 = load_pose(io.tf1, pair), tf2 = load_pose(io.tf2, pair);
        RT_R = tmul(tf1.R, tf2.R);  // traversal_node_setup.h:560-563
        RT_T = tmul(tf1.R, tf2.t - tf1.t);
      }
      if (level) {
        for (uint32_t j = uint32_t(lig); j < s.n_child; j += uint32_t(W)) stack[s.n_child - 1u - j] = split.cut_words[s.first_child + j];  // the chunk's entries
      } else {
        for (uint32_t j = uint32_t(lig); j < s.n_child; j += uint32_t(W)) stack[s.n_child - 1u - j] = split.tasks[s.first_child + j].entry;  // child 0 on top
      }
      sp = int(s.n_child);
      dlb = s.dlb;
      rec_dist = s.rec_dist;
      cand_val = s.cand_val;
      t_begin = __builtin_readcyclecounter();
      ++n_walks;
      np1 = s.np1;
      np2 = s.np2;
      nn = s.nn;
      fb1 = fb2 = -1;
      ncontacts = 0;
      overflow = (s.flags & BVH_SUM_OVERFLOW) != 0 || sp > COOP_CAP;
      if (overflow) sp = 0;
      have = true;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (!__any(have)) {
      if (__all(exhausted)) break;
      continue;  // (the units drawn were chunks nobody needs)
    }
    if (have && level && (++trip_no & 15u) == 0u && bvh_moot<T>(split, my_parent, my_order)) {
      // (every 16th trip: the look costs a dependent load per level, every trip 3.3 -> 3.75 ms on cfg4s) a chunk in front of this one
      // has found a contact meanwhile: the sequential walk ended there, nobody reads this summary
      if (lig == 0) bvh_sum<T>(split, split.n_queries + unit0 + unit)->flags = 0u;
      COOP_WALK_END(lig == 0, t_begin);
      have = false;
      continue;
    }
    bool done = have && sp == 0;
    if (have && sp > 0) {
      const int w = min(W, min(sp, max(COOP_CAP - sp, 1)));
      const bool act = lig < w;
      const uint32_t e = act ? stack[sp - 1 - lig] : 0u;
      sp -= w;
      const uint32_t b1 = EN::first(e), b2 = EN::second(e);
      const DNode<T>* const p1n = bv.nodes + m1.node_off + b1;
      const DNode<T>* const p2n = bv.nodes + m2.node_off + b2;
      const int32_t fc1 = act ? p1n->first_child : 0, fc2 = act ? p2n->first_child : 0;
      const bool l1 = fc1 < 0, l2 = fc2 < 0;
      const bool is_leaf = act && l1 && l2, is_int = act && !(l1 && l2);
      T val = big, recv = big;
      bool overlap = false, first = false;
      if (is_int) {
        const DNode<T> n1 = *p1n;
        const DNode<T> n2 = *p2n;
        first = l2 || (!l1 && (sqnorm(n1.extent) > sqnorm(n2.extent)));  // firstOverSecond
        T sq;
        // argument order of the reference: overlap(RT.R, RT.T, model2.bv(b2), model1.bv(b1))
        if (obb_disjoint(RT_R, RT_T, n2, n1, q.security_margin, break_distance2, sq)) {  // updateDistanceLowerBoundFromBV
          const T nd = hsqrt(sq);
          val = nd;
          recv = nd + q.security_margin;
        } else {
          overlap = true;
        }
      }
      const uint64_t omask = gballot(overlap);
      const int f = omask ? __ffsll((unsigned long long)omask) - 1 : W;  // entries [0, f) are visited now
      bool visit = act && lig < f;
      bool contact = false, leaf_ok = false;
      TriLeafOut<T> lo;
      lo.distance = big;
      const uint32_t lb1 = uint32_t(-(fc1 + 1)), lb2 = uint32_t(-(fc2 + 1));
      if (is_leaf && visit) {
        tri_leaf_call<T>(bv.verts + 3 * size_t(m1.vert_off), bv.tris + 3 * size_t(m1.tri_off + lb1), bv.verts + 3 * size_t(m2.vert_off),
                         bv.tris + 3 * size_t(m2.tri_off + lb2), io.tf1, io.tf2, pair, &q, leaf_ps, &lo);
        const T dtc = lo.distance - q.security_margin;  // updateDistanceLowerBoundFromLeaf
        val = dtc;
        recv = lo.distance;
        contact = dtc <= q.collision_distance_threshold;
        leaf_ok = true;
      }
      const uint64_t cmask = gballot(contact);
      const int c = cmask ? __ffsll((unsigned long long)cmask) - 1 : W;  // the first contact in stack order ends the walk
      visit = visit && lig <= c;
      if (!visit) {
        val = big;
        leaf_ok = false;
      }
      const T before = hmin(dlb, group_min_excl_scan<T, W>(val, lig, big));  // the bound as entry `lig` found it
      const bool lowered = visit && val < before;
      const T wmin = group_min_all<T, W>(val);
      if (gballot(lowered)) {
        const int src = __ffsll((unsigned long long)gballot(visit && val == wmin)) - 1;
        dlb = wmin;
        rec_dist = __shfl(recv, src, W);
      }
      const uint64_t wmask = gballot(lowered && leaf_ok);  // the witness: the last leaf that lowered the bound on its visit
      {
        const int L = wmask ? 63 - __clzll((unsigned long long)wmask) : 0;
        const V3<T> c1 = mk<T>(__shfl(lo.p1.x, L, W), __shfl(lo.p1.y, L, W), __shfl(lo.p1.z, L, W));
        const V3<T> c2 = mk<T>(__shfl(lo.p2.x, L, W), __shfl(lo.p2.y, L, W), __shfl(lo.p2.z, L, W));
        const V3<T> cn = mk<T>(__shfl(lo.n.x, L, W), __shfl(lo.n.y, L, W), __shfl(lo.n.z, L, W));
        if (wmask) {
          np1 = c1;
          np2 = c2;
          nn = cn;
          cand_val = __shfl(val, L, W);
        }
      }
      const int cs = c < W ? c : 0;
      const int cb1 = __shfl(int(lb1), cs, W), cb2 = __shfl(int(lb2), cs, W);
      if (c < W) {  // canStop() (num_max_contacts == 1: the split forms only)
        fb1 = cb1;
        fb2 = cb2;
        ncontacts = 1;
        sp = 0;
      } else {
        const int cnt = !act || lig < f ? 0 : (overlap ? 2 : 1);
        const uint64_t mm2 = gballot(cnt == 2), mm1 = gballot(cnt == 1);
        const uint64_t deeper = ~((uint64_t(2) << lig) - 1);  // window entries behind this one (pushed first)
        const int pos = sp + 2 * __popcll(mm2 & deeper) + __popcll(mm1 & deeper);
        if (cnt == 2) {
          uint32_t ea, eb;
          if (first) {
            ea = EN::pack(uint32_t(fc1), b2);
            eb = EN::pack(uint32_t(fc1) + 1u, b2);
          } else {
            ea = EN::pack(b1, uint32_t(fc2));
            eb = EN::pack(b1, uint32_t(fc2) + 1u);
          }
          stack[pos] = eb;      // second child below
          stack[pos + 1] = ea;  // first child on top
        } else if (cnt == 1) {
          stack[pos] = e;
        }
        sp += 2 * __popcll(mm2) + __popcll(mm1);
        if (sp > COOP_CAP + COOP_SLACK - 2) {
          overflow = true;
          sp = 0;
        }
      }
      done = sp == 0;
      if (cut_ticks && sp > COOP_CHUNK && __builtin_readcyclecounter() - t_begin > cut_ticks) {
        // ---- the walk has had its time: what is left of it becomes chunks for the next launch (coop_cut)
        if (coop_cut<T, W>(split, level ? split.n_queries + unit0 + unit : unit, pair, my_parent, my_order, stack, static_cast<const T*>(nullptr), sp, lig, dlb, rec_dist, cand_val,
                           np1, np2, nn, overflow)) {
          COOP_CUT_COUNT(lig == 0);
          COOP_WALK_END(lig == 0, t_begin);
          have = false;
          sp = 0;
        } else {
          t_begin = __builtin_readcyclecounter();  // (no room: the walk goes on and asks again after another budget)
        }
      }
    }
    if (done && level) {
      // ---- a chunk's summary (k_bvh_combine folds it into the walk it was cut from)
      if (lig == 0) {
        coop_write_sum<T>(split, split.n_queries + unit0 + unit, dlb, rec_dist, cand_val, np1, np2, nn, fb1, fb2, ncontacts, 0u, 0u,
                          overflow ? BVH_SUM_OVERFLOW : 0u, my_parent, my_order);
        if (ncontacts) coop_report_contact<T>(split, my_parent, my_order);
      }
      COOP_WALK_END(lig == 0, t_begin);
      have = false;
      done = false;
    }
    if (done) {
      if (lig == 0) {
        bvh_sum<T>(split, unit)->flags = 0u;  // (not cut: k_bvh_combine has nothing to fold for this query)
        PairOut<T> o;
        o.distance = rec_dist;
        o.normal = nn;
        o.p1 = np1;
        o.p2 = np2;
        o.gjk_status = GJK_DID_NOT_RUN;
        o.epa_status = EPA_DID_NOT_RUN;
        o.gjk_iters = o.epa_iters = 0;
        store_bvh_record(io, pair, o, ncontacts, fb1, fb2, overflow);
      }
      COOP_WALK_END(lig == 0, t_begin);
      have = false;
    }
  }
  COOP_WAVE_END(t_wave, n_walks);
}

// ---------------------------------------------------------------------------------------
// k_triangle: top-level TriangleP pairs (other than against Plane / Halfspace, which are closed forms):
// TriangleP x TriangleP (triangle_triangle.cpp:46-105), TriangleP x Sphere (triangle_sphere.cpp:45-68) and
// TriangleP x {Box, Capsule, Cone, Cylinder, Ellipsoid, ConvexBase} through GJKSolver::shapeDistance's
// TriangleP overloads (narrowphase.h:320-348).  One pair per BS_W-lane group, as the mesh x solid leaves.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(64) k_triangle(Work wk, LibView<T> lib, IO<T> io, QParams<T> q) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<T, EPA_MAX_ITER> scratch[G];
  const uint32_t cnt = wk.counts[B_TRI];
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint32_t it = blockIdx.x * G + grp; it < cnt; it += gridDim.x * G) {
    const uint32_t pair = wk.lists[size_t(B_TRI) * wk.n + it];
    const DShape<T> a = lib.shapes[wk.shape1[pair]], b = lib.shapes[wk.shape2[pair]];
    const Pose<T> tf1 = load_pose(io.tf1, pair), tf2 = load_pose(io.tf2, pair);
    const bool t1 = a.kind == K_TRIANGLE;
    GroupSolid<T> solid;  // the non-triangle shape (unused for TriangleP x TriangleP)
    solid.s = t1 ? b : a;
    solid.v = lib.verts + 3 * size_t(solid.s.vertex_offset);
    solid.lig = lig;
    if (solid.s.kind == K_CONVEX && solid.s.num_points <= uint32_t(HULL_MAX)) solid.h.load(solid.v, solid.s.num_points, lig);
    PairOut<T> o;
    triangle_pair<T, LaneGroup<BS_W>>(a, b, lib.verts, tf1, tf2, solid, q, initial_guess<T>(io, q, pair), &scratch[grp], o);
    if (lig == 0) {
      write_out<T>(io, q, pair, o);
      write_guess<T>(io, pair, o.cached_guess, 0, 0);
    }
    LaneGroup<BS_W>::sync();
  }
}

#ifndef HFCL_TRI_LEAVES_INLINE
#define HFCL_TRI_LEAVES_INLINE 1
#endif
// k_tri_leaves: every triangle pair the round's walks listed, one per lane (leafCollides' distance, traversal_node_bvhs.h:184-233).
// By default (HFCL_TRI_LEAVES_INLINE = 1) the leaf is this kernel's own inlined copy of tri_tri_distance, as k_bvh_collide's, while
// k_bvh_coop runs the non-inlined tri_leaf_call: a triangle pair has more than one machine code in this object, which keeps hipcc's
// default contraction (Makefile: FLAGS_k_bvh), and which copy tests a pair depends on the rounds and budgets chosen for the batch.
// HFCL_TRI_LEAVES_INLINE = 0: the one tri_leaf_call for both.
template <typename T>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 8)))
k_tri_leaves(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q, WalkArgs wa) {
  __shared__ T w0_slab[W0Lds<T, 64>::WORDS];
  const W0Lds<T, 64> leaf_ps{w0_slab + threadIdx.x};
  const WalkRec<T>* const recs = reinterpret_cast<const WalkRec<T>*>(wa.recs);
  TriLeafOut<T>* const res = reinterpret_cast<TriLeafOut<T>*>(wa.res);
  const uint32_t n_items = min(wa.ctr[8 * wa.round + 1], wa.item_cap);
  for (uint32_t base = blockIdx.x * 64u; base < n_items; base += gridDim.x * 64u) {
    const uint32_t it = base + threadIdx.x;
    if (it < n_items) {
      const uint32_t item = wa.items[it];
      const WalkRec<T>* const r = recs + (item & 0x0FFFFFFFu);
      const uint32_t s2 = item >> 28, pair = r->pair;
      const DMesh m1 = bv.meshes[lib.shapes[wk.shape1[pair]].bvh_index], m2 = bv.meshes[lib.shapes[wk.shape2[pair]].bvh_index];
      TriLeafOut<T> tlo;
#if HFCL_TRI_LEAVES_INLINE
      {  // the leaf inline (k_bvh_collide's form of it): no walk shares the lane's registers here, and the call cost 192 B of scratch per lane
        const T* const v1 = bv.verts + 3 * size_t(m1.vert_off);
        const T* const v2 = bv.verts + 3 * size_t(m2.vert_off);
        const uint32_t* const t1 = bv.tris + 3 * size_t(m1.tri_off + r->leaf1[s2]);
        const uint32_t* const t2 = bv.tris + 3 * size_t(m2.tri_off + r->leaf2[s2]);
        auto vtx = [](const T* v, uint32_t i) { return mk<T>(v[3 * size_t(i)], v[3 * size_t(i) + 1], v[3 * size_t(i) + 2]); };
        TriSupport<T> tri;
        {
          const Pose<T> tf1 = load_pose(io.tf1, pair);
          tri.p1 = xform(tf1, vtx(v1, t1[0]));
          tri.p2 = xform(tf1, vtx(v1, t1[1]));
          tri.p3 = xform(tf1, vtx(v1, t1[2]));
        }
        {
          const Pose<T> tf2 = load_pose(io.tf2, pair);
          tri.q1 = xform(tf2, vtx(v2, t2[0]));
          tri.q2 = xform(tf2, vtx(v2, t2[1]));
          tri.q3 = xform(tf2, vtx(v2, t2[2]));
        }
        int gst, git;
        tlo.distance = tri_tri_distance(tri, q.gjk, q.guess_mode == HFCL_GUESS_CACHED, mk<T>(q.guess[0], q.guess[1], q.guess[2]), tlo.p1, tlo.p2, tlo.n, gst, git,
                                        (V3<T>*)nullptr, leaf_ps);
      }
#else
      tri_leaf_call<T>(bv.verts + 3 * size_t(m1.vert_off), bv.tris + 3 * size_t(m1.tri_off + r->leaf1[s2]), bv.verts + 3 * size_t(m2.vert_off),
                       bv.tris + 3 * size_t(m2.tri_off + r->leaf2[s2]), io.tf1, io.tf2, pair, &q, leaf_ps, &tlo);
#endif
      res[it] = tlo;
    }
  }
}

// =======================================================================================
// launchers (hfcl_launch.hpp), over the level launches of hfcl_mesh_collide.hpp
// =======================================================================================
// one launch of the collide kernel in the form the batch asks for: WIDE (32-bit node ids) or not, with the fp32 filter in
// front of the fp64 test (fp64 batches of a library whose filter records are uploaded, bv.fnodes) or without
template <typename T>
static void launch_collide_kernel(bool wide, int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, const BvhParams& bp, T break_distance2, const BvhSplit& split, const BvhSpill& spill) {
#if HFCL_KEEP_AB_FORMS
  if constexpr (sizeof(T) == 8) {
    if (bv.fnodes) {
      if (wide)
        hipLaunchKernelGGL((k_bvh_collide<T, true, true>), dim3(grid), dim3(BVH_BLOCK), 0, st, wk, lv, bv, io, q, bp, break_distance2, split, spill);
      else
        hipLaunchKernelGGL((k_bvh_collide<T, false, true>), dim3(grid), dim3(BVH_BLOCK), 0, st, wk, lv, bv, io, q, bp, break_distance2, split, spill);
      return;
    }
  }
#endif
  if (wide)
    hipLaunchKernelGGL((k_bvh_collide<T, true, false>), dim3(grid), dim3(BVH_BLOCK), 0, st, wk, lv, bv, io, q, bp, break_distance2, split, spill);
  else
    hipLaunchKernelGGL((k_bvh_collide<T, false, false>), dim3(grid), dim3(BVH_BLOCK), 0, st, wk, lv, bv, io, q, bp, break_distance2, split, spill);
}
template <typename T>
void launch_bvh_collide(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, const BvhParams& bp, T break_distance2, BvhSplit split, BvhSpill spill, const AsideStream* aside) {
  if (spill.wide) {  // models with 32-bit node ids: single pass, global spill instead of tasks
    split.tasks = nullptr;
    split.budget = 0;
    split.level = 0;
    split.can_suspend = 0;
    if (spill.slab) grid = std::min(grid, int(spill.max_blocks));
    launch_collide_kernel<T>(true, grid, st, wk, lv, bv, io, q, bp, break_distance2, split, spill);
    return;
  }
  if (bvh_splitting(split, bp) && split.coop) {
    // the queries for their step budget, one per lane; then the suspended ones, a lane group each (k_bvh_coop)
    BvhSplit s0 = split;
    s0.level = 0;
    s0.budget = split.budget0;
    s0.can_suspend = 1;
    uint32_t n_early = 0;  // helper streams with a continuation launch on them
    if (split.walk.recs && split.walk_rounds) {
      // the queries' own phase in rounds: walk (its leaves listed), leaves (one per lane), resolve (hfcl_dev.hpp: WalkRec)
      WalkArgs wa = split.walk;
      uint32_t* const lists = wa.list_in;
      const int lgrid = std::max(1, std::min(grid * 2, int(split.coop_grid ? split.coop_grid : 2048u)));
      // The queries a round hands over (step budget) are continued on a helper stream BESIDE the later rounds: at 100k queries neither
      // fills the chip (1 500 waves of lanes, then a few thousand waves of one query each), both are chains of dependent steps.
      const bool early = aside && split.walk_rounds > 1 && !(split.cut_ticks && split.cut_words);
      const int coop_grid_w = std::max(1, std::min(grid * BVH_BLOCK, split.coop_grid ? int(split.coop_grid) : grid * 2));
      for (uint32_t r = 0; r < split.walk_rounds; ++r) {
        if (early && r >= 1 && aside[r - 1].stream) {
          const AsideStream& as = aside[r - 1];
          hipLaunchKernelGGL((k_walk_order<T>), dim3(1), dim3(1024), 0, st, s0, r - 1u);
          hipEventRecord(as.fork, st);
          hipStreamWaitEvent(as.stream, as.fork, 0);
          BvhSplit s1 = s0;
          s1.coop_range = r;  // (1 + the round that just ended)
          s1.can_suspend = 0u;
          hipLaunchKernelGGL((k_bvh_coop<T>), dim3(coop_grid_w), dim3(64), 0, as.stream, wk, lv, bv, io, q, bp, break_distance2, s1);
          hipEventRecord(as.join, as.stream);
          s0.coop_range = 0x100u + (r - 1u);
          n_early = r;
        }
        wa.round = r;
        wa.k = std::min<uint32_t>(split.walk_k[r], uint32_t(WALK_K));
        wa.budget = split.walk_budget[r];
        wa.last = r + 1 == split.walk_rounds ? 1u : 0u;
        wa.list_out = lists + size_t(r & 1u) * wa.list_stride;
        wa.list_in = lists + size_t((r + 1u) & 1u) * wa.list_stride;  // (= the list_out of round r - 1; not read in round 0)
        hipLaunchKernelGGL((k_bvh_walk<T>), dim3(grid), dim3(BVH_BLOCK), 0, st, wk, lv, bv, io, q, break_distance2, wa);
        hipLaunchKernelGGL((k_tri_leaves<T>), dim3(lgrid), dim3(64), 0, st, wk, lv, bv, io, q, wa);
        hipLaunchKernelGGL((k_bvh_resolve<T>), dim3(std::max(1, std::min(grid, 1024))), dim3(256), 0, st, wk, lv, io, q, s0, wa);
      }
    } else {
      launch_collide_kernel<T>(false, grid, st, wk, lv, bv, io, q, bp, break_distance2, s0, spill);
    }
    // a wave per suspended query, up to what the chip holds (`grid` blocks of BVH_BLOCK queries: `grid * 2` waves left a quarter of the
    // wave slots empty at 100k queries, profiles/r04_h)
    const int coop_grid = std::max(1, std::min(grid * BVH_BLOCK, split.coop_grid ? int(split.coop_grid) : grid * 2));
    if (s0.order && split.walk.recs && split.walk_rounds && !(split.cut_ticks && split.cut_words)) {
      // (what the last round added -- or, without launches beside the rounds, every suspended query -- longest stack first)
      hipLaunchKernelGGL((k_walk_order<T>), dim3(1), dim3(1024), 0, st, s0, n_early ? split.walk_rounds - 1u : 0u);
    } else {
      s0.order = nullptr;
    }
    launch_coop_levels<T, MESH_UNIT_PART>(grid, st, wk, io, s0, int(B_COUNT + 2), [&](const BvhSplit& s) {
      hipLaunchKernelGGL((k_bvh_coop<T>), dim3(coop_grid), dim3(64), 0, st, wk, lv, bv, io, q, bp, break_distance2, s);
    });
    for (uint32_t r = 0; r < n_early; ++r) hipStreamWaitEvent(st, aside[r].join, 0);
    return;
  }
  // the walk in task levels (or unsplit)
  bvh_collide_levels<T, MESH_UNIT_PART>(grid, st, wk, io, bp, split, int(B_COUNT + 2), [&](const BvhSplit& s) {
    launch_collide_kernel<T>(false, grid, st, wk, lv, bv, io, q, bp, break_distance2, s, spill);
  });
}
template <typename T>
void launch_triangle(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q) {
  hipLaunchKernelGGL((k_triangle<T>), dim3(grid), dim3(64), 0, st, wk, lv, io, q);
}
#define HFCL_INST(T)                                                                                                             \
  template void launch_bvh_collide<T>(int, hipStream_t, const Work&, const LibView<T>&, const BvhView<T>&, const IO<T>&, const QParams<T>&, const BvhParams&, T, BvhSplit, BvhSpill, const AsideStream*); \
  template void launch_triangle<T>(int, hipStream_t, const Work&, const LibView<T>&, const IO<T>&, const QParams<T>&);
HFCL_INST(float)
HFCL_INST(double)
#undef HFCL_INST
