// hfcl_mesh_collide.hpp -- what the two collide() objects of the mesh unit share as templates: hfcl_k_bvh.hip (hfcl_k_bvh.o, mesh x mesh
// collide() and triangle pairs) and hfcl_k_bvhc.hip (hfcl_k_bvhc.o, mesh x solid collide()).  Only these two include it;
// hfcl_k_bvhs.hip (hfcl_k_bvhs.o, mesh x solid distance()) shares hfcl_mesh.hpp with them and nothing of this.  Here: the lanes' walk
// with its task levels and their fold-back (k_bvh_collide, k_bvh_level_mark, k_bvh_combine), the lane-group helpers of the waves'
// continuations (k_bvh_coop, k_bvh_shape_coop: each in its object's source), the walk in rounds without its leaves (k_bvh_walk,
// k_walk_order, k_bvh_resolve) and the launch templates of the levels.
//
// The three mesh sources are built under two contraction settings (Makefile: hfcl_k_bvh.o with hipcc's default, hfcl_k_bvhc.o and
// hfcl_k_bvhs.o with -ffp-contract=off), and every template is instantiated by the object that uses it.  A kernel or a non-inlined device
// function instantiated with the same arguments in two of these objects would therefore be built twice, differently, and the two copies
// would collide at the kernel's host stub (a template's stub is one weak symbol for the whole library): which arithmetic a launch then
// runs is the linker's choice.  The forms of a walk write the same bytes (tests/test_options_gpu.py, test_bvh_collide_forms_agree,
// test_gpu_mesh_solid_*_forms_agree) only because each object runs its own copies.  So whatever two objects launch carries the
// launching object's part as a template argument -- each source names its own once, MESH_UNIT_PART = 1 (hfcl_k_bvh.hip), 2
// (hfcl_k_bvhs.hip), 3 (hfcl_k_bvhc.hip), and passes it explicitly: k_bvh_level_mark and k_bvh_combine here, k_bvh_shape_finish in
// hfcl_mesh.hpp -- and what one object launches is told apart by its own arguments (SOLID of k_bvh_collide / k_bvh_walk / k_bvh_resolve:
// hfcl_k_bvh.hip instantiates the plain forms alone, hfcl_k_bvhc.hip the SOLID ones alone; the W0Lds block size of the leaf calls).
// tests/test_mesh_units_cpu.py holds the built objects to it: no kernel's host stub in two of them, and each object's number of kernels.
#pragma once
#include "hfcl_mesh.hpp"

#ifndef HFCL_BVH_PREFETCH
#define HFCL_BVH_PREFETCH 1  // cfg4 100k: 7.5 -> 6.7 ms, 1M: 61.6 -> 67.6 M q/s (profiles/r02_r); touching the sibling as well gave nothing more
#endif
#ifndef HFCL_WPE_BVH_COLLIDE
#define HFCL_WPE_BVH_COLLIDE 2  // two waves per SIMD: the walk waits for its node gathers most of the time (profiles/r02_m)
#endif
// FILT (fp64 only): the separating-axis test runs as an fp32 filter on 64-byte node records (hfcl_bvh.hpp: obb_filter, with
// its error analysis) and the fp64 test of the reference -- on the 128-byte records, with the relative pose rebuilt from the
// query's poses -- only where the filter cannot prove what that test would do: 4 % of the steps on cfg4 (3.9 %: a
// disjoint pair whose value could lower the running bound, i.e. the record lows of the bound; 0.4 %: a quantity within the
// error bound of its threshold).  A lane that needs the fp64 test parks (like a lane waiting for its leaf test) and the wave
// runs it for all parked lanes at once.  Decisions and reported numbers are the fp64 test's throughout; the walk's
// persistent state is the fp32 relative pose (13 registers instead of 24).
// MEASURED SLOWER than the plain fp64 kernel and therefore off by default (HFCL_BVH_FILTER=1 selects it; profiles/r03_b):
// cfg4 100k queries 6.9 against 5.3 ms, 1M queries 53 against 68 M q/s.  The fp32 test is ~1.3x the instructions of the
// fp64 one (bounds, rebuilt third axes) at 1.8x the issue rate, the kernel keeps the registers of its fp64 leaf phase (256:
// two waves per SIMD either way; forced to three it spills 396 B per lane and takes 10.8 ms), and the step is a gather
// round trip in both forms.  The walk ALONE (no leaf tests, no fp64 re-tests) fits 152 registers = three waves per SIMD
// and does 29 G steps/s against the 12 G/s of the full kernel: the headroom is in separating the walk from the fp64
// phases, not in the arithmetic of the test.
#ifndef HFCL_WPE_BVH_FILT
#define HFCL_WPE_BVH_FILT 2
#endif
// The leaf of the SOLID form as a call: inlined (HFCL_SOLID_LEAF_OUTLINE=0), the leaf's GJK over every support function
// shares the register allocation of the walk -- 7 % slower on tools/mesh_solid_bench.py (profiles/r03_i).
#ifndef HFCL_SOLID_LEAF_OUTLINE
#define HFCL_SOLID_LEAF_OUTLINE 1
#endif

// the triangle pair of a mesh x mesh leaf as a call (k_bvh_coop; k_bvh_collide with HFCL_BVH_LEAF_OUTLINE=1)
#ifndef HFCL_BVH_LEAF_OUTLINE
#define HFCL_BVH_LEAF_OUTLINE 0
#endif
template <typename T>
struct TriLeafOut {
  T distance;
  V3<T> p1, p2, n;
};
template <typename T, class PS>
__device__ __noinline__ void tri_leaf_call(const T* v1, const uint32_t* t1, const T* v2, const uint32_t* t2, const decltype(IO<T>::tf1) pose1,
                                           const decltype(IO<T>::tf1) pose2, uint32_t pair, const QParams<T>* qp, const PS ps, TriLeafOut<T>* out) {
  const QParams<T> q = *qp;
  auto vtx = [](const T* v, uint32_t i) { return mk<T>(v[3 * size_t(i)], v[3 * size_t(i) + 1], v[3 * size_t(i) + 2]); };
  TriSupport<T> tri;
  {
    const Pose<T> tf1 = load_pose(pose1, pair);
    tri.p1 = xform(tf1, vtx(v1, t1[0]));
    tri.p2 = xform(tf1, vtx(v1, t1[1]));
    tri.p3 = xform(tf1, vtx(v1, t1[2]));
  }
  {
    const Pose<T> tf2 = load_pose(pose2, pair);
    tri.q1 = xform(tf2, vtx(v2, t2[0]));
    tri.q2 = xform(tf2, vtx(v2, t2[1]));
    tri.q3 = xform(tf2, vtx(v2, t2[2]));
  }
  int gst, git;
  out->distance = tri_tri_distance(tri, q.gjk, q.guess_mode == HFCL_GUESS_CACHED, mk<T>(q.guess[0], q.guess[1], q.guess[2]), out->p1, out->p2,
                                   out->n, gst, git, (V3<T>*)nullptr, ps);
}
#ifndef HFCL_BVH_PARK_MAX
#define HFCL_BVH_PARK_MAX 32  // lanes waiting for a leaf test or an fp64 re-test that end the BV phase of a wave
#endif
// ---------------------------------------------------------------------------------------
// k_bvh_collide: BVHModel<OBBRSS> x BVHModel<OBBRSS> collide().
// Traversal = collisionRecurse (src/traversal/traversal_recurse.cpp:44-85) with the recursion
// flattened into a per-lane LDS stack; children are pushed right-then-left so they pop in the
// reference's order, and the walk ends as soon as num_max_contacts contacts exist (canStop()).
//
// Long traversals are cut into tasks.  Queries differ by two orders of magnitude in length (cfg4: 135 BV tests on
// average, > 2000 for the longest), and with 1.5 queries per resident lane the kernel used to last as long as its longest
// query.  Now a unit of work (level 0: a query; deeper levels: a task = one pending (b1, b2) subtree pair) that has used
// up its step budget -- or whose LDS stack is full -- *suspends*: every entry of its stack becomes a task of the next
// level (in DFS order: top of the stack first), its state so far is parked as a summary, and the lane takes new work.
// The levels run as separate launches; afterwards k_bvh_combine folds the children of every suspended unit back, deepest
// level first, exactly as the sequential walk would have seen them:
//   * the walk's running lower bound is a minimum over all its BV / leaf events: order-free;
//   * the reported witness points are those of the LAST leaf that lowered the bound when it was visited.  Within a task
//     those leaves have decreasing values, so only its last one can also lie below the bound accumulated before the task:
//     a task reports that leaf (cand_val, np1, np2, nn) and its overall minimum (dlb, rec_dist), nothing else;
//   * a contact ends the walk: children after the first one with a contact are ignored (their work was speculative).
// Contact lists (num_max_contacts > 1) need the running count of the whole query and run unsplit.
// ---------------------------------------------------------------------------------------
// SOLID: BVHModel<OBBRSS> x convex solid (bucket B_BVHSHAPE, either operand order) walked by the same machinery, one query
// per lane.  The second "tree" is the solid's fitted OBB (k_shape_obb wrote its products with the mesh pose, ObbQuery, per
// query), so an entry is a node of the mesh, every step splits the mesh node (collisionRecurse with a leaf second node) and
// a leaf is ShapeShapeDistance<TriangleP, S>: closed form or per-lane GJK.  A leaf that needs EPA is a contact on the
// host's word (mesh_shape_lane_request) and ends the unit like any contact; its numbers come later, from
// k_bvh_shape_finish.  The 16-lane group kernel this replaces where the request allows walked the long queries of a
// batch alone (the steps per query have a heavy tail: median 1, mean 60, maximum > 3000 with > 1000 leaf tests on
// tools/mesh_solid_bench.py's scenes) -- here they suspend into tasks like the long mesh x mesh queries.
template <typename T, bool WIDE, bool FILT = false, bool SOLID = false>
__global__ void __launch_bounds__(BVH_BLOCK) __attribute__((amdgpu_waves_per_eu(FILT ? HFCL_WPE_BVH_FILT : HFCL_WPE_BVH_COLLIDE, 8))) k_bvh_collide(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q,
                                                          BvhParams bp, T break_distance2, BvhSplit split, BvhSpill spill) {
  static_assert(!FILT || sizeof(T) == 8, "the fp32 filter stands in front of the fp64 test");
  static_assert(!SOLID || (!WIDE && !FILT), "mesh x solid: 32-bit node ids in the narrow entry, plain tests");
  typedef BvhEntry<WIDE> EN;
  typedef typename EN::E E;
  // the filter form is built for three waves per SIMD: six 128-thread blocks per CU = 20 LDS allocation units (25 600 B) each
  constexpr int STACK = FILT ? (WIDE ? BVH_STACK_FILT / 2 : BVH_STACK_FILT) : EN::STACK, HALF = STACK / 2;
  __shared__ E stack[STACK][BVH_BLOCK];
  __shared__ T w0_slab[W0Lds<T, BVH_BLOCK>::WORDS];  // witness payload of the leaf tests' GJK simplex (hfcl_dev.hpp: W0Lds)
  const W0Lds<T, BVH_BLOCK> leaf_ps{w0_slab + threadIdx.x};
  // this lane's slab of spilled entries (WIDE only)
  E* const slab = WIDE && spill.slab ? reinterpret_cast<E*>(spill.slab) + size_t(blockIdx.x * BVH_BLOCK + threadIdx.x) * spill.cap : nullptr;
  uint32_t nspill = 0;
  const uint32_t level = split.level;
  const uint32_t unit0 = level ? split.ctr[BVH_CTR_LEVEL0 + level - 1] : 0u;  // first task of this level
  const uint32_t cnt = level ? min(split.ctr[BVH_CTR_LEVEL0 + level], split.cap) - min(unit0, split.cap) : wk.counts[SOLID ? B_BVHSHAPE : B_BVH];
  if (cnt == 0u) return;  // (no unit of this kind in the batch / on this level: no wave draws a ticket)
  uint32_t* const ticket = &wk.counts[SOLID ? CTR_SHAPE_TICKET : B_COUNT + 2];
  auto ent_first = [](E e) -> uint32_t { return SOLID ? uint32_t(e) : EN::first(e); };  // SOLID: the entry is the mesh node
  const uint32_t budget = split.budget;  // steps a unit may take before it suspends (0: never)
  const int tid = threadIdx.x, lane = tid & 63;
  const T nanv = Lim<T>::nan();
  // Per-lane unit state.  The lanes of a wave do not advance through the batch in lockstep: a lane whose traversal is
  // over parks its result (`pending`) and, as soon as BVH_REFILL_MIN lanes of the wave are idle, all of them write
  // their records and take the next units from a global ticket counter.
  constexpr int refill_min = BVH_REFILL_MIN;
  bool live = false, pending = false, exhausted = false;  // exhausted is wave-uniform
  uint32_t pair = 0, unit = 0, steps = 0;
  // What a lane keeps in registers across a walk is what the BV tests need: the relative pose and the running bounds.
  // The poses themselves (leaf tests only: ~5 per query) are re-read there, the witness of the bound (p1, p2, normal:
  // updated a handful of times) lives where it will be read -- the query's record, or the task's summary.
  DMesh m1 = {0, 0, 0, 0}, m2 = {0, 0, 0, 0};
  typedef typename std::conditional<FILT, float, T>::type TR;  // precision the walk keeps the relative pose in
  M3<TR> RT_R;
  V3<TR> RT_T;
  float t0mag = 0.f;        // FILT: >= |RT_T|_1 (error bound of the filter)
  // FILT: a lane that needs the fp64 test parks with need_exact = 1 (the pair `pend`, which the filter could not decide)
  // or 2 (the candidate `cand`: a disjoint pair whose value may be the minimum of the bound, known to [cand_lo, cand_hi];
  // its fp64 value is computed only when something is compared with it -- a leaf test, a second candidate it cannot be
  // told apart from, the end of a contact-free walk, a suspension)
  int need_exact = 0;
  bool pend_first = false, has_cand = false;
  E pend = 0, cand = 0;
  float cand_lo = 0.f, cand_hi = 0.f;
  const float marginf = float(q.security_margin), bd2f = float(break_distance2);
  int sp = 0;
  bool overflow = false;
  uint32_t ncontacts = 0;
  T dlb = Lim<T>::max(), rec_dist = Lim<T>::max(), cand_val = Lim<T>::max();
  int fb1 = -1, fb2 = -1;
  bool have_leaf = false;
  uint32_t lb1 = 0, lb2 = 0;
  uint32_t my_parent = 0xFFFFFFFFu, my_order = 0;  // (tasks) where this unit hangs
  // SOLID: RT_R / RT_T hold the ObbQuery's M / V, q_ext its extent; the solid, the operand order, the solver's cached guess
  V3<T> q_ext = mk<T>(T(0), T(0), T(0)), guess = mk<T>(T(1), T(0), T(0));
  uint32_t solid_id = 0;
  bool swapped = false;
  auto witness_store = [&](const V3<T>& p1, const V3<T>& p2, const V3<T>& n) {  // the witness of the bound, in place
    if (level) {
      BvhSum<T>* sm = bvh_sum<T>(split, split.n_queries + unit);
      sm->np1 = p1;
      sm->np2 = p2;
      sm->nn = n;
    } else {
      store_witness(io, pair, p1, p2, n);
    }
  };
  auto write_sum_head = [&](uint32_t slot, uint32_t first_child, uint32_t n_child, uint32_t flags) {  // all but np1 / np2 / nn
    BvhSum<T>* sm = bvh_sum<T>(split, slot);
    sm->contact_order = 0xFFFFFFFFu; sm->parent = my_parent; sm->order = my_order; sm->pad_ = 0;
    sm->dlb = dlb; sm->rec_dist = rec_dist; sm->cand_val = cand_val;
    sm->fb1 = fb1; sm->fb2 = fb2;
    sm->ncontacts = ncontacts; sm->first_child = first_child; sm->n_child = n_child; sm->flags = flags;
  };
  auto flush = [&]() {  // the unit this lane finished: a query's record, or a task's summary (the witness is in place)
    if (level)
      write_sum_head(split.n_queries + unit, 0u, 0u, overflow ? BVH_SUM_OVERFLOW : 0u);
    else {
      store_bvh_record_head(io, pair, rec_dist, ncontacts, fb1, fb2, overflow);
      if constexpr (SOLID) write_guess<T>(io, pair, guess, 0, 0);
    }
  };
  auto moot = [&](uint32_t p, uint32_t o) -> bool { return bvh_moot<T>(split, p, o); };
  // a contact in this task ends the walk of every unit above it at this child's position
  auto report_contact = [&](uint32_t p, uint32_t o) {
    for (int hop = 0; hop < BVH_MAX_LEVELS + 1 && p != 0xFFFFFFFFu; ++hop) {
      BvhSum<T>* ps = bvh_sum<T>(split, p);
      atomicMin(&ps->contact_order, o);
      o = ps->order;
      p = ps->parent;
    }
  };
  // Turn the `n_extra` entries in `extra` (children about to be pushed: first one on top) and the whole stack into tasks
  // of the next level and park this unit.  false: no room in the task table (the unit then simply goes on).
  // SOLID: every entry is EXPANDED ONCE on the way out -- its box is tested here, and its two children (or the bound, if the
  // boxes are disjoint: a child that is already finished) take its place among the tasks.  A suspended stack holds subtrees
  // of geometrically decreasing size (the bottom entry is the sibling of the walk's first step: half the tree), so plain
  // suspension halves the longest chain per level at best; with the expansion it is quartered (profiles/r03_i: mesh x solid
  // 6.2 -> 4.6 ms per 100k sphere queries, nine levels -> six; the same on mesh x mesh stacks LOSES, 4.97 -> 5.28 ms per
  // 100k cfg4 queries: twice the tasks, and a task costs its set-up).
  auto suspend = [&](uint32_t ea, uint32_t eb, int n_extra) -> bool {
    const uint32_t n_ent = uint32_t(sp + n_extra);
    if (WIDE || !split.can_suspend || n_ent == 0) return false;  // (tasks carry 16-bit node ids)
    const bool expand = SOLID && !split.coop;  // (a suspended stack that k_bvh_shape_coop continues stays as it is)
    const uint32_t n_slots = expand ? 2u * n_ent : n_ent;
    const uint32_t first = atomicAdd(&split.ctr[BVH_CTR_TASKS], n_slots);
    if (first + n_slots > split.cap) {  // table full: the slots taken become no-ops for the next level
      for (uint32_t j = first; j < min(first + n_slots, split.cap); ++j) split.tasks[j] = BvhTask{0u, 0u, 0xFFFFFFFFu, 0u};
      steps = 0;  // the unit goes on; it asks again after another budget of steps, not at every step (a full table stays full)
      return false;
    }
    uint32_t my_slot;
    if (level) {
      my_slot = split.n_queries + unit;
    } else {
      my_slot = atomicAdd(&split.ctr[BVH_CTR_SUSPENDED], 1u);  // < n_queries: one per query at most
      split.suspended[my_slot] = pair;
    }
    uint32_t j = first, o = 0;
    auto as_they_are = [&]() {
      if (n_extra > 0) split.tasks[j++] = BvhTask{pair, my_slot, ea, o++};
      if (n_extra > 1) split.tasks[j++] = BvhTask{pair, my_slot, eb, o++};
      for (int k = sp - 1; k >= 0; --k) split.tasks[j++] = BvhTask{pair, my_slot, uint32_t(stack[k][tid]), o++};  // DFS order: top first
    };
    if (SOLID && !expand) {
      as_they_are();
    } else if constexpr (SOLID) {
      ObbQuery<T> oq;
      oq.M = RT_R;
      oq.V = RT_T;
      oq.ext = q_ext;
      for (int k = int(n_ent) - 1; k >= 0; --k) {  // DFS order: the children about to be pushed, then the stack from the top
        const uint32_t e = k >= sp ? (k == int(n_ent) - 1 ? ea : eb) : uint32_t(stack[k][tid]);
        const DNode<T>* const np = bv.nodes + m1.node_off + e;
        const int32_t fc = np->first_child;
        if (fc < 0) {
          split.tasks[j++] = BvhTask{pair, my_slot, e, o++};
          continue;
        }
        const DNode<T> n1 = *np;
        T sq;
        if (obb_disjoint_q(oq, n1, q.security_margin, break_distance2, sq)) {
          // a child that is finished: its summary is the bound (updateDistanceLowerBoundFromBV, folded in at its place)
          BvhSum<T>* sm = bvh_sum<T>(split, split.n_queries + j);
          const T nd = hsqrt(sq);
          sm->dlb = nd;
          sm->rec_dist = nd + q.security_margin;
          sm->cand_val = Lim<T>::max();
          sm->fb1 = sm->fb2 = -1;
          sm->ncontacts = 0; sm->first_child = 0; sm->n_child = 0; sm->flags = 0;
          sm->contact_order = 0xFFFFFFFFu; sm->parent = my_slot; sm->order = o; sm->pad_ = 0;
          split.tasks[j++] = BvhTask{pair, my_slot, 0xFFFFFFFFu, o++};
        } else {
          split.tasks[j++] = BvhTask{pair, my_slot, uint32_t(fc), o++};
          split.tasks[j++] = BvhTask{pair, my_slot, uint32_t(fc) + 1u, o++};
        }
      }
      for (uint32_t u = j; u < first + n_slots; ++u) split.tasks[u] = BvhTask{0u, 0u, 0xFFFFFFFFu, 0u};  // slots not needed
    } else {
      as_they_are();
    }
    write_sum_head(my_slot, first, j - first, BVH_SUM_SUSPENDED);
    if (!level) {  // a query's witness so far sits in its record: the summary needs a copy
      BvhSum<T>* sm = bvh_sum<T>(split, my_slot);
      load_witness(io, pair, sm->np1, sm->np2, sm->nn);
    }
    sp = 0;
    live = false;  // nothing to flush: the summary is written
    return true;
  };
  for (;;) {
    if (WIDE && live && !have_leaf && !need_exact && sp == 0 && nspill > 0) {  // the LDS part ran empty: take spilled entries back
      const uint32_t m = min(nspill, uint32_t(HALF));
      for (uint32_t k = 0; k < m; ++k) stack[k][tid] = slab[nspill - m + k];
      nspill -= m;
      sp = int(m);
    }
    if (FILT && live && !have_leaf && !need_exact && sp == 0 && has_cand) {  // the walk is over: does its bound matter?
      if (ncontacts == 0 && !overflow)
        need_exact = 2;  // a contact-free walk reports its bound: the candidate's value is needed
      else
        has_cand = false;
    }
    if (live && !have_leaf && !need_exact && sp == 0) {  // traversal over
      live = false;
      pending = true;
    }
    const uint64_t live_mask = __ballot(live);
    const int n_live = __popcll(live_mask);
    if (exhausted ? n_live == 0 : 64 - n_live >= refill_min) {
      // ---- refill (wave-uniform decision; live lanes sit it out)
      if (pending) {
        flush();
        pending = false;
      }
      if (exhausted) break;
      const int n_need = 64 - n_live;
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(ticket, uint32_t(n_need));
      base = __builtin_amdgcn_readfirstlane(base);
      if (!live) {
        const uint32_t rank = uint32_t(__popcll(~live_mask & ((uint64_t(1) << lane) - 1)));
        const uint32_t it = base + rank;
        if (it < cnt) {
          E entry = 0u;  // (b1 = 0, b2 = 0)
          bool valid = true;
          if (level) {
            unit = unit0 + it;
            const BvhTask t = split.tasks[unit];
            pair = t.pair;
            entry = t.entry;
            my_parent = t.parent;
            my_order = t.order;
            valid = t.entry != 0xFFFFFFFFu;
            if (valid && moot(my_parent, my_order)) {  // speculative work nobody will read: an empty summary
              valid = false;
              dlb = rec_dist = cand_val = Lim<T>::max();
              ncontacts = 0;
              overflow = false;
              write_sum_head(split.n_queries + unit, 0u, 0u, 0u);
            }
          } else {
            pair = wk.lists[size_t(SOLID ? B_BVHSHAPE : B_BVH) * wk.n + it];
          }
          if constexpr (SOLID) {
            if (valid) {
              const uint32_t id1 = wk.shape1[pair], id2 = wk.shape2[pair];
              swapped = lib.kinds[id1] != uint8_t(K_BVH);  // (shape, BVH): collide(o2, o1) then swapObjects (collision.cpp:93-108)
              solid_id = swapped ? id1 : id2;
              m1 = bv.meshes[lib.shapes[swapped ? id2 : id1].bvh_index];
              const ObbQuery<T> oq = reinterpret_cast<const ObbQuery<T>*>(wk.shape_oq)[pair];
              if (!(oq.ext.x == oq.ext.x)) {  // k_shape_obb: no OBB for this solid (swept-sphere radius, < 4 bound vertices)
                valid = false;
                store_unsupported(io, pair);
              }
              RT_R = oq.M;
              RT_T = oq.V;
              q_ext = oq.ext;
              guess = initial_guess<T>(io, q, pair);
            }
          }
          if (valid) {
            if constexpr (!SOLID) {
            const DShape<T> a = lib.shapes[wk.shape1[pair]], b = lib.shapes[wk.shape2[pair]];
            m1 = bv.meshes[a.bvh_index];
            m2 = bv.meshes[b.bvh_index];
            }
            if constexpr (!SOLID) {
              const Pose<T> tf1 = load_pose(io.tf1, pair), tf2 = load_pose(io.tf2, pair);
              const M3<T> R = tmul(tf1.R, tf2.R);  // traversal_node_setup.h:560-563
              const V3<T> t = tmul(tf1.R, tf2.t - tf1.t);
              RT_R.r0 = mk<TR>(TR(R.r0.x), TR(R.r0.y), TR(R.r0.z));
              RT_R.r1 = mk<TR>(TR(R.r1.x), TR(R.r1.y), TR(R.r1.z));
              RT_R.r2 = mk<TR>(TR(R.r2.x), TR(R.r2.y), TR(R.r2.z));
              RT_T = mk<TR>(TR(t.x), TR(t.y), TR(t.z));
              if (FILT) t0mag = (habs(float(RT_T.x)) + habs(float(RT_T.y)) + habs(float(RT_T.z))) * (1.f + 4.f * OBBF_U);
            }
            stack[0][tid] = entry;
            sp = 1;
            nspill = 0;
            steps = 0;
            overflow = false;
            ncontacts = 0;
            dlb = rec_dist = cand_val = Lim<T>::max();
            witness_store(mk<T>(nanv, nanv, nanv), mk<T>(nanv, nanv, nanv), mk<T>(nanv, nanv, nanv));
            fb1 = fb2 = -1;
            have_leaf = false;
            need_exact = 0;
            has_cand = false;
            live = true;
          }
        }
      }
      if (base + uint32_t(n_need) >= cnt) exhausted = true;
      continue;
    }
    // ---- BV phase: advance every lane that has no leaf test (or fp64 re-test) pending, until half the wave waits for
    // one, nobody can advance, or enough lanes ran out of work to make a refill due
    // what a BV test's outcome does to the walk (the same for the filter's verdict and the fp64 test's):
    auto on_disjoint = [&](T sq) {  // updateDistanceLowerBoundFromBV
      if (!(dlb <= T(0))) {
        const T nd = hsqrt(sq);
        if (nd < dlb) {
          dlb = nd;
          rec_dist = nd + q.security_margin;
        }
      }
    };
    auto on_overlap = [&](bool first, uint32_t b1, uint32_t b2, int32_t fc1, int32_t fc2) {
      E ea, eb;
      if (first) {
        const uint32_t c1 = uint32_t(fc1);
        ea = EN::pack(c1, b2);
        eb = EN::pack(c1 + 1, b2);
      } else {
        const uint32_t c1 = uint32_t(fc2);
        ea = EN::pack(b1, c1);
        eb = EN::pack(b1, c1 + 1);
      }
      if (WIDE && sp + 2 > STACK && slab && nspill + uint32_t(HALF) <= spill.cap) {
        // the LDS stack is full: its lower half (the entries needed last) moves to the lane's slab
        for (int k = 0; k < HALF; ++k) slab[nspill + k] = stack[k][tid];
        nspill += uint32_t(HALF);
        for (int k = HALF; k < sp; ++k) stack[k - HALF][tid] = stack[k][tid];
        sp -= HALF;
      }
      if (sp + 2 > STACK) {
        // the LDS stack is full: the whole stack (and the two children) go on as tasks; only where that is not
        // possible (contact lists, last level, task table full, slab full) the unit is flagged as overflowed
        if (!suspend(uint32_t(ea), uint32_t(eb), 2)) {
          overflow = true;
          sp = 0;
          nspill = 0;
        }
      } else {
        stack[sp++][tid] = eb;  // second child below
        stack[sp++][tid] = ea;  // first child on top
      }
    };
    for (;;) {
      const bool can_bv = live && !have_leaf && !need_exact && sp > 0;
      if (!__any(can_bv)) break;
      if (__popcll(__ballot(have_leaf || need_exact)) >= HFCL_BVH_PARK_MAX) break;
      if (!exhausted && 64 - __popcll(__ballot(live && (have_leaf || need_exact || sp > 0 || nspill > 0))) >= refill_min) break;
      if (can_bv) {
        if (FILT && has_cand && budget && steps >= budget) {
          // about to suspend (step budget): a summary carries an exact bound, so the candidate is resolved first
          need_exact = 2;
          continue;
        }
        if (budget && steps >= budget && suspend(0u, 0u, 0)) continue;
        if (level && (steps & 15u) == 15u && moot(my_parent, my_order)) {  // an earlier sibling ended the walk meanwhile
          sp = 0;
          has_cand = false;
          continue;
        }
        ++steps;
        const E e = stack[--sp][tid];
        const uint32_t b1 = ent_first(e), b2 = SOLID ? 0u : EN::second(e);
        if constexpr (FILT) {
          const DNodeF f1 = bv.fnodes[m1.node_off + b1];
          const DNodeF f2 = bv.fnodes[m2.node_off + b2];
          const bool l1 = f1.first_child < 0, l2 = f2.first_child < 0;
          if (l1 && l2) {
            have_leaf = true;
            lb1 = uint32_t(-(f1.first_child + 1));
            lb2 = uint32_t(-(f2.first_child + 1));
            if (has_cand) need_exact = 2;  // the leaf's distance is compared with the bound: the bound must be exact
          } else {
            const bool first = l2 || (!l1 && ((f1.rank & OBBF_RANK_MASK) > (f2.rank & OBBF_RANK_MASK)));  // firstOverSecond
#if HFCL_BVH_PREFETCH
            const DNodeF* const next = bv.fnodes + (first ? m1.node_off + uint32_t(f1.first_child) : m2.node_off + uint32_t(f2.first_child));
            const int32_t touched = next[0].first_child;
#endif
            float nd_lo, nd_hi;
            // argument order of the reference: overlap(RT.R, RT.T, model2.bv(b2), model1.bv(b1))
            const int verdict = obb_filter(RT_R, RT_T, t0mag, f2, f1, marginf, bd2f, nd_lo, nd_hi);
#if HFCL_BVH_PREFETCH
            asm volatile("" ::"v"(touched));
#endif
            if (verdict == OBBF_OVERLAP) {
              if (sp + 2 > STACK && has_cand && !WIDE) {  // this expansion will suspend the unit: candidate first, then again
                stack[sp++][tid] = e;
                need_exact = 2;
              } else {
                on_overlap(first, b1, b2, f1.first_child, f2.first_child);
              }
            } else if (verdict == OBBF_DISJOINT) {
              if (dlb <= T(0) || T(nd_lo) >= dlb || (has_cand && nd_lo >= cand_hi)) {
                // the value the fp64 test would report cannot lower the bound: nothing changes
              } else if (!has_cand || nd_hi < cand_lo) {
                has_cand = true;  // (a candidate that is certainly above this one is dropped)
                cand = e;
                cand_lo = nd_lo;
                cand_hi = nd_hi;
              } else {  // two candidates that cannot be told apart: the old one is resolved, this pair is looked at again
                stack[sp++][tid] = e;
                need_exact = 2;
              }
            } else {
              need_exact = 1;
              pend = e;
              pend_first = first;
            }
          }
        } else if constexpr (SOLID) {
          const DNode<T>* const np = bv.nodes + m1.node_off + b1;
          const int32_t fc = np->first_child;
          if (fc < 0) {
            have_leaf = true;
            lb1 = uint32_t(-(fc + 1));
          } else {
            const DNode<T> n1 = *np;
#if HFCL_BVH_PREFETCH
            const int32_t touched = np[fc - int32_t(b1)].first_child;  // the node popped next if the boxes overlap
#endif
            ObbQuery<T> oq;
            oq.M = RT_R;
            oq.V = RT_T;
            oq.ext = q_ext;
            T sq;
            const bool disjoint = obb_disjoint_q(oq, n1, q.security_margin, break_distance2, sq);
#if HFCL_BVH_PREFETCH
            asm volatile("" ::"v"(touched));
#endif
            if (disjoint)
              on_disjoint(sq);
            else
              on_overlap(true, b1, 0u, fc, 0);
          }
        } else {
        const DNode<T> n1 = bv.nodes[m1.node_off + b1];
        const DNode<T> n2 = bv.nodes[m2.node_off + b2];
        const bool l1 = n1.first_child < 0, l2 = n2.first_child < 0;
        if (l1 && l2) {
          have_leaf = true;
          lb1 = uint32_t(-(n1.first_child + 1));
          lb2 = uint32_t(-(n2.first_child + 1));
        } else {
          const T sz1 = sqnorm(n1.extent), sz2 = sqnorm(n2.extent);
          const bool first = l2 || (!l1 && (sz1 > sz2));  // firstOverSecond
#if HFCL_BVH_PREFETCH
          // The pair this lane pops next, if the boxes overlap, is (first child of the node that gets split, other node):
          // touch that child's record (one 128-byte line in fp64) before the separating-axis test, so that the gather of
          // the next step finds it on its way up the cache hierarchy instead of starting after the test.
          const DNode<T>* const next = bv.nodes + (first ? m1.node_off + uint32_t(n1.first_child) : m2.node_off + uint32_t(n2.first_child));
          const int32_t touched = next[0].first_child;
#endif
          T sq;
          // argument order of the reference: overlap(RT.R, RT.T, model2.bv(b2), model1.bv(b1))
          const bool disjoint = obb_disjoint(RT_R, RT_T, n2, n1, q.security_margin, break_distance2, sq);
#if HFCL_BVH_PREFETCH
          asm volatile("" ::"v"(touched));
#endif
          if (disjoint)
            on_disjoint(sq);
          else
            on_overlap(first, b1, b2, n1.first_child, n2.first_child);
        }
        }
      }
    }
    // ---- fp64 tests (FILT): pairs the filter could not decide, and candidates whose exact value is needed now
    if constexpr (FILT) {
      if (need_exact) {
        const bool is_cand = need_exact == 2;
        need_exact = 0;
        const E e = is_cand ? cand : pend;
        const uint32_t b1 = EN::first(e), b2 = EN::second(e);
        const DNode<T> n1 = bv.nodes[m1.node_off + b1];
        const DNode<T> n2 = bv.nodes[m2.node_off + b2];
        const Pose<T> tf1 = load_pose(io.tf1, pair), tf2 = load_pose(io.tf2, pair);
        const M3<T> R = tmul(tf1.R, tf2.R);  // traversal_node_setup.h:560-563
        const V3<T> t = tmul(tf1.R, tf2.t - tf1.t);
        T sq;
        const bool disjoint = obb_disjoint(R, t, n2, n1, q.security_margin, break_distance2, sq);
        if (is_cand) {
          has_cand = false;
          on_disjoint(sq);  // (the filter proved "disjoint")
        } else if (disjoint) {
          on_disjoint(sq);
        } else if (sp + 2 > STACK && has_cand && !WIDE) {  // this expansion will suspend the unit: candidate first, then again
          stack[sp++][tid] = e;
          need_exact = 2;
        } else {
          on_overlap(pend_first, b1, b2, n1.first_child, n2.first_child);
        }
      }
    }
    // ---- leaf phase (leafCollides, traversal_node_bvhs.h:184-233)
    if constexpr (SOLID) {
      if (have_leaf) {
        have_leaf = false;
        const uint32_t* t3 = bv.tris + 3 * size_t(m1.tri_off + lb1);
        const T* mv = bv.verts + 3 * size_t(m1.vert_off);
        const uint32_t kind = lib.kinds[solid_id];
        // what the leaf costs in BV tests (the unit of the step budget): a GJK run against the solid, or a closed form
        steps += (kind == uint32_t(K_SPHERE) || kind_is_flat(int(kind))) ? max(split.leaf_cost / 8u, 1u) : split.leaf_cost;
        T distance;
        V3<T> p1, p2, n;
        bool to_epa;
#if HFCL_SOLID_LEAF_OUTLINE
        {
          SolidLeafIn<T> in{mv, t3, lib.shapes, lib.verts, swapped ? io.tf2 : io.tf1, swapped ? io.tf1 : io.tf2,
                            reinterpret_cast<ShapeDeferItem<T>*>(wk.shape_defer), &wk.counts[CTR_SHAPE_DEFER], wk.shape_defer_cap, pair, solid_id, lb1, my_parent, my_order,
                            T(0), -1};
          SolidLeafOut<T> lo;
          to_epa = solid_leaf_call<T>(in, &q, leaf_ps, guess, &lo);
          distance = lo.distance;
          p1 = lo.p1;
          p2 = lo.p2;
          n = lo.n;
          guess = lo.guess;
        }
#else
        {
        auto vtx = [&](uint32_t i) { return mk<T>(mv[3 * size_t(i)], mv[3 * size_t(i) + 1], mv[3 * size_t(i) + 2]); };
        const V3<T> ta = vtx(t3[0]), tb = vtx(t3[1]), tc = vtx(t3[2]);
        LaneSolid<T> solid;
        solid.s = lib.shapes[solid_id];
        solid.v = lib.verts + 3 * size_t(solid.s.vertex_offset);
        auto tfm_of = [&]() { return load_pose(swapped ? io.tf2 : io.tf1, pair); };
        auto tfs_of = [&]() { return load_pose(swapped ? io.tf1 : io.tf2, pair); };
        const MDiff<T> sMt = make_mdiff(tfs_of(), tfm_of());  // Transform3f::inverseTimes: the mesh frame in the solid's frame
        ShapeDeferItem<T> item;
        to_epa = mesh_shape_leaf_lane(ta, tb, tc, sMt, tfm_of, tfs_of, solid.s, solid, swept_radius(solid.s), q, guess, leaf_ps,
                                      distance, p1, p2, n, item);
        if (to_epa) {
          item.seed.pair = pair;
          item.prim = lb1;
          item.parent = my_parent;
          item.order = my_order;
          const uint32_t slot = atomicAdd(&wk.counts[CTR_SHAPE_DEFER], 1u);
          if (slot < wk.shape_defer_cap) reinterpret_cast<ShapeDeferItem<T>*>(wk.shape_defer)[slot] = item;
        }
        }
#endif
        bool contact = to_epa;
        if (!to_epa) {
          const T dtc = distance - q.security_margin;
          if (dtc < dlb) {  // updateDistanceLowerBoundFromLeaf
            dlb = dtc;
            cand_val = dtc;
            rec_dist = distance;
            witness_store(swapped ? p2 : p1, swapped ? p1 : p2, swapped ? -n : n);
          }
          contact = dtc <= q.collision_distance_threshold;
        }
        if (contact) {
          if (ncontacts < bp.num_max_contacts) {
            if (ncontacts == 0) {
              fb1 = swapped ? -1 : int(lb1);
              fb2 = swapped ? int(lb1) : -1;
              if (level) report_contact(my_parent, my_order);
            }
            ++ncontacts;
            if (!to_epa) emit_shape_contact(bp, pair, swapped, int(lb1), distance, p1, p2, n);
          }
          if (to_epa || ncontacts >= bp.num_max_contacts) {  // canStop()
            sp = 0;
            nspill = 0;
          }
        }
      }
    } else
    if (have_leaf) {
      have_leaf = false;
      steps += 8;  // a triangle pair costs about as much as eight BV tests
      const uint32_t* t1 = bv.tris + 3 * size_t(m1.tri_off + lb1);
      const uint32_t* t2 = bv.tris + 3 * size_t(m2.tri_off + lb2);
      const T* v1 = bv.verts + 3 * size_t(m1.vert_off);
      const T* v2 = bv.verts + 3 * size_t(m2.vert_off);
#if HFCL_BVH_LEAF_OUTLINE
      TriLeafOut<T> tlo;
      tri_leaf_call<T>(v1, t1, v2, t2, io.tf1, io.tf2, pair, &q, leaf_ps, &tlo);
      const T distance = tlo.distance;
      const V3<T> p1 = tlo.p1, p2 = tlo.p2, n = tlo.n;
#else
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
      V3<T> p1, p2, n;
      int gst, git;
      const T distance = tri_tri_distance(tri, q.gjk, q.guess_mode == HFCL_GUESS_CACHED,
                                          mk<T>(q.guess[0], q.guess[1], q.guess[2]), p1, p2, n, gst, git, (V3<T>*)nullptr, leaf_ps);
#endif
      const T dtc = distance - q.security_margin;
      if (dtc < dlb) {  // updateDistanceLowerBoundFromLeaf
        dlb = dtc;
        cand_val = dtc;
        rec_dist = distance;
        witness_store(p1, p2, n);
      }
      if (dtc <= q.collision_distance_threshold) {
        if (ncontacts < bp.num_max_contacts) {
          if (ncontacts == 0) {
            fb1 = int(lb1);
            fb2 = int(lb2);
            if (level) report_contact(my_parent, my_order);
          }
          ++ncontacts;
          if (bp.contacts) {
            const uint32_t slot = atomicAdd(bp.contacts_count, 1u);
            if (slot < bp.contacts_cap) {
              hfcl_contact c;
              c.pair = pair;
              c.b1 = int(lb1);
              c.b2 = int(lb2);
              c._pad = 0;
              c.penetration_depth = double(distance);
              c.normal[0] = n.x; c.normal[1] = n.y; c.normal[2] = n.z;
              c.p1[0] = p1.x; c.p1[1] = p1.y; c.p1[2] = p1.z;
              c.p2[0] = p2.x; c.p2[1] = p2.y; c.p2[2] = p2.z;
              bp.contacts[slot] = c;
            }
          }
        }
        if (ncontacts >= bp.num_max_contacts) {  // canStop(): nothing else is visited
          sp = 0;
          nspill = 0;
        }
      }
    }
  }
}

// Between two levels: the tasks made so far are the next level's units; the ticket counter starts over.
template <int PART>
__global__ void k_bvh_level_mark(Work wk, BvhSplit split, int ticket) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    split.ctr[BVH_CTR_LEVEL0 + split.level + 1] = split.ctr[BVH_CTR_TASKS];
    wk.counts[ticket] = 0u;
    if (ticket == CTR_SHAPE_TICKET && split.level == 1) wk.counts[CTR_SHAPE_DEFER_MARK] = min(wk.counts[CTR_SHAPE_DEFER], wk.shape_defer_cap);  // (the first launch of k_bvh_shape_coop is over)
  }
}

// Fold the children of the suspended units of level `split.level` back (the children's own children are folded already).
template <typename T, int PART>
__global__ void __launch_bounds__(256) k_bvh_combine(Work wk, IO<T> io, BvhSplit split) {
  const uint32_t level = split.level;
  const uint32_t unit0 = level ? min(split.ctr[BVH_CTR_LEVEL0 + level - 1], split.cap) : 0u;
  const uint32_t cnt = level ? min(split.ctr[BVH_CTR_LEVEL0 + level], split.cap) - unit0 : split.ctr[BVH_CTR_SUSPENDED];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
    const uint32_t slot = level ? split.n_queries + unit0 + i : i;
    BvhSum<T> s = *bvh_sum<T>(split, slot);
    if (!(s.flags & BVH_SUM_SUSPENDED)) continue;  // (level 0: a suspended query that k_bvh_coop / k_bvh_shape_coop walked to its end)
    if (level && split.tasks[unit0 + i].entry == 0xFFFFFFFFu) continue;
    bool overflow = (s.flags & BVH_SUM_OVERFLOW) != 0;
    for (uint32_t j = 0; j < s.n_child; ++j) {
      const BvhSum<T> c = *bvh_sum<T>(split, split.n_queries + s.first_child + j);
      overflow = overflow || (c.flags & BVH_SUM_OVERFLOW);
      if (c.cand_val < s.dlb) {  // the child's last bound-lowering leaf also lowers the bound as it stood before the child
        s.cand_val = c.cand_val;
        s.np1 = c.np1;
        s.np2 = c.np2;
        s.nn = c.nn;
      }
      if (c.dlb < s.dlb) {
        s.dlb = c.dlb;
        s.rec_dist = c.rec_dist;
      }
      if (c.ncontacts) {  // the walk ended here
        s.ncontacts = c.ncontacts;
        s.fb1 = c.fb1;
        s.fb2 = c.fb2;
        break;
      }
    }
    if (level) {
      s.flags = overflow ? BVH_SUM_OVERFLOW : 0u;
      s.n_child = 0;
      *bvh_sum<T>(split, slot) = s;
    } else {
      PairOut<T> o;
      o.distance = s.rec_dist;
      o.normal = s.nn;
      o.p1 = s.np1;
      o.p2 = s.np2;
      o.gjk_status = GJK_DID_NOT_RUN;
      o.epa_status = EPA_DID_NOT_RUN;
      o.gjk_iters = o.epa_iters = 0;
      store_bvh_record(io, split.suspended[i], o, s.ncontacts, s.fb1, s.fb2, overflow);
    }
  }
}

// A walk's state is the same in every lane of its group; when the group is the wave (W == 64) it belongs in SGPRs, not in 64 copies
// that stay live across the leaf's GJK (k_bvh_shape_coop<double>: 624 B/lane of scratch before, profiles/r05_f): wave_uniform() says so
// to the compiler (v_readfirstlane), a no-op for narrower groups.
template <int W>
__device__ __forceinline__ uint32_t wave_uniform(uint32_t x) {
  if constexpr (W == 64) return uint32_t(__builtin_amdgcn_readfirstlane(int(x)));
  return x;
}
template <int W>
__device__ __forceinline__ int wave_uniform(int x) {
  if constexpr (W == 64) return __builtin_amdgcn_readfirstlane(x);
  return x;
}
template <int W>
__device__ __forceinline__ float wave_uniform(float x) {
  if constexpr (W == 64) return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
  return x;
}
template <int W>
__device__ __forceinline__ double wave_uniform(double x) {
  if constexpr (W == 64) return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
  return x;
}
template <int W, typename T>
__device__ __forceinline__ V3<T> wave_uniform(const V3<T>& v) {
  return mk<T>(wave_uniform<W>(v.x), wave_uniform<W>(v.y), wave_uniform<W>(v.z));
}
template <typename T, int W>
__device__ __forceinline__ T group_min_excl_scan(T v, int lig, T identity) {  // exclusive prefix minimum over the lanes of a group
#pragma unroll
  for (int d = 1; d < W; d <<= 1) {
    const T o = __shfl_up(v, d, W);
    if (lig >= d) v = o < v ? o : v;
  }
  const T up = __shfl_up(v, 1, W);
  return lig == 0 ? identity : up;
}
template <typename T, int W>
__device__ __forceinline__ T group_min_all(T v) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) {
    const T o = __shfl_xor(v, d, W);
    v = o < v ? o : v;
  }
  return v;
}
// COOP_W lanes per query (a wave walks 64 / COOP_W queries side by side, each with its own stack).  Narrower groups were
// expected to pay -- the triangles that can be visited in one trip rarely come 64 in a row -- and LOSE: the kernel's time
// is that of its longest walks, which need more trips the narrower the window (100k ellipsoid queries: 16.5 / 12 / 9.8 /
// 7.7 ms at 8 / 16 / 32 / 64 lanes, profiles/r03_i).
#ifndef HFCL_COOP_W
#define HFCL_COOP_W 64
#endif
constexpr int COOP_W = HFCL_COOP_W;
#ifndef HFCL_COOP_CAP
#define HFCL_COOP_CAP 448
#endif
constexpr int COOP_CAP = HFCL_COOP_CAP, COOP_SLACK = 64;  // entries of a query's stack: a full stack narrows the window down to plain DFS, which needs the tree's depth more
// What is known about a stack entry travels with it (two bits of the entry word + a value): a box found disjoint keeps its
// bound, a triangle its distance -- its result does not depend on the walk's state (the leaf solver starts from the
// request's guess).  A trip with a triangle in it costs a GJK run whatever the number of lanes that have one, so triangles
// are EVALUATED when HFCL_COOP_LEAF_BATCH lanes of the window hold an unevaluated one or the window has no box left to
// split, wherever they stand -- and VISITED (applied to the walk's state) later, when everything in front of them is done.
// 100k queries per kind, batch 16 / 32 / 64: ellipsoid 7.1 / 6.2 / 5.5 ms, convex32 5.3 / 4.5 / 3.9, cylinder 3.6 / 3.2 / 2.7
// (evaluated where they are visited: 8.1 / 6.2 / 3.8; evaluating whenever the TOP entry is an unevaluated triangle, the first
// form of this idea, gained nothing: nearly every trip then has one) -- profiles/r03_k.
#ifndef HFCL_COOP_LEAF_BATCH
#define HFCL_COOP_LEAF_BATCH 64
#endif
constexpr uint32_t COOP_NODE = 0x3FFFFFFFu, COOP_DISJOINT = 1u << 30, COOP_LEAF = 2u << 30, COOP_LEAF_EPA = 3u << 30;
// HFCL_COOP_PROF (variant builds only, tools/build_variant.sh ... k_bvh -DHFCL_COOP_PROF): how long the walks of k_bvh_shape_coop /
// k_bvh_coop and their waves live, in clock ticks -- [0] longest walk, [1] sum over the walks, [2] walks, [3] longest wave, [4] sum over
// the waves that had a walk, [5] their number, [6] walks cut -- read back by tools/coop_prof.py through hfcl_debug_coop_prof
#ifdef HFCL_COOP_PROF
__device__ unsigned long long coop_prof[32];
#define COOP_WALK_END(first_lane, t_begin)                                                         \
  do {                                                                                             \
    if (first_lane) {                                                                              \
      const unsigned long long dt_ = __builtin_readcyclecounter() - (t_begin);                     \
      atomicMax(&coop_prof[0], dt_);                                                               \
      atomicAdd(&coop_prof[1], dt_);                                                               \
      atomicAdd(&coop_prof[2], 1ull);                                                              \
    }                                                                                              \
  } while (0)
#define COOP_WAVE_END(t_begin, n_walks)                                                            \
  do {                                                                                             \
    if (threadIdx.x == 0 && (n_walks) > 0) {                                                       \
      const unsigned long long dt_ = __builtin_readcyclecounter() - (t_begin);                     \
      atomicMax(&coop_prof[3], dt_);                                                               \
      atomicAdd(&coop_prof[4], dt_);                                                               \
      atomicAdd(&coop_prof[5], 1ull);                                                              \
    }                                                                                              \
  } while (0)
#define COOP_CUT_COUNT(first_lane)                      \
  do {                                                  \
    if (first_lane) atomicAdd(&coop_prof[6], 1ull);     \
  } while (0)
extern "C" int hfcl_debug_coop_prof(unsigned long long* out16, int reset) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(coop_prof), sizeof(coop_prof)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(coop_prof), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#define COOP_PROF_DECL unsigned long long pf_[18] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, pt_ = 0
#define COOP_PROF_T0 (pt_ = __builtin_readcyclecounter())
#define COOP_PROF_ADD(k, x) (pf_[k] += (unsigned long long)(x))
#define COOP_PROF_DT(k) (pf_[k] += __builtin_readcyclecounter() - pt_)
#define COOP_PROF_FLUSH                                                 \
  do {                                                                  \
    if (threadIdx.x == 0)                                               \
      for (int k_ = 0; k_ < 18; ++k_) atomicAdd(&coop_prof[7 + k_], pf_[k_]); \
  } while (0)
#else
#define COOP_WALK_END(first_lane, t_begin)
#define COOP_WAVE_END(t_begin, n_walks)
#define COOP_CUT_COUNT(first_lane)
#define COOP_PROF_DECL
#define COOP_PROF_T0
#define COOP_PROF_ADD(k, x)
#define COOP_PROF_DT(k)
#define COOP_PROF_FLUSH
#endif
// Cutting a long walk (BvhSplit::cut_ticks).  A batch of 100 000 queries used to end with one wave on its longest walk (mesh x solid:
// 1.7 of the kernel's 2.9 ms, the waves busy 54 % of the time; mesh x mesh: 79 %; profiles/r04_j).  A walk that has had its time is
// therefore cut: its stack (DFS order, top first) goes to BvhSplit::cut_words / cut_vals as it is -- tags and values included -- in
// chunks of COOP_CHUNK entries, each chunk a BvhTask of the next launch of the same kernel, whose unit starts from those entries with an
// empty state and ends with a summary (BvhSum) instead of a record; the cut walk's own state is the summary its chunks hang under, and
// k_bvh_combine folds them back in DFS order exactly as it folds k_bvh_collide's task levels (bound: a minimum; witness: the last
// triangle of a chunk that lowered the chunk's own bound, if it also lies below the bound as it stood before the chunk; a contact ends
// the fold).  A chunk can be cut again (two more launches); where it is cut never changes a record, only when its parts are walked.
// What a lane group draws from the launch's ticket: a suspended query (level 0) or a chunk of a cut walk.
struct CoopUnit {
  bool take;       // there is a unit to walk (not: the ticket ran out, a slot of a table that was full, a chunk behind a contact)
  bool exhausted;  // the ticket has run past the launch's units
  uint32_t index;  // of the unit among the launch's units
  uint32_t pair, parent, order;  // the query; (chunks) the summary slot of the walk it was cut from and its place among that walk's chunks
  uint32_t first, count;         // chunks: its entries are cut_words / cut_vals [first, first + count)
};
template <typename T, int W>
__device__ __forceinline__ CoopUnit coop_draw(const BvhSplit& split, uint32_t* ticket, uint32_t level, uint32_t unit0, uint32_t n_units, int lig, int grp) {
  CoopUnit u = {false, false, 0u, 0u, 0xFFFFFFFFu, 0u, 0u, 0u};
  uint32_t qi = 0;
  if (lig == 0) qi = atomicAdd(ticket, 1u);
  qi = uint32_t(__shfl(int(qi), grp * W));
  u.index = qi;
  u.exhausted = qi >= n_units;
  if (u.exhausted) return u;
  if (!level) {  // (unit0: where this launch's part of the suspended list starts, BvhSplit::coop_range)
    u.index = split.order ? split.order[unit0 + qi] : unit0 + qi;
    u.pair = split.suspended[u.index];
    u.take = true;
    return u;
  }
  const BvhTask task = split.tasks[unit0 + qi];
  if (task.entry == 0xFFFFFFFFu) return u;  // (a slot of a table that was full)
  if (bvh_moot<T>(split, task.parent, task.order & 0xFFFFu)) {  // it stands behind a contact: nobody reads its summary
    if (lig == 0) bvh_sum<T>(split, split.n_queries + unit0 + qi)->flags = 0u;
    return u;
  }
  u.pair = task.pair;
  u.parent = task.parent;
  u.order = task.order & 0xFFFFu;
  u.first = task.entry;
  u.count = task.order >> 16;
  u.take = true;
  return u;
}
// a contact in a chunk ends the walk of every unit above it at that chunk's position (k_bvh_collide: report_contact)
template <typename T>
__device__ __forceinline__ void coop_report_contact(const BvhSplit& split, uint32_t p, uint32_t o) {
  for (int hop = 0; hop < BVH_MAX_LEVELS + 1 && p != 0xFFFFFFFFu; ++hop) {
    BvhSum<T>* ps = bvh_sum<T>(split, p);
    atomicMin(&ps->contact_order, o);
    o = ps->order;
    p = ps->parent;
  }
}
template <typename T>
__device__ __forceinline__ void coop_write_sum(const BvhSplit& split, uint32_t slot, T dlb, T rec_dist, T cand_val, const V3<T>& np1, const V3<T>& np2,
                                               const V3<T>& nn, int fb1, int fb2, uint32_t ncontacts, uint32_t first_child, uint32_t n_child,
                                               uint32_t flags, uint32_t parent, uint32_t order) {
  BvhSum<T>* sm = bvh_sum<T>(split, slot);
  sm->dlb = dlb; sm->rec_dist = rec_dist; sm->cand_val = cand_val;
  sm->np1 = np1; sm->np2 = np2; sm->nn = nn;
  sm->fb1 = fb1; sm->fb2 = fb2;
  sm->ncontacts = ncontacts; sm->first_child = first_child; sm->n_child = n_child; sm->flags = flags;
  sm->contact_order = 0xFFFFFFFFu; sm->parent = parent; sm->order = order; sm->pad_ = 0;
}
// The cut itself, by the lanes of the unit's group: the stack (sp entries, top first; `value`: what is known about them, or nullptr) to
// cut_words / cut_vals in chunks of COOP_CHUNK, a BvhTask per chunk, the unit's state as the summary they hang under.  false: the tables
// have no room (the slots taken are no-ops): the walk goes on.
template <typename T, int W>
__device__ __forceinline__ bool coop_cut(const BvhSplit& split, uint32_t my_slot, uint32_t pair, uint32_t my_parent, uint32_t my_order, const uint32_t* stack,
                                         const T* value, int sp, int lig, T dlb, T rec_dist, T cand_val, const V3<T>& np1, const V3<T>& np2, const V3<T>& nn,
                                         bool overflow) {
  const uint32_t n_ent = uint32_t(sp), n_chunks = (n_ent + COOP_CHUNK - 1u) / COOP_CHUNK;
  uint32_t first_task = 0, first_word = 0;
  if (lig == 0) {
    first_task = atomicAdd(&split.ctr[BVH_CTR_TASKS], n_chunks);
    first_word = atomicAdd(&split.ctr[BVH_CTR_CUT], n_ent);
  }
  first_task = uint32_t(__shfl(int(first_task), 0, W));
  first_word = uint32_t(__shfl(int(first_word), 0, W));
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the stack was written back by the lanes of this trip)
  __builtin_amdgcn_wave_barrier();
  if (first_task + n_chunks > min(split.cap, split.cut_task_cap) || first_word + n_ent > split.cut_cap) {
    for (uint32_t c = first_task + uint32_t(lig); c < min(first_task + n_chunks, split.cap); c += uint32_t(W)) split.tasks[c] = BvhTask{0u, 0u, 0xFFFFFFFFu, 0u};
    return false;
  }
  T* const cut_vals = reinterpret_cast<T*>(split.cut_vals);
  for (uint32_t k = uint32_t(lig); k < n_ent; k += uint32_t(W)) {
    split.cut_words[first_word + k] = stack[sp - 1 - int(k)];
    if (value) cut_vals[first_word + k] = value[sp - 1 - int(k)];
  }
  for (uint32_t c = uint32_t(lig); c < n_chunks; c += uint32_t(W))
    split.tasks[first_task + c] = BvhTask{pair, my_slot, first_word + c * COOP_CHUNK, c | (min(uint32_t(COOP_CHUNK), n_ent - c * COOP_CHUNK) << 16)};
  if (lig == 0)
    coop_write_sum<T>(split, my_slot, dlb, rec_dist, cand_val, np1, np2, nn, -1, -1, 0u, first_task, n_chunks,
                      BVH_SUM_SUSPENDED | (overflow ? BVH_SUM_OVERFLOW : 0u), my_parent, my_order);
  return true;
}

// ---------------------------------------------------------------------------------------
// Mesh x mesh collide() in rounds of three kernels (hfcl_dev.hpp: WalkRec): the walk without its leaves, the leaves without a walk, the
// replay of each query's events in the reference's order.
// ---------------------------------------------------------------------------------------
// the lanes of `active` each need `count` consecutive slots behind *counter: one atomic per wave, the lane's first slot back
__device__ __forceinline__ uint32_t wave_reserve(uint32_t* counter, uint32_t count, bool active) {
  const int lane = threadIdx.x & 63;
  uint32_t incl = active ? count : 0u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = uint32_t(__shfl_up(int(incl), d));
    if (lane >= d) incl += o;
  }
  const uint32_t total = uint32_t(__shfl(int(incl), 63));
  uint32_t base = 0;
  if (lane == 0 && total) base = atomicAdd(counter, total);
  base = uint32_t(__builtin_amdgcn_readfirstlane(int(base)));
  return base + incl - (active ? count : 0u);
}
// the distance k_shape_leaves files for a leaf that needs EPA (no leaf is that far inside anything)
template <typename T> __device__ __forceinline__ T walk_leaf_epa() { return -Lim<T>::max(); }
#ifndef HFCL_WPE_BVH_WALK
#define HFCL_WPE_BVH_WALK 2
#endif
#ifndef HFCL_WALK_NODE_CACHE
#define HFCL_WALK_NODE_CACHE 1
#endif
// k_bvh_walk: collisionRecurse (src/traversal/traversal_recurse.cpp:44-85) with the triangle pairs LISTED instead of tested, one query
// per lane, lanes refilled from a ticket as in k_bvh_collide.  A disjoint box pair only ever enters the walk's state through a
// minimum (updateDistanceLowerBoundFromBV), so the boxes between two leaves leave one number: the smallest bound among them.
// SOLID (mesh x solid, its own instantiation in its own object, hfcl_k_bvhc.hip): one tree -- the entry is the mesh node, the other box is the
// solid's (k_shape_obb's ObbQuery, kept where the mesh x mesh walk keeps the relative pose), a leaf is a triangle against the solid.
template <typename T, bool SOLID = false>
__global__ void __launch_bounds__(BVH_BLOCK) __attribute__((amdgpu_waves_per_eu(HFCL_WPE_BVH_WALK, 8)))
k_bvh_walk(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q, T break_distance2, WalkArgs wa) {
  typedef BvhEntry<false> EN;
  constexpr int STACK = BVH_STACK_WALK;
  __shared__ uint32_t stack[STACK][BVH_BLOCK];
  WalkRec<T>* const recs = reinterpret_cast<WalkRec<T>*>(wa.recs);
  uint32_t* const c = wa.ctr + 8 * wa.round;
  const uint32_t cnt = wa.round ? wa.ctr[8 * (wa.round - 1) + 2] : wk.counts[SOLID ? B_BVHSHAPE : B_BVH];
  if (cnt == 0u) return;  // (a batch without mesh x mesh pairs: not one ticket drawn -- 1 500 same-address atomics are 30 us)
  const int tid = threadIdx.x, lane = tid & 63;
  V3<T> q_ext = mk<T>(T(0), T(0), T(0));  // SOLID: RT_R / RT_T hold the ObbQuery's M / V, q_ext its extent
  const T big = Lim<T>::max(), nanv = Lim<T>::nan();
  bool live = false, pending = false, exhausted = false;  // exhausted is wave-uniform
  uint32_t ri = 0, steps = 0, n_leaf = 0, flags = 0, noff1 = 0, noff2 = 0;
  int sp = 0;
  M3<T> RT_R;
  V3<T> RT_T = mk<T>(T(0), T(0), T(0));
  RT_R.r0 = RT_R.r1 = RT_R.r2 = RT_T;
  T pre_cur = big;
#if HFCL_WALK_NODE_CACHE
  DNode<T> n1, n2;
  n1.first_child = n2.first_child = 0;
  n1.axes = n2.axes = RT_R;
  n1.To = n2.To = n1.extent = n2.extent = RT_T;
  uint32_t id1 = 0xFFFFFFFFu, id2 = 0xFFFFFFFFu;
#endif
  for (;;) {
    if (live && (sp == 0 || n_leaf >= wa.k || flags != 0u)) {  // this round is over for the lane's query
      if (sp == 0) flags |= WALK_OVER;
      live = false;
      pending = true;
    }
    const uint64_t live_mask = __ballot(live);
    const int n_live = __popcll(live_mask);
    if (exhausted ? n_live == 0 : 64 - n_live >= BVH_REFILL_MIN) {
      // ---- the parked queries' records and their items (one reservation per wave), then new queries from the ticket
      if (__ballot(pending)) {
        WalkRec<T>* const r = recs + ri;
        const uint32_t first = wave_reserve(&c[1], n_leaf, pending);
        if (pending) {
          const bool fits = first + n_leaf <= wa.item_cap;  // (the host sizes the list for WALK_K items per query: always)
          r->sp = uint32_t(sp);
          r->n_leaf = fits ? n_leaf : 0u;
          r->flags = fits ? flags : (flags | WALK_LOST);
          r->first_item = first;
          r->pre[n_leaf] = pre_cur;
          for (int k = 0; k < sp; ++k) r->stack[k] = stack[k][tid];
          if (fits)
            for (uint32_t s2 = 0; s2 < n_leaf; ++s2) wa.items[first + s2] = ri | (s2 << 28);
          pending = false;
        }
      }
      if (exhausted) break;
      const int n_need = 64 - n_live;
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&c[0], uint32_t(n_need));
      base = uint32_t(__builtin_amdgcn_readfirstlane(int(base)));
      if (!live) {
        const uint32_t it = base + uint32_t(__popcll(~live_mask & ((uint64_t(1) << lane) - 1)));
        if (it < cnt) {
          uint32_t pair;
          if (wa.round) {
            ri = wa.list_in[it];
            const WalkRec<T>* const r = recs + ri;
            pair = r->pair;
            sp = int(r->sp);
            for (int k = 0; k < sp; ++k) stack[k][tid] = r->stack[k];
          } else {
            ri = it;
            pair = wk.lists[size_t(SOLID ? B_BVHSHAPE : B_BVH) * wk.n + it];
            WalkRec<T>* const r = recs + ri;
            r->pair = pair;
            r->dlb = r->rec_dist = r->cand_val = big;
            store_witness(io, pair, mk<T>(nanv, nanv, nanv), mk<T>(nanv, nanv, nanv), mk<T>(nanv, nanv, nanv));
            stack[0][tid] = 0u;  // (b1 = 0, b2 = 0)
            sp = 1;
          }
          bool valid = true;
          if constexpr (SOLID) {
            const uint32_t sid1 = wk.shape1[pair], sid2 = wk.shape2[pair];
            const bool swapped = lib.kinds[sid1] != uint8_t(K_BVH);  // (shape, BVH): collide(o2, o1) then swapObjects (collision.cpp:93-108)
            noff1 = bv.meshes[lib.shapes[swapped ? sid2 : sid1].bvh_index].node_off;
            const ObbQuery<T> oq = reinterpret_cast<const ObbQuery<T>*>(wk.shape_oq)[pair];
            if (!(oq.ext.x == oq.ext.x)) {  // k_shape_obb: no OBB for this solid (k_bvh_collide's SOLID form flags the pair the same way)
              valid = false;
              store_unsupported(io, pair);
              WalkRec<T>* const r = recs + ri;
              r->sp = 0u;
              r->n_leaf = 0u;
              r->flags = WALK_VOID;
              r->first_item = 0u;
              sp = 0;
            }
            RT_R = oq.M;
            RT_T = oq.V;
            q_ext = oq.ext;
          } else {
          noff1 = bv.meshes[lib.shapes[wk.shape1[pair]].bvh_index].node_off;
          noff2 = bv.meshes[lib.shapes[wk.shape2[pair]].bvh_index].node_off;
          const Pose<T> tf1 = load_pose(io.tf1, pair), tf2 = load_pose(io.tf2, pair);
          RT_R = tmul(tf1.R, tf2.R);  // traversal_node_setup.h:560-563
          RT_T = tmul(tf1.R, tf2.t - tf1.t);
          }
          steps = 0;
          n_leaf = 0;
          flags = 0;
          pre_cur = big;
#if HFCL_WALK_NODE_CACHE
          id1 = id2 = 0xFFFFFFFFu;
#endif
          live = valid;
        }
      }
      if (base + uint32_t(n_need) >= cnt) exhausted = true;
      continue;
    }
    for (;;) {
      const bool can = live && sp > 0 && n_leaf < wa.k && flags == 0u;
      const uint64_t can_mask = __ballot(can);
      if (!can_mask) break;
      if (!exhausted && 64 - __popcll(can_mask) >= BVH_REFILL_MIN) break;
      if (!can) continue;
      if (wa.budget && steps >= wa.budget) {
        flags = WALK_BUDGET;
        continue;
      }
      ++steps;
      const uint32_t e = stack[--sp][tid];
      if constexpr (SOLID) {
        const DNode<T>* const np = bv.nodes + noff1 + e;
        const int32_t fc = np->first_child;
        if (fc < 0) {
          WalkRec<T>* const r = recs + ri;
          r->leaf1[n_leaf] = uint32_t(-(fc + 1));
          r->pre[n_leaf] = pre_cur;
          pre_cur = big;
          ++n_leaf;
          continue;
        }
        const DNode<T> nd1 = *np;
#if HFCL_BVH_PREFETCH
        const int32_t touched = np[fc - int32_t(e)].first_child;  // the node popped next if the boxes overlap
#endif
        ObbQuery<T> oq;
        oq.M = RT_R;
        oq.V = RT_T;
        oq.ext = q_ext;
        T sq;
        const bool disjoint = obb_disjoint_q(oq, nd1, q.security_margin, break_distance2, sq);
#if HFCL_BVH_PREFETCH
        asm volatile("" ::"v"(touched));
#endif
        if (disjoint) {
          const T nd = hsqrt(sq);
          if (nd < pre_cur) pre_cur = nd;
        } else if (sp + 2 > STACK) {
          stack[sp++][tid] = e;  // (a tree deeper than the stack: the rest of the walk is k_bvh_shape_coop's)
          flags = WALK_BUDGET;
        } else {
          stack[sp++][tid] = uint32_t(fc) + 1u;  // second child below
          stack[sp++][tid] = uint32_t(fc);       // first child on top
        }
        continue;
      }
      const uint32_t b1 = EN::first(e), b2 = EN::second(e);
#if HFCL_WALK_NODE_CACHE
      // the pair popped behind a box test shares a node with the pair tested (its child pair or its sibling): that record stays in registers
      if (b1 != id1) {
        n1 = bv.nodes[noff1 + b1];
        id1 = b1;
      }
      if (b2 != id2) {
        n2 = bv.nodes[noff2 + b2];
        id2 = b2;
      }
#else
      const DNode<T> n1 = bv.nodes[noff1 + b1];
      const DNode<T> n2 = bv.nodes[noff2 + b2];
#endif
      const bool l1 = n1.first_child < 0, l2 = n2.first_child < 0;
      if (l1 && l2) {
        WalkRec<T>* const r = recs + ri;
        r->leaf1[n_leaf] = uint32_t(-(n1.first_child + 1));
        r->leaf2[n_leaf] = uint32_t(-(n2.first_child + 1));
        r->pre[n_leaf] = pre_cur;
        pre_cur = big;
        ++n_leaf;
        continue;
      }
      const T sz1 = sqnorm(n1.extent), sz2 = sqnorm(n2.extent);
      const bool first = l2 || (!l1 && (sz1 > sz2));  // firstOverSecond
#if HFCL_BVH_PREFETCH
      const DNode<T>* const next = bv.nodes + (first ? noff1 + uint32_t(n1.first_child) : noff2 + uint32_t(n2.first_child));
      const int32_t touched = next[0].first_child;  // (k_bvh_collide: the record of the pair popped next, on its way up the caches)
#endif
      T sq;
      // argument order of the reference: overlap(RT.R, RT.T, model2.bv(b2), model1.bv(b1))
      const bool disjoint = obb_disjoint(RT_R, RT_T, n2, n1, q.security_margin, break_distance2, sq);
#if HFCL_BVH_PREFETCH
      asm volatile("" ::"v"(touched));
#endif
      if (disjoint) {
        const T nd = hsqrt(sq);
        if (nd < pre_cur) pre_cur = nd;
      } else if (sp + 2 > STACK) {
        stack[sp++][tid] = e;  // no room for its children: the pair goes back, the rest of the walk is k_bvh_coop's
        flags = WALK_BUDGET;
      } else {
        uint32_t ea, eb;
        if (first) {
          const uint32_t c1 = uint32_t(n1.first_child);
          ea = EN::pack(c1, b2);
          eb = EN::pack(c1 + 1, b2);
        } else {
          const uint32_t c1 = uint32_t(n2.first_child);
          ea = EN::pack(b1, c1);
          eb = EN::pack(b1, c1 + 1);
        }
        stack[sp++][tid] = eb;  // second child below
        stack[sp++][tid] = ea;  // first child on top
      }
    }
  }
}

// The suspended queries as round `round` left them (the launch of k_bvh_coop that runs beside the later rounds continues those this round
// added), and the order its waves draw them in: by the stack entries a query still holds, most first (BvhSplit::order; counting sort by
// one block).  10 000 walks of 80 us on 2 048 wave slots are 0.4 ms of work; drawn as they were suspended the launch took 0.85.
template <typename T>
__global__ void __launch_bounds__(1024) k_walk_order(BvhSplit split, uint32_t round) {
  __shared__ uint32_t hist[64], base[64];
  const uint32_t hi = min(split.ctr[BVH_CTR_SUSPENDED], split.n_queries);
  const uint32_t lo = round ? min(split.walk.ctr[8u * (round - 1u) + WALK_CTR_SNAP], hi) : 0u;
  if (!split.order) {  // (option bvh_walk_order = 0: the snapshot alone)
    if (threadIdx.x == 0) split.walk.ctr[8u * round + WALK_CTR_SNAP] = hi;
    return;
  }
  if (threadIdx.x < 64) hist[threadIdx.x] = 0u;
  __syncthreads();
  auto key = [&](uint32_t slot) -> uint32_t { return 63u - min(bvh_sum<T>(split, slot)->n_child, 63u); };  // (most entries: bucket 0)
  for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) atomicAdd(&hist[key(i)], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = lo;
    for (int b = 0; b < 64; ++b) {
      base[b] = run;
      run += hist[b];
    }
    split.walk.ctr[8u * round + WALK_CTR_SNAP] = hi;
  }
  __syncthreads();
  for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) split.order[atomicAdd(&base[key(i)], 1u)] = i;
}

// k_bvh_resolve: a query's events of this round in the reference's order -- the boxes in front of a leaf (their smallest bound:
// updateDistanceLowerBoundFromBV), the leaf (updateDistanceLowerBoundFromLeaf, the witness of the last one that lowered the bound, the
// contact that ends the walk: whatever the walk listed behind it is void) -- and where the query goes from here: its record, the next
// round, or k_bvh_coop (a suspended query with its stack as tasks, exactly what k_bvh_collide's suspension leaves).
// SOLID: the leaf is a triangle against the solid (fb1 / fb2 and the witness in the caller's operand order: collision.cpp:93-108), a leaf that
// needs EPA ends the walk as a contact whose numbers k_bvh_shape_finish writes: it goes on the redo list (k_shape_leaves, redo = 1).
template <typename T, bool SOLID = false>
__global__ void __launch_bounds__(256) k_bvh_resolve(Work wk, LibView<T> lib, IO<T> io, QParams<T> q, BvhSplit split, WalkArgs wa) {
  WalkRec<T>* const recs = reinterpret_cast<WalkRec<T>*>(wa.recs);
  const TriLeafOut<T>* const res = reinterpret_cast<const TriLeafOut<T>*>(wa.res);
  uint32_t* const c = wa.ctr + 8 * wa.round;
  const uint32_t cnt = wa.round ? wa.ctr[8 * (wa.round - 1) + 2] : wk.counts[SOLID ? B_BVHSHAPE : B_BVH];
  for (uint32_t base = blockIdx.x * blockDim.x; base < cnt; base += gridDim.x * blockDim.x) {
    const uint32_t it = base + threadIdx.x;
    const bool valid = it < cnt;
    uint32_t ri = 0, pair = 0, sp = 0, redo_item = 0;
    bool next = false, coop = false, lost = false, redo = false;
    WalkRec<T>* r = recs;
    T dlb = T(0), rec_dist = T(0), cand_val = T(0);
    if (valid && !(SOLID && (recs[wa.round ? wa.list_in[it] : it].flags & WALK_VOID))) {
      ri = wa.round ? wa.list_in[it] : it;
      r = recs + ri;
      pair = r->pair;
      sp = r->sp;
      const uint32_t n_leaf = r->n_leaf, flags = r->flags;
      bool swapped = false;
      if constexpr (SOLID) swapped = lib.kinds[wk.shape1[pair]] != uint8_t(K_BVH);
      dlb = r->dlb;
      rec_dist = r->rec_dist;
      cand_val = r->cand_val;
      int fb1 = -1, fb2 = -1, wit = -1;
      bool contact = false;
      auto boxes = [&](T pre) {  // updateDistanceLowerBoundFromBV over a run of disjoint boxes
        if (!(dlb <= T(0)) && pre < dlb) {
          dlb = pre;
          rec_dist = pre + q.security_margin;
        }
      };
      for (uint32_t s2 = 0; s2 < n_leaf; ++s2) {
        boxes(r->pre[s2]);
        const T distance = res[r->first_item + s2].distance;
        if (SOLID && distance == walk_leaf_epa<T>()) {  // canStop(): the bound and its witness stay as they are (k_bvh_collide's SOLID form)
          contact = true;
          redo = true;
          redo_item = ri | (s2 << 28);
          fb1 = swapped ? -1 : int(r->leaf1[s2]);
          fb2 = swapped ? int(r->leaf1[s2]) : -1;
          break;
        }
        const T dtc = distance - q.security_margin;
        if (dtc < dlb) {  // updateDistanceLowerBoundFromLeaf
          dlb = dtc;
          cand_val = dtc;
          rec_dist = distance;
          wit = int(s2);
        }
        if (dtc <= q.collision_distance_threshold) {  // the first contact: canStop()
          contact = true;
          fb1 = SOLID ? (swapped ? -1 : int(r->leaf1[s2])) : int(r->leaf1[s2]);
          fb2 = SOLID ? (swapped ? int(r->leaf1[s2]) : -1) : int(r->leaf2[s2]);
          break;
        }
      }
      if (!contact) boxes(r->pre[n_leaf]);
      if (wit >= 0) {
        const TriLeafOut<T> w = res[r->first_item + uint32_t(wit)];
        if (SOLID && swapped)
          store_witness(io, pair, w.p2, w.p1, -w.n);
        else
          store_witness(io, pair, w.p1, w.p2, w.n);
      }
      lost = (flags & WALK_LOST) != 0u;  // (its items did not fit the list)
      if (contact || (flags & WALK_OVER) || lost) {
        store_bvh_record_head(io, pair, rec_dist, contact ? 1u : 0u, fb1, fb2, lost);
      } else if (!wa.last && !(flags & WALK_BUDGET)) {
        next = true;
      } else {
        coop = true;
      }
      if (next || coop) {
        r->dlb = dlb;
        r->rec_dist = rec_dist;
        r->cand_val = cand_val;
      }
    }
    // ---- the queries that walk on: next round's list
    {
      const uint32_t slot = wave_reserve(&c[2], 1u, next);
      if (next) wa.list_out[slot] = ri;
    }
    if constexpr (SOLID) {  // ---- the leaves that ended their walks needing EPA
      const uint32_t slot = wave_reserve(&c[5], 1u, redo);
      if (redo && slot < wa.list_stride) wa.redo[slot] = redo_item;
    }
    // ---- the queries k_bvh_coop continues: a suspended query (its state a summary) whose stack entries are its tasks, top first
    if (__ballot(coop)) {
      const uint32_t my_slot = wave_reserve(&split.ctr[BVH_CTR_SUSPENDED], 1u, coop);
      const uint32_t first = wave_reserve(&split.ctr[BVH_CTR_TASKS], sp, coop);
      if (coop) {
        const bool fits = first + sp <= split.cap && my_slot < split.n_queries;
        if (my_slot < split.n_queries) split.suspended[my_slot] = pair;
        if (fits)
          for (uint32_t j = 0; j < sp; ++j) split.tasks[first + j] = BvhTask{pair, my_slot, r->stack[sp - 1u - j], j};
        else
          for (uint32_t j = first; j < min(first + sp, split.cap); ++j) split.tasks[j] = BvhTask{0u, 0u, 0xFFFFFFFFu, 0u};
        if (my_slot < split.n_queries) {
          BvhSum<T>* const sm = bvh_sum<T>(split, my_slot);
          sm->contact_order = 0xFFFFFFFFu; sm->parent = 0xFFFFFFFFu; sm->order = 0u; sm->pad_ = 0u;
          sm->dlb = dlb; sm->rec_dist = rec_dist; sm->cand_val = cand_val;
          sm->fb1 = sm->fb2 = -1;
          sm->ncontacts = 0u; sm->first_child = first; sm->n_child = fits ? sp : 0u;
          sm->flags = BVH_SUM_SUSPENDED | (fits ? 0u : BVH_SUM_OVERFLOW);  // (a full task table: flagged, as k_bvh_collide flags a stack it cannot hand on)
          load_witness(io, pair, sm->np1, sm->np2, sm->nn);
        }
      }
    }
  }
}

// =======================================================================================
// what both objects launch with, as templates over the object's part (MESH_UNIT_PART, passed explicitly) and over the object's own launch
// of its kernels; each object's launchers (hfcl_launch.hpp) are in its source
// =======================================================================================
// is a walk cut into tasks at all?  Contact lists need the running count of the whole query and run unsplit (k_bvh_collide, above)
static inline bool bvh_splitting(const BvhSplit& split, const BvhParams& bp) {
  return split.tasks && split.n_levels > 1 && bp.num_max_contacts == 1 && !bp.contacts;
}
// The continuation of the suspended queries by k_bvh_coop / k_bvh_shape_coop: one launch, or -- BvhSplit::cut_ticks -- three, the second and
// third walking the chunks the launch before cut its long walks into (levels 2 and 3 of the task table: k_bvh_level_mark files the
// tasks made so far under ctr[LEVEL0 + level + 1] and resets the ticket), and the fold-back of the chunks' summaries.
// after_first (optional): called once the mark behind the first launch is in the stream -- returns false when there is no such mark (no cutting)
template <typename T, int PART, class Launch, class AfterFirst>
static bool launch_coop_levels(int grid, hipStream_t st, const Work& wk, const IO<T>& io, BvhSplit s, int ticket, Launch&& launch, AfterFirst&& after_first) {
  const bool cutting = s.cut_ticks != 0 && s.cut_words != nullptr;
  s.level = 0;
  for (uint32_t l = 0; l < (cutting ? 3u : 1u); ++l) {
    hipLaunchKernelGGL((k_bvh_level_mark<PART>), dim3(1), dim3(64), 0, st, wk, s, ticket);
    if (l == 1) after_first();
    s.level = l ? l + 1 : 0u;  // launch 0: the suspended queries; launches 1, 2: the chunks of the launch before
    s.can_suspend = cutting && l < 2 ? 1u : 0u;
    launch(s);
    s.level = l + 1;  // (what the next mark files the tasks under)
  }
  if (cutting) {
    s.level = 2;
    hipLaunchKernelGGL((k_bvh_combine<T, PART>), dim3(std::max(1, std::min(grid, 1024))), dim3(256), 0, st, wk, io, s);
    s.level = 0;
    hipLaunchKernelGGL((k_bvh_combine<T, PART>), dim3(std::max(1, std::min(grid, 1024))), dim3(256), 0, st, wk, io, s);
  }
  return cutting;
}
template <typename T, int PART, class Launch>
static void launch_coop_levels(int grid, hipStream_t st, const Work& wk, const IO<T>& io, BvhSplit s, int ticket, Launch&& launch) {
  launch_coop_levels<T, PART>(grid, st, wk, io, s, ticket, launch, [] {});
}
// k_bvh_collide's task levels: one level per launch (levels > 0 walk the tasks the level before made), the fold-back launches in
// reverse order.  split.tasks == nullptr (or split.n_levels <= 1): the plain single-pass traversal.  launch_collide(split): the object's
// own launch of its narrow form of k_bvh_collide -- the mesh x mesh object's plain one, the mesh x solid object's SOLID one, so neither
// instantiates the other's --; ticket: the counter the levels draw their units from.
template <typename T, int PART, class LaunchCollide>
static void bvh_collide_levels(int grid, hipStream_t st, const Work& wk, const IO<T>& io, const BvhParams& bp, BvhSplit split, int ticket, LaunchCollide&& launch_collide) {
  if (!bvh_splitting(split, bp)) {
    split.tasks = nullptr;
    split.budget = 0;
    split.level = 0;
    split.can_suspend = 0;
    launch_collide(split);
    return;
  }
  const uint32_t budget = split.budget;
  for (uint32_t l = 0; l < split.n_levels; ++l) {
    split.level = l;
    split.budget = l + 1 < split.n_levels ? (l == 0 ? split.budget0 : budget) : 0u;  // the last level runs to the end
    BvhSplit s = split;
    s.can_suspend = l + 1 < split.n_levels;  // ... and cannot suspend (its stack overflows are flagged)
    launch_collide(s);
    hipLaunchKernelGGL((k_bvh_level_mark<PART>), dim3(1), dim3(64), 0, st, wk, s, ticket);
  }
  for (int l = int(split.n_levels) - 2; l >= 0; --l) {
    split.level = uint32_t(l);
    hipLaunchKernelGGL((k_bvh_combine<T, PART>), dim3(std::max(1, std::min(grid, 1024))), dim3(256), 0, st, wk, io, split);
  }
}
