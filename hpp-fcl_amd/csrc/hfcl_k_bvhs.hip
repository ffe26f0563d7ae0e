// hfcl_k_bvhs.hip -- BVHModel<OBBRSS> x convex solid distance(), either operand order: one query per lane group (k_bvh_shape_distance),
// or one per lane with its continuations (k_bvh_shape_distance_lane / _coop / _pool) and the leaves that needed EPA (k_bvh_shape_finish,
// hfcl_mesh.hpp).  Built WITHOUT contraction of a*b+c (Makefile: FLAGS_k_bvhs): the reported triangle hangs on comparisons of
// distances that are equal or an ulp apart (triangles that share the closest vertex or edge), and with the reference's arithmetic the
// ids, distances and witness points are the oracle's (profiles/r05_c: ids 77-93 % -> 100 % equal, distances 29-71 % -> 100 % bit-equal),
// as for mesh x mesh (hfcl_k_bvhd.hip).
#include "hfcl_mesh.hpp"

constexpr int MESH_UNIT_PART = 2;  // what this object's copy of a kernel two mesh objects launch carries (hfcl_mesh.hpp; hfcl_k_bvh.hip: 1, hfcl_k_bvhc.hip: 3)

// k_shape_obbrss: computeBV<OBBRSS, S>(solid, tf) per query, by pair, as k_shape_obb's for collide() (hfcl_k_bvhc.hip) -- for
// distance() the solid's OBBRSS itself (rss_lower_bound takes the mesh pose as an argument)
template <typename T>
__global__ void __launch_bounds__(256) k_shape_obbrss(Work wk, LibView<T> lib, IO<T> io) {
  const uint32_t cnt = wk.counts[B_BVHSHAPE];
  RssQuery<T>* const table = reinterpret_cast<RssQuery<T>*>(wk.shape_oq);
  for (uint32_t it = blockIdx.x * blockDim.x + threadIdx.x; it < cnt; it += gridDim.x * blockDim.x) {
    const uint32_t pair = wk.lists[size_t(B_BVHSHAPE) * wk.n + it];
    const uint32_t id1 = wk.shape1[pair], id2 = wk.shape2[pair];
    const bool swapped = lib.kinds[id1] != uint8_t(K_BVH);
    const DShape<T> shape = lib.shapes[swapped ? id1 : id2];
    const Pose<T> tfs = load_pose(swapped ? io.tf1 : io.tf2, pair);
    DNode<T> bv2;
    DRss<T> rss2;
    RssQuery<T> rq;
    if (shape_obbrss(shape, lib.verts, tfs, bv2, &rss2)) {
      rq.axes = bv2.axes;
      rq.Tr = rss2.Tr;
      rq.l0 = rss2.l0;
      rq.l1 = rss2.l1;
      rq.r = rss2.r;
    } else {
      const T nanv = Lim<T>::nan();
      rq.axes.r0 = rq.axes.r1 = rq.axes.r2 = rq.Tr = mk<T>(nanv, nanv, nanv);
      rq.l0 = rq.l1 = rq.r = nanv;
    }
    table[pair] = rq;
  }
}

// distance() counterpart: same lane-group layout, RSS lower bounds instead of OBB overlap tests.
template <typename T>
__global__ void __launch_bounds__(64) k_bvh_shape_distance(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<T, EPA_MAX_ITER> scratch[G];
  __shared__ uint32_t stack_n[G][BS_STACK];
  __shared__ T stack_d[G][BS_STACK];
  const uint32_t cnt = wk.counts[B_BVHSHAPE];
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint32_t it = blockIdx.x * G + grp; it < cnt; it += gridDim.x * G) {
    const uint32_t pair = wk.lists[size_t(B_BVHSHAPE) * wk.n + it];
    const DShape<T> a = lib.shapes[wk.shape1[pair]], b = lib.shapes[wk.shape2[pair]];
    const bool swapped = a.kind != K_BVH;  // distance.cpp:74-88
    const DShape<T> ms = swapped ? b : a;
    GroupSolid<T> solid;
    solid.s = swapped ? a : b;
    solid.v = lib.verts + 3 * size_t(solid.s.vertex_offset);
    solid.lig = lig;
    if (solid.s.kind == K_CONVEX && solid.s.num_points <= uint32_t(HULL_MAX)) solid.h.load(solid.v, solid.s.num_points, lig);
    const Pose<T> tf1 = load_pose(io.tf1, pair), tf2 = load_pose(io.tf2, pair);
    const Pose<T> tfm = swapped ? tf2 : tf1, tfs = swapped ? tf1 : tf2;
    const DMesh m = bv.meshes[ms.bvh_index];
    MeshShapeDist<T> st;
    mesh_shape_distance<T, LaneGroup<BS_W>>(bv.nodes + m.node_off, bv.rss + m.node_off, bv.verts + 3 * size_t(m.vert_off),
                                            bv.tris + 3 * size_t(m.tri_off), tfm, solid.s, lib.verts, tfs, solid, q, stack_n[grp],
                                            stack_d[grp], BS_STACK, &scratch[grp], initial_guess<T>(io, q, pair), st);
    if (lig == 0) {
      if (st.unsupported) {
        auto r = io.out[pair];
        memset(&r, 0, sizeof(r));
        r.status = 0x80000000u;
        io.out[pair] = r;
      } else {
        PairOut<T> o;
        o.distance = st.min_distance;
        o.normal = (swapped && st.nn.x == st.nn.x) ? -st.nn : st.nn;  // (no witness: the one NaN of every form, not its negative)
        o.p1 = swapped ? st.np2 : st.np1;
        o.p2 = swapped ? st.np1 : st.np2;
        o.gjk_status = GJK_DID_NOT_RUN;
        o.epa_status = EPA_DID_NOT_RUN;
        o.gjk_iters = o.epa_iters = 0;
        // b1 = the triangle, b2 = NONE whatever the operand order (distance.cpp:84-88 swaps o1/o2 only)
        store_bvh_record(io, pair, o, st.min_distance <= T(0) ? 0x80000000u : 0u, st.prim, -1, st.overflow);
        write_guess<T>(io, pair, st.guess, 0, 0);
      }
    }
    LaneGroup<BS_W>::sync();
  }
}

// ---------------------------------------------------------------------------------------
// k_bvh_shape_distance_lane: distance() between a mesh and a solid with ONE QUERY PER LANE (the streaming scheme of
// k_bvh_distance; MeshShapeDistanceTraversalNodeOBBRSS + distanceRecurse as in hfcl_bvh_shape.hpp: mesh_shape_distance).
// The solid's OBBRSS comes from k_shape_obbrss's table (re-read at every step: 15 numbers that do not wait for the node
// gather), the leaf is the SOLID collide form's (solid_leaf_call), the witness of the minimum lives in the record.  A leaf
// that needs EPA ends the walk -- its distance is <= 0 and every bound left on the stack >= 0 -- and is finished by
// k_bvh_shape_finish.  Bounds travel as in k_bvh_distance (4 bytes, rounded down, exact re-evaluation in the band).
// ---------------------------------------------------------------------------------------
#ifndef HFCL_BSD_PARK_MIN
#define HFCL_BSD_PARK_MIN 16
#endif
template <typename T>
__global__ void __launch_bounds__(BVHD_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 8)))
k_bvh_shape_distance_lane(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q, BvhSpill spill) {
  constexpr int STACK = BVHD_STACK;
  typedef typename std::conditional<sizeof(T) == 8, uint32_t, float>::type BD;
  __shared__ uint32_t stack_e[STACK][BVHD_BLOCK];
  __shared__ BD stack_d[STACK][BVHD_BLOCK];
  __shared__ T w0_slab[W0Lds<T, BVHD_BLOCK>::WORDS];
  const W0Lds<T, BVHD_BLOCK> leaf_ps{w0_slab + threadIdx.x};
  auto bound_down = [](T d) -> BD {
    if constexpr (sizeof(T) == 8)
      return uint32_t(__double2hiint(d));
    else
      return d;
  };
  auto bound_value = [](BD b) -> T {
    if constexpr (sizeof(T) == 8)
      return __hiloint2double(int(b), 0);
    else
      return b;
  };
  const uint32_t cnt = wk.counts[B_BVHSHAPE];
  uint32_t* const ticket = &wk.counts[CTR_SHAPE_TICKET];
  const RssQuery<T>* const table = reinterpret_cast<const RssQuery<T>*>(wk.shape_oq);
  const int tid = threadIdx.x, lane = tid & 63;
  const T nanv = Lim<T>::nan();
  bool live = false, pending = false, exhausted = false, swapped = false, overflow = false, unsupported = false, deferred = false;
  bool have_leaf = false;
  uint32_t pair = 0, solid_id = 0, leaf_prim = 0, steps = 0;
  DMesh m1 = {0, 0, 0, 0};
  Pose<T> tfm;
  tfm.R.r0 = tfm.R.r1 = tfm.R.r2 = tfm.t = mk<T>(T(0), T(0), T(0));
  T mind = Lim<T>::max();
  int fb1 = -1, sp = 0;
  V3<T> guess = mk<T>(T(1), T(0), T(0));
  // lower bound between the solid's volume and mesh node b (distance(tf1.R, tf1.T, model2_bv, model1.bv(b)))
  auto bound_of = [&](uint32_t b) -> T {
    const RssQuery<T> rq = table[pair];
    DNode<T> n2;
    n2.axes = rq.axes;
    DRss<T> r2;
    r2.Tr = rq.Tr;
    r2.l0 = rq.l0;
    r2.l1 = rq.l1;
    r2.r = rq.r;
    return rss_lower_bound(tfm.R, tfm.t, n2, r2, bv.nodes[m1.node_off + b], bv.rss[m1.node_off + b]);
  };
  auto leaf = [&](uint32_t prim) {
    SolidLeafIn<T> in{bv.verts + 3 * size_t(m1.vert_off), bv.tris + 3 * size_t(m1.tri_off + prim), lib.shapes, lib.verts,
                      swapped ? io.tf2 : io.tf1, swapped ? io.tf1 : io.tf2, reinterpret_cast<ShapeDeferItem<T>*>(wk.shape_defer),
                      &wk.counts[CTR_SHAPE_DEFER], wk.shape_defer_cap, pair, solid_id, prim, 0xFFFFFFFFu, 0u, mind, fb1};
    SolidLeafOut<T> lo;
    if (solid_leaf_call<T>(in, &q, leaf_ps, guess, &lo)) {
      deferred = true;  // k_bvh_shape_finish writes the record
      sp = 0;
      return;
    }
    guess = lo.guess;
    if (mind > lo.distance) {  // DistanceResult::update
      mind = lo.distance;
      fb1 = int(prim);
      store_witness(io, pair, swapped ? lo.p2 : lo.p1, swapped ? lo.p1 : lo.p2, swapped ? -lo.n : lo.n);
    }
  };
  for (;;) {
    if (live && sp == 0 && !have_leaf) {
      live = false;
      pending = !deferred;
    }
    const uint64_t live_mask = __ballot(live);
    const int n_live = __popcll(live_mask);
    if (exhausted ? n_live == 0 : 64 - n_live >= BVH_REFILL_MIN) {
      if (pending) {
        if (unsupported) {
          store_unsupported(io, pair);
        } else {
          // b1 = the triangle, b2 = NONE whatever the operand order (distance.cpp:84-88 swaps o1 / o2 only)
          store_bvh_record_head(io, pair, mind, mind <= T(0) ? 0x80000000u : 0u, fb1, -1, overflow);
          write_guess<T>(io, pair, guess, 0, 0);
        }
        pending = false;
      }
      if (exhausted) break;
      const int n_need = 64 - n_live;
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(ticket, uint32_t(n_need));
      base = __builtin_amdgcn_readfirstlane(base);
      if (!live) {
        const uint32_t it = base + uint32_t(__popcll(~live_mask & ((uint64_t(1) << lane) - 1)));
        if (it < cnt) {
          pair = wk.lists[size_t(B_BVHSHAPE) * wk.n + it];
          const uint32_t id1 = wk.shape1[pair], id2 = wk.shape2[pair];
          swapped = lib.kinds[id1] != uint8_t(K_BVH);  // distance.cpp:74-88
          solid_id = swapped ? id1 : id2;
          m1 = bv.meshes[lib.shapes[swapped ? id2 : id1].bvh_index];
          tfm = load_pose(swapped ? io.tf2 : io.tf1, pair);
          mind = Lim<T>::max();
          fb1 = -1;
          overflow = deferred = have_leaf = false;
          steps = 0;
          guess = initial_guess<T>(io, q, pair);
          const T probe = table[pair].r;
          unsupported = !(probe == probe);
          sp = 0;
          if (unsupported) {
            pending = true;
          } else {
            const V3<T> nan3 = mk<T>(nanv, nanv, nanv);
            store_witness(io, pair, nan3, nan3, nan3);
            live = true;
            sp = 1;  // (leaf() of a deferred preprocess() sets it back to 0)
            stack_e[0][tid] = 0u;
            stack_d[0][tid] = bound_down(T(-1));
            leaf(0u);  // preprocess(): triangle 0
          }
        }
      }
      if (base + uint32_t(n_need) >= cnt) exhausted = true;
      continue;
    }
    // A triangle against the solid is a GJK run: ten times a BV step.  A lane that pops one waits until HFCL_BSD_PARK_MIN
    // lanes do (or nobody can walk) and the wave runs the leaves together (k_bvh_distance, whose triangle pairs cost what a
    // BV step costs, evaluates them where they are popped).
    for (;;) {
      if (spill.budget && live && sp > 0 && !have_leaf && steps >= spill.budget) {
        // a long walk: its stack and its minimum go to a record, a wave takes it over (k_bvh_shape_distance_coop)
        ShapeDistSusp<T>* r = reinterpret_cast<ShapeDistSusp<T>*>(spill.susp) + atomicAdd(spill.susp_count, 1u);
        r->pair = pair;
        r->sp = uint32_t(sp);
        r->fb1 = fb1;
        r->pad_ = 0;
        r->mind = mind;
        for (int k = 0; k < sp; ++k) {
          r->entry[k] = stack_e[k][tid];
          r->bound[k] = bound_value(stack_d[k][tid]);
        }
        sp = 0;
        deferred = true;  // (no record from this lane)
      }
      const bool run = live && sp > 0 && !have_leaf;
      const int n_run = __popcll(__ballot(run)), n_wait = __popcll(__ballot(have_leaf));
      if (n_run == 0 || n_wait >= HFCL_BSD_PARK_MIN || (!exhausted && 64 - n_run - n_wait >= BVH_REFILL_MIN)) break;
      if (!run) continue;
      ++steps;
      --sp;
      const uint32_t b = stack_e[sp][tid];
      const BD dc = stack_d[sp][tid];
      const T de = bound_value(dc);
      if (de >= T(0) && de >= mind) continue;  // canStop(d)
      if constexpr (sizeof(T) == 8) {
        if (de >= T(0) && __hiloint2double(int(dc) + 1, 0) > mind) {  // the exact bound may reach the minimum: ask it
          if (bound_of(b) >= mind) continue;
        }
      }
      const int32_t fc = bv.nodes[m1.node_off + b].first_child;
      if (fc < 0) {
        have_leaf = true;
        steps += 15;  // (a GJK leaf counts sixteen steps)
        leaf_prim = uint32_t(-(fc + 1));
        continue;
      }
      const uint32_t a1 = uint32_t(fc), c1 = a1 + 1;
      const T d1 = bound_of(a1), d2 = bound_of(c1);
      if (sp + 2 > STACK) {
        overflow = true;
        sp = 0;
        continue;
      }
      const bool c_first = d2 < d1;  // the nearer child is visited first
      stack_e[sp][tid] = c_first ? a1 : c1;
      stack_d[sp][tid] = bound_down(c_first ? d1 : d2);
      ++sp;
      stack_e[sp][tid] = c_first ? c1 : a1;
      stack_d[sp][tid] = bound_down(c_first ? d2 : d1);
      ++sp;
    }
    if (have_leaf) {
      have_leaf = false;
      leaf(leaf_prim);
    }
  }
}

// ---------------------------------------------------------------------------------------
// k_bvh_shape_distance_coop: the long mesh x solid distance() walks, a wave per query (the scheme of k_bvh_distance_coop, hfcl_k_bvhd.hip;
// the triangles in front of the first node that is split run their leaves -- per-lane GJK -- side by side; a triangle that
// needs EPA ends the walk as in the lane kernel: only the FIRST such triangle in stack order queues its item).
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 8)))
k_bvh_shape_distance_coop(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q, BvhSpill spill) {
  constexpr int CAP = 960, SLACK = 64;
  __shared__ uint32_t stack_e[CAP + SLACK];
  __shared__ T stack_d[CAP + SLACK];
  __shared__ T w0_slab[W0Lds<T, 64>::WORDS];
  const W0Lds<T, 64> leaf_ps{w0_slab + threadIdx.x};
  const int lane = threadIdx.x;
  const uint32_t n_susp = *spill.susp_count;
  const RssQuery<T>* const table = reinterpret_cast<const RssQuery<T>*>(wk.shape_oq);
  const T big = Lim<T>::max();
  for (uint32_t qi = blockIdx.x; qi < n_susp; qi += gridDim.x) {
    const ShapeDistSusp<T>* const r = reinterpret_cast<const ShapeDistSusp<T>*>(spill.susp) + qi;
    const uint32_t pair = r->pair;
    const uint32_t id1 = wk.shape1[pair], id2 = wk.shape2[pair];
    const bool swapped = lib.kinds[id1] != uint8_t(K_BVH);
    const uint32_t solid_id = swapped ? id1 : id2;
    const DMesh m1 = bv.meshes[lib.shapes[swapped ? id2 : id1].bvh_index];
    const Pose<T> tfm = load_pose(swapped ? io.tf2 : io.tf1, pair);
    const RssQuery<T> rq = table[pair];
    DNode<T> n2;
    n2.axes = rq.axes;
    DRss<T> r2;
    r2.Tr = rq.Tr;
    r2.l0 = rq.l0;
    r2.l1 = rq.l1;
    r2.r = rq.r;
    auto bound_of = [&](uint32_t b) -> T { return rss_lower_bound(tfm.R, tfm.t, n2, r2, bv.nodes[m1.node_off + b], bv.rss[m1.node_off + b]); };
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int sp = int(r->sp);
    if (lane < sp) {
      stack_e[lane] = r->entry[lane];
      stack_d[lane] = r->bound[lane];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    T mind = r->mind;
    int fb1 = r->fb1;
    bool overflow = false, deferred = false;
    const V3<T> guess0 = initial_guess<T>(io, q, pair);  // (walks whose leaves hand a cached guess on are not suspended)
    V3<T> guess = guess0;
    while (sp > 0) {
      const int w = min(64, min(sp, max(CAP - sp, 1)));
      const bool act = lane < w;
      const uint32_t b = act ? stack_e[sp - 1 - lane] : 0u;
      const T db = act ? stack_d[sp - 1 - lane] : big;
      sp -= w;
      const bool alive = act && !(db >= T(0) && db >= mind);  // canStop(d), with the minimum of the moment
      const int32_t fc = alive ? bv.nodes[m1.node_off + b].first_child : 0;
      const bool is_leaf = alive && fc < 0, split = alive && fc >= 0;
      T d1 = big, d2 = big;
      if (split) {
        d1 = bound_of(uint32_t(fc));
        d2 = bound_of(uint32_t(fc) + 1u);
      }
      const uint64_t smask = __ballot(split);
      const int f = smask ? __ffsll((unsigned long long)smask) - 1 : 64;  // the triangles in front of it are visited now
      const bool visit = is_leaf && lane < f;
      T val = big;
      bool to_epa = false;
      SolidLeafOut<T> lo;
      lo.distance = big;
      const uint32_t prim = uint32_t(-(fc + 1));
      auto run_leaf = [&](bool push, T bound, int prev) -> bool {
        SolidLeafIn<T> in{bv.verts + 3 * size_t(m1.vert_off), bv.tris + 3 * size_t(m1.tri_off + prim), lib.shapes, lib.verts,
                          swapped ? io.tf2 : io.tf1, swapped ? io.tf1 : io.tf2, push ? reinterpret_cast<ShapeDeferItem<T>*>(wk.shape_defer) : nullptr,
                          push ? &wk.counts[CTR_SHAPE_DEFER] : nullptr, wk.shape_defer_cap, pair, solid_id, prim, 0xFFFFFFFFu, 0u, bound, prev};
        return solid_leaf_call<T>(in, &q, leaf_ps, guess0, &lo);
      };
      if (visit) {
        to_epa = run_leaf(false, T(0), -1);
        if (!to_epa) val = lo.distance;
      }
      // The evaluated triangles, in stack order, exactly as the lane's walk takes them: a triangle counts only if its bound does
      // not let it be skipped at ITS turn (canStop with the minimum as it stands then -- a bound is clamped at 0, so after a
      // penetration every bounded entry is skipped, and the bounds of unbounded solids are NaN and never skip), the minimum is
      // lowered by strictly smaller distances only, and a counted triangle that needs EPA ends the walk.
      const uint64_t emask = __ballot(to_epa);
      int start = 0, src = -1;
      bool epa_end = false;
      T run = mind;
      for (;;) {
        const uint64_t em = emask & ~((uint64_t(1) << start) - 1);
        const int c = em ? __ffsll((unsigned long long)em) - 1 : 64;  // the next triangle that needs EPA
        for (;;) {  // the record-setting triangles in front of it
          const bool cand = visit && !to_epa && lane >= start && lane < c && !(db >= T(0) && db >= run) && val < run;
          const uint64_t m = __ballot(cand);
          if (!m) break;
          src = __ffsll((unsigned long long)m) - 1;
          run = __shfl(val, src);
          start = src + 1;
        }
        if (c >= 64) break;
        const T dbc = __shfl(db, c);
        if (!(dbc >= T(0) && dbc >= run)) {  // it is visited: the walk ends here
          epa_end = true;
          start = c;
          break;
        }
        start = c + 1;  // (skipped like any entry whose bound cannot beat the minimum)
        if (start >= 64) break;
      }
      if (src >= 0) {  // DistanceResult::update
        mind = run;
        fb1 = __shfl(int(prim), src);
        if (lane == src) store_witness(io, pair, swapped ? lo.p2 : lo.p1, swapped ? lo.p1 : lo.p2, swapped ? -lo.n : lo.n);
        guess = mk<T>(__shfl(lo.guess.x, src), __shfl(lo.guess.y, src), __shfl(lo.guess.z, src));
      }
      if (epa_end) {
        if (lane == start) run_leaf(true, mind, fb1);  // its leaf once more, with the EPA item: k_bvh_shape_finish writes the record
        deferred = true;
        sp = 0;
        break;
      }
      // the stack again, in order: visited triangles and dropped entries are gone, a split node is its two children (the
      // nearer one on top), a triangle behind the first split stays
      const int cnt = split ? 2 : ((is_leaf && lane >= f) ? 1 : 0);
      const uint64_t m2b = __ballot(cnt == 2), m1b = __ballot(cnt == 1);
      const uint64_t deeper = ~((uint64_t(2) << lane) - 1);
      const int pos = sp + 2 * __popcll(m2b & deeper) + __popcll(m1b & deeper);
      if (cnt == 2) {
        const uint32_t a1 = uint32_t(fc), c1 = a1 + 1u;
        const bool c_first = d2 < d1;  // the nearer child is visited first
        stack_e[pos] = c_first ? a1 : c1;
        stack_d[pos] = c_first ? d1 : d2;
        stack_e[pos + 1] = c_first ? c1 : a1;
        stack_d[pos + 1] = c_first ? d2 : d1;
      } else if (cnt == 1) {
        stack_e[pos] = b;
        stack_d[pos] = db;
      }
      sp += 2 * __popcll(m2b) + __popcll(m1b);
      if (sp > CAP + SLACK - 2) {
        overflow = true;
        sp = 0;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0 && !deferred) {
      // b1 = the triangle, b2 = NONE whatever the operand order (distance.cpp:84-88 swaps o1 / o2 only)
      store_bvh_record_head(io, pair, mind, mind <= T(0) ? 0x80000000u : 0u, fb1, -1, overflow);
      write_guess<T>(io, pair, guess, 0, 0);
    }
  }
}

// ---------------------------------------------------------------------------------------
// k_bvh_shape_distance_pool: the long mesh x solid distance() walks with the scheme of k_bvh_distance_pool (hfcl_k_bvhd.hip, round 4):
// SDP_Q walks per wave, each with its stack in LDS in DFS order; the child tests of every mesh node that is split go into one list for
// the wave, worked off 64 at a time (one rss_lower_bound per lane against the walk's solid, on the packed DNodeD records); the
// triangles of the wave's windows are evaluated together, one GJK run per lane, whichever walk they belong to; a marker per walk
// (entries that stand behind the triangle of the minimum) keeps the reference's choice among equal distances whatever the order of
// the evaluations.  What this row adds to the mesh x mesh form: a triangle inside the solid (its leaf asks for EPA) ends the walk at
// its turn, so the FIRST such triangle in DFS order is the walk's result -- it ranks below every distance, ties by DFS order --, the
// entries behind it are dropped, the ones in front are finished (they may hold an earlier one), and when the stack is empty its
// lane runs the leaf once more to queue the EPA item (k_bvh_shape_finish writes the record), as k_bvh_shape_distance_coop does.
// Suspended walks never hand a cached guess on and their final guess is not read (the host does not suspend those).
// ---------------------------------------------------------------------------------------
// (124 entries before the windows narrow -- it was 160 --: with the chain word per entry the fp64 block is 20 288 B, eight waves per CU)
constexpr int SDP_Q = 4, SDP_SEG = 64 / SDP_Q, SDP_CAPW = 124, SDP_CAP = SDP_CAPW + BVHD_STACK + 8;
template <typename T>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 8)))
k_bvh_shape_distance_pool(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q, BvhSpill spill) {
  constexpr int Q = SDP_Q, SEG = SDP_SEG;
  __shared__ uint32_t st_x[Q][SDP_CAP];  // bit 31: a triangle (bits 0-30 its id); else a mesh node whose first child is bits 0-30
  __shared__ T st_d[Q][SDP_CAP];
  __shared__ float st_c[Q][SDP_CAP];  // the largest bound among the entry's ancestors where it exceeds the entry's own, rounded up (0: none; k_bvh_distance_pool)
  __shared__ T q_tf[Q][12];    // pose of the mesh (R rows, t): the R0, T0 of the bound
  __shared__ T q_rss[Q][15];   // the solid's RSS in the mesh frame's terms (RssQuery): axes, Tr, l0, l1, r
  __shared__ uint32_t q_ids[Q][6];  // pair, solid id, swapped, vert_off, tri_off, node_off
  __shared__ uint32_t t_node[128], t_x[128];
  __shared__ uint8_t t_q[128];
  __shared__ T t_res[128];
  __shared__ T w0_slab[W0Lds<T, 64>::WORDS];
  const W0Lds<T, 64> leaf_ps{w0_slab + threadIdx.x};
  const int lane = threadIdx.x, qs = lane / SEG, j = lane % SEG;
  const uint64_t lt_mask = (uint64_t(1) << lane) - 1;
  const uint64_t segm = ((uint64_t(1) << SEG) - 1) << (qs * SEG);
  const uint64_t deeper = segm & ~((uint64_t(2) << lane) - 1);
  const uint32_t n_susp = *spill.susp_count;
  const RssQuery<T>* const table = reinterpret_cast<const RssQuery<T>*>(wk.shape_oq);
  const int leaf_min = int(spill.pool_leaf_min), starve = int(spill.pool_starve);
  const T big = Lim<T>::max();
  auto sync = []() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  // slot state, identical in the SEG lanes of a slot
  // `ended`: a triangle that ENDS the sequential walk at its turn has been found (p marks it): it asks for EPA (ended_epa), or its
  // leaf reported a negative distance without EPA (a closed form) while its bound is a number -- bounds are clamped at 0, so behind
  // such a triangle every bounded entry is skipped: the walk's result is the FIRST such triangle in DFS order, not the smallest value
  // `ordered`: the slot walks a flagged record again, in the reference's order (k_bvh_distance_pool, hfcl_k_bvhd.hip; below); `redo`: it is
  // about to take that record again; `touched`: the ordered walk has set a minimum or ended (else the record's witness, which the pooled
  // pass has overwritten, is evaluated again at the end)
  bool active = false, exhausted = false, ended = false, ended_epa = false, overflow = false, flagged = false, ordered = false, redo = false, touched = false;
  int sp = 0, p = 0, fb1 = -1, end_prim = -1;
  T mind = big, end_val = T(0), margin = T(0), pooled = T(0), cut = big;
  uint32_t pair = 0, susp_it = 0;
  for (;;) {
    const uint64_t idle = __ballot(!active && !redo && j == 0);
    const bool any_redo = __ballot(redo) != 0;
    if ((idle && !exhausted) || any_redo) {
      uint32_t it = n_susp;
      if (idle && !exhausted) {
        const int n_need = __popcll(idle);
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(spill.pool_ticket, uint32_t(n_need));
        base = __builtin_amdgcn_readfirstlane(base);
        if (base + uint32_t(n_need) >= n_susp) exhausted = true;
        it = base + uint32_t(__popcll(idle & ((uint64_t(1) << (qs * SEG)) - 1)));
      }
      if (redo) it = susp_it;  // the slot's own record once more
      if ((!active && it < n_susp) || redo) {
        const ShapeDistSusp<T>* const r = reinterpret_cast<const ShapeDistSusp<T>*>(spill.susp) + it;
        pair = r->pair;
        ordered = redo;
        redo = touched = false;
        const uint32_t id1 = wk.shape1[pair], id2 = wk.shape2[pair];
        const bool swapped = lib.kinds[id1] != uint8_t(K_BVH);
        const DMesh m1 = bv.meshes[lib.shapes[swapped ? id2 : id1].bvh_index];
        sp = int(r->sp);
        p = sp;  // everything on the stack comes after what the lane has visited
        mind = r->mind;
        fb1 = r->fb1;
        ended = ended_epa = false;
        end_prim = -1;
        overflow = false;
        susp_it = it;
        flagged = false;  // (the lane's minimum is one the sequential walk holds)
        const RssQuery<T> rq0 = table[pair];
        const Pose<T> ltf = load_pose(swapped ? io.tf2 : io.tf1, pair);
        DNodeD<T> lS;
        lS.axes = rq0.axes;
        lS.Tr = rq0.Tr;
        lS.l0 = rq0.l0;
        lS.l1 = rq0.l1;
        lS.r = rq0.r;
        // (not vectorised: hipcc 7.2's instruction selection dies on the masked gather the loop vectoriser makes of this loop)
#pragma clang loop vectorize(disable) interleave(disable)
        for (int k = j; k < sp; k += SEG) {
          const uint32_t b = r->entry[k];
          const DNodeD<T>* const mn = bv.dnodes + m1.node_off + b;
          const int32_t fc = mn->first_child;
          st_x[qs][k] = fc < 0 ? (0x80000000u | uint32_t(-(fc + 1))) : uint32_t(fc);
          // fp64: the exact bounds again (the lane's stack carries them rounded down to 32 bits); the root's -1 stays
          T bk = r->bound[k];
          if constexpr (sizeof(T) == 8) {
            if (bk >= T(0)) bk = rss_lower_bound(ltf.R, ltf.t, lS, *mn);
          }
          st_d[qs][k] = bk;
          st_c[qs][k] = 0.0f;  // (its ancestors were decided by the lane, in the reference's order)
        }
        {
          // what a bound may exceed a distance beneath it by: a few ulps of the scene's size (the solid's volume in the mesh's frame and
          // the mesh's root volume), as in k_bvh_distance_pool -- an entry IN FRONT of the minimum is kept within that margin
          const DNodeD<T>* const root = bv.dnodes + m1.node_off;
          const T scale = habs(rq0.Tr.x) + habs(rq0.Tr.y) + habs(rq0.Tr.z) + rq0.l0 + rq0.l1 + T(2) * rq0.r + habs(root->Tr.x) + habs(root->Tr.y) +
                          habs(root->Tr.z) + root->l0 + root->l1 + T(2) * root->r;
          margin = T(16) * Lim<T>::eps() * scale;
          // ... and what a leaf's distance may fall short of the true one by: the supports of Box, Cone and Cylinder are inflated by 1e-10
          // (support_functions.cpp:146,229,281: hfcl_shapes.hpp), so GJK measures to a solid that much larger than the one the bound is
          // taken to -- a triangle 0.89 from a box had its leaf bound 2.9e-11 ABOVE its distance
          const DShape<T> sd = lib.shapes[swapped ? id1 : id2];
          if (sd.kind == K_BOX || sd.kind == K_CONE || sd.kind == K_CYLINDER) margin += T(2e-10) * (habs(sd.p0) + habs(sd.p1) + habs(sd.p2));
        }
        if (j == 0) {
          const Pose<T>& tfm = ltf;
          T* o = q_tf[qs];
          o[0] = tfm.R.r0.x; o[1] = tfm.R.r0.y; o[2] = tfm.R.r0.z; o[3] = tfm.R.r1.x; o[4] = tfm.R.r1.y; o[5] = tfm.R.r1.z;
          o[6] = tfm.R.r2.x; o[7] = tfm.R.r2.y; o[8] = tfm.R.r2.z; o[9] = tfm.t.x; o[10] = tfm.t.y; o[11] = tfm.t.z;
          const RssQuery<T>& rq = rq0;
          T* g = q_rss[qs];
          g[0] = rq.axes.r0.x; g[1] = rq.axes.r0.y; g[2] = rq.axes.r0.z; g[3] = rq.axes.r1.x; g[4] = rq.axes.r1.y; g[5] = rq.axes.r1.z;
          g[6] = rq.axes.r2.x; g[7] = rq.axes.r2.y; g[8] = rq.axes.r2.z; g[9] = rq.Tr.x; g[10] = rq.Tr.y; g[11] = rq.Tr.z;
          g[12] = rq.l0; g[13] = rq.l1; g[14] = rq.r;
          uint32_t* c = q_ids[qs];
          c[0] = pair; c[1] = swapped ? id1 : id2; c[2] = swapped ? 1u : 0u; c[3] = m1.vert_off; c[4] = m1.tri_off; c[5] = m1.node_off;
        }
        active = true;
      }
      sync();
    }
    if (__ballot(active) == 0) break;
    // ---- the windows
    const int w = active ? min(SEG, min(sp, max(SDP_CAPW - sp, 1))) : 0;
    const int base_i = sp - w;
    const bool act = j < w;
    const int idx = sp - 1 - j;
    uint32_t x = 0u;
    T db = big;
    float ch = 0.0f;
    if (act) {
      x = st_x[qs][idx];
      db = st_d[qs][idx];
      ch = st_c[qs][idx];
    }
    // behind a triangle that ends the walk nothing is visited; else canStop(bound) with the slot's minimum: behind the triangle of
    // the minimum the sequential walk's test, in front of it a tie is kept (k_bvh_distance_pool; NaN bounds never skip)
    // (ordered mode: what lies above the cut is gone, everything else is decided below)
    const bool alive = act && (ordered ? !(db > cut) : !(ended && idx < p) && !(db >= T(0) && (idx < p && !ended ? db >= mind : db > mind + margin)));
    bool is_leaf = alive && (x >> 31) != 0u, split = alive && (x >> 31) == 0u, held = false;
    // ---- Ordered mode (k_bvh_distance_pool): a node whose bound is below the pooled minimum -- or 0: the sequential walk's minimum is
    // positive until the walk ends -- is split by that walk whatever its minimum, and so here, wherever it stands; a node of the band
    // between that and the cut is decided at the top of the stack only; the triangles in front of the slot's first node are evaluated
    // together and applied in stack order (the scan below does that in either mode); everything else waits for its turn.
    if (__ballot(ordered) != 0) {
      const uint64_t boxm = __ballot(split) & segm;
      const int f = boxm ? __ffsll((unsigned long long)boxm) - 1 - qs * SEG : SEG;
      if (ordered) {
        if (split && !(db < pooled || db <= T(0))) {
          if (j == 0) {
            if (db >= mind) split = false;  // canStop at its turn
          } else {
            split = false;
            held = true;
          }
        } else if (is_leaf) {
          if (j > f) {
            is_leaf = false;  // behind a node: not its turn yet
            held = true;
          } else if (db >= T(0) && db >= mind) {
            is_leaf = false;  // canStop with a minimum that is not above the one of its turn
          }
        }
      }
    }
    // ---- the children's bounds of every split node of the wave in one list
    const uint64_t smask = __ballot(split);
    const int ns = __popcll(smask), k2 = 2 * __popcll(smask & lt_mask);
    if (split) {
      t_node[k2] = x;
      t_node[k2 + 1] = x + 1u;
      t_q[k2] = uint8_t(qs);
      t_q[k2 + 1] = uint8_t(qs);
    }
    sync();
    for (int tb = 0; tb < 2 * ns; tb += 64) {
      const int t = tb + lane;
      if (t < 2 * ns) {
        const uint32_t ts = t_q[t];
        const T* const f = q_tf[ts];
        const T* const g = q_rss[ts];
        M3<T> R0;
        R0.r0 = mk<T>(f[0], f[1], f[2]);
        R0.r1 = mk<T>(f[3], f[4], f[5]);
        R0.r2 = mk<T>(f[6], f[7], f[8]);
        const V3<T> T0 = mk<T>(f[9], f[10], f[11]);
        DNodeD<T> S;
        S.axes.r0 = mk<T>(g[0], g[1], g[2]);
        S.axes.r1 = mk<T>(g[3], g[4], g[5]);
        S.axes.r2 = mk<T>(g[6], g[7], g[8]);
        S.Tr = mk<T>(g[9], g[10], g[11]);
        S.l0 = g[12];
        S.l1 = g[13];
        S.r = g[14];
        const DNodeD<T> M = bv.dnodes[q_ids[ts][5] + t_node[t]];
        t_res[t] = rss_lower_bound(R0, T0, S, M);
        t_x[t] = M.first_child < 0 ? (0x80000000u | uint32_t(-(M.first_child + 1))) : uint32_t(M.first_child);
      }
    }
    sync();
    T d1 = big, d2 = big;
    uint32_t xa = 0u, xc = 0u;
    if (split) {
      d1 = t_res[k2];
      d2 = t_res[k2 + 1];
      xa = t_x[k2];
      xc = t_x[k2 + 1];
    }
    // ---- the triangles, once they are worth a pass (one GJK run per lane)
    const int nl = __popcll(__ballot(is_leaf));
    const bool do_leaves = nl > 0 && (nl >= leaf_min || 2 * ns < starve || ns == 0);  // (nothing but triangles in the windows: they run, whatever the knobs say)
    int jw = -1;
    T run_at = mind;  // the slot's minimum as of this lane's own turn in the pass, and whether the pass had set one / ended the walk by then
    bool upd_at = false, stop_at = false;
    if (do_leaves) {
      T val = big;
      bool to_epa = false;
      SolidLeafOut<T> lo;
      lo.distance = big;
      const uint32_t prim = x & 0x7FFFFFFFu;
      if (is_leaf) {
        const uint32_t* c = q_ids[qs];
        const bool swapped = c[2] != 0u;
        SolidLeafIn<T> in{bv.verts + 3 * size_t(c[3]), bv.tris + 3 * size_t(c[4] + prim), lib.shapes, lib.verts,
                          swapped ? io.tf2 : io.tf1, swapped ? io.tf1 : io.tf2, nullptr, nullptr, 0u, pair, c[1], prim, 0xFFFFFFFFu, 0u, T(0), -1};
        to_epa = solid_leaf_call<T>(in, &q, leaf_ps, initial_guess<T>(io, q, pair), &lo);
        if (!to_epa) val = lo.distance;
      }
      // DistanceResult::update over the slot's evaluated triangles IN THE ORDER OF THEIR VISITS (window index 0 = the top of the stack
      // = visited first).  The sequential walk tests an entry against the minimum of ITS turn: a triangle behind a minimum that an
      // earlier triangle of this very pass has set is visited only if its bound is below that minimum -- evaluated together, a
      // triangle whose bound exceeds its own distance by an ulp would otherwise lower a minimum the reference never lowers (two
      // records in 20 000 box queries, profiles/r05_c).  A triangle that ends the walk (asks for EPA, or a negative closed-form
      // distance behind a bound) is the result if the walk reaches it; against the standing result a tie wins only in front of it.
      const bool ends = is_leaf && (to_epa || (val < T(0) && db >= T(0)));
      // a bound of the triangle's chain above its distance (an ending triangle: above 0 -- the sequential walk's minimum is positive until
      // the walk ends, so bounds of 0 never turn it away): the sequential walk may not have come here, the walk is re-run in order
      const T chain = ch != 0.0f ? T(ch) : db;
      const bool viol = is_leaf && chain > (ends ? T(0) : val);
      T run = mind;
      bool upd = false, stop = false;
      int win_min = -1, win_end = -1;
#pragma unroll 4
      for (int s = 0; s < SEG; ++s) {
        const int src = qs * SEG + s;
        if (j == s) {
          run_at = run;
          upd_at = upd;
          stop_at = stop;
        }
        const bool leaf_s = __shfl(int(is_leaf), src) != 0, ends_s = __shfl(int(ends), src) != 0, viol_s = __shfl(int(viol), src) != 0;
        const T db_s = __shfl(db, src), val_s = __shfl(val, src);
        const int idx_s = sp - 1 - s;
        const bool visited = leaf_s && !stop && !(upd && db_s >= T(0) && db_s >= run);
        const bool take_end = visited && ends_s && (!ended || idx_s >= p);
        const bool take_min = visited && !ends_s && !ended && (val_s < run || (val_s == run && !upd && idx_s >= p && !ordered));
        if (take_min) {
          run = val_s;
          win_min = s;
          upd = true;
        }
        if (take_end) {
          win_end = s;
          stop = true;
        }
        flagged = flagged || ((take_min || take_end) && viol_s);
      }
      const bool swapped = q_ids[qs][2] != 0u;
      bool w_epa = false;
      if (win_min >= 0) {
        mind = run;
        fb1 = __shfl(int(prim), qs * SEG + win_min);
        jw = win_min;
        touched = true;
      }
      if (win_end >= 0) {
        const int src = qs * SEG + win_end;
        w_epa = __shfl(int(to_epa), src) != 0;
        ended = true;
        touched = true;
        ended_epa = w_epa;
        end_prim = __shfl(int(prim), src);
        if (!w_epa) end_val = __shfl(val, src);
        jw = win_end;
      }
      // the witness of the record: the ending triangle's when it carries a distance, else the minimum's (an EPA item falls back to it)
      const int w_lane = (win_end >= 0 && !w_epa) ? win_end : win_min;
      if (w_lane >= 0 && j == w_lane && (w_lane == win_end || win_min >= 0))
        store_witness(io, pair, swapped ? lo.p2 : lo.p1, swapped ? lo.p1 : lo.p2, swapped ? -lo.n : lo.n);
    }
    // ---- the windows written back, in order (a node behind a minimum of this pass that its bound does not beat, or behind a triangle
    // that ended the walk in this pass, is not split: the sequential walk skips it at its turn)
    const bool unsplit = split && (stop_at || (upd_at && db >= T(0) && db >= run_at));
    const int cnt = (split && !unsplit) ? 2 : (((is_leaf && !do_leaves) || held) ? 1 : 0);
    const uint64_t m2b = __ballot(cnt == 2), m1b = __ballot(cnt == 1);
    const int pos = base_i + 2 * __popcll(m2b & deeper) + __popcll(m1b & deeper);
    if (cnt == 2) {
      const bool c_first = d2 < d1;  // the nearer child is visited first
      // the children's chains: the parent's largest bound (its own, or what it inherited) where the child's own is below it
      const T pc = ch != 0.0f ? T(ch) : db;
      const float pcw = ch != 0.0f ? ch : chain_up(db);
      const float ca = d1 >= pc ? 0.0f : pcw, cc = d2 >= pc ? 0.0f : pcw;
      st_x[qs][pos] = c_first ? xa : xc;
      st_d[qs][pos] = c_first ? d1 : d2;
      st_c[qs][pos] = c_first ? ca : cc;
      st_x[qs][pos + 1] = c_first ? xc : xa;
      st_d[qs][pos + 1] = c_first ? d2 : d1;
      st_c[qs][pos + 1] = c_first ? cc : ca;
    } else if (cnt == 1) {
      st_x[qs][pos] = x;
      st_d[qs][pos] = db;
      st_c[qs][pos] = ch;
    }
    const uint64_t later_m = __ballot(act && (jw >= 0 ? j > jw : idx < p)) & segm;
    p = (jw >= 0 ? base_i : min(p, base_i)) + 2 * __popcll(m2b & later_m) + __popcll(m1b & later_m);
    sp = base_i + 2 * __popcll(m2b & segm) + __popcll(m1b & segm);
    if (sp > SDP_CAP - 2) {
      overflow = true;
      sp = 0;
    }
    // ordered mode: a triangle that ends the walk has everything that is left behind it; and a minimum that has come down to the pooled one
    // is the first the reference meets at the final distance -- nothing behind it replaces it
    if (ordered && (ended || mind <= pooled)) sp = 0;
    sync();
    if (active && sp == 0) {  // this walk is over
      if ((flagged || spill.rerun_all) && !ordered && !overflow && spill.rerun_count) {
        // not written: the slot takes the record again and walks it in the reference's order.  What the pooled pass found bounds that walk:
        // no entry whose bound exceeds it by a multiple of the arithmetic's slack can hold the reference's triangle
        pooled = ended ? T(0) : mind;
        cut = pooled + T(64) * margin;
        redo = true;
        if (j == 0) atomicAdd(spill.rerun_count, 1u);
      } else if (j == 0) {
        const bool epa_item = ended && ended_epa && !overflow;
        // the ordered walk has kept the minimum its record came with: that triangle's witness once more (the pooled pass wrote its own)
        const bool witness_again = ordered && !touched && !overflow && fb1 >= 0;
        if (epa_item || witness_again) {
          // the triangle that ended the walk: its leaf once more, with the EPA item (k_bvh_shape_finish writes the record)
          const uint32_t* c = q_ids[qs];
          const bool swapped = c[2] != 0u;
          const uint32_t again = uint32_t(epa_item ? end_prim : fb1);
          SolidLeafIn<T> in{bv.verts + 3 * size_t(c[3]), bv.tris + 3 * size_t(c[4] + again), lib.shapes, lib.verts,
                            swapped ? io.tf2 : io.tf1, swapped ? io.tf1 : io.tf2, epa_item ? reinterpret_cast<ShapeDeferItem<T>*>(wk.shape_defer) : nullptr,
                            epa_item ? &wk.counts[CTR_SHAPE_DEFER] : nullptr, epa_item ? wk.shape_defer_cap : 0u, pair, c[1], again, 0xFFFFFFFFu, 0u, epa_item ? mind : T(0), epa_item ? fb1 : -1};
          SolidLeafOut<T> lo;
          const bool deferred = solid_leaf_call<T>(in, &q, leaf_ps, initial_guess<T>(io, q, pair), &lo);
          if (!epa_item && !deferred) store_witness(io, pair, swapped ? lo.p2 : lo.p1, swapped ? lo.p1 : lo.p2, swapped ? -lo.n : lo.n);
        }
        if (!epa_item) {
          // b1 = the triangle, b2 = NONE whatever the operand order (distance.cpp:84-88 swaps o1 / o2 only)
          const T dist = ended && !overflow ? end_val : mind;
          store_bvh_record_head(io, pair, dist, dist <= T(0) ? 0x80000000u : 0u, ended && !overflow ? end_prim : fb1, -1, overflow);
          write_guess<T>(io, pair, initial_guess<T>(io, q, pair), 0, 0);
        }
      }
      active = false;
      ordered = false;
    }
  }
}

// =======================================================================================
// launchers (hfcl_launch.hpp)
// =======================================================================================
// mesh x solid distance(), one query per lane
template <typename T>
void launch_bvh_shape_distance_fast(int grid, int grid_finish, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, BvhSpill spill) {
  hipLaunchKernelGGL((k_shape_obbrss<T>), dim3(std::max(1, grid / 4)), dim3(256), 0, st, wk, lv, io);
  hipLaunchKernelGGL((k_bvh_shape_distance_lane<T>), dim3(grid), dim3(BVHD_BLOCK), 0, st, wk, lv, bv, io, q, spill);
  const int n_est = int(std::min<uint32_t>(wk.n, 0x7FFFFFFFu));
  if (spill.budget && spill.pool)
    hipLaunchKernelGGL((k_bvh_shape_distance_pool<T>), dim3(std::max(1, std::min((n_est + SDP_Q - 1) / SDP_Q, int(spill.max_blocks)))), dim3(64), 0, st, wk, lv, bv, io, q, spill);
  else if (spill.budget)
    hipLaunchKernelGGL((k_bvh_shape_distance_coop<T>), dim3(std::max(1, std::min(n_est, int(spill.max_blocks)))), dim3(64), 0, st, wk, lv, bv, io, q, spill);
  BvhSplit none;
  memset(&none, 0, sizeof(none));
  BvhParams bp;
  memset(&bp, 0, sizeof(bp));
  launch_shape_finish<T, MESH_UNIT_PART>(grid_finish, st, wk, lv, io, q, bp, none, 1);
}
template <typename T>
void launch_bvh_shape_distance(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q) {
  hipLaunchKernelGGL((k_bvh_shape_distance<T>), dim3(grid), dim3(64), 0, st, wk, lv, bv, io, q);
}
#define HFCL_INST(T)                                                                                                             \
  template void launch_bvh_shape_distance<T>(int, hipStream_t, const Work&, const LibView<T>&, const BvhView<T>&, const IO<T>&, const QParams<T>&);          \
  template void launch_bvh_shape_distance_fast<T>(int, int, hipStream_t, const Work&, const LibView<T>&, const BvhView<T>&, const IO<T>&, const QParams<T>&, BvhSpill);
HFCL_INST(float)
HFCL_INST(double)
#undef HFCL_INST
