// hfcl_k_bvhc.hip -- BVHModel<OBBRSS> x convex solid collide() (hfcl_k_bvhc.o), WITHOUT contraction of a*b+c (Makefile: FLAGS_k_bvhc):
// every inlined copy of a leaf, of the fit of the solid's box and of the box tests is then the same arithmetic, and the forms of the walk
// write the same bytes.  The lanes' walk, its task levels and the walk in rounds are templates this object shares with mesh x mesh
// collide() (hfcl_mesh_collide.hpp, which also says what keeps the mesh objects' kernels apart); here: the 16-lane group kernel, the fit
// of the solids' boxes, the waves' continuation, the listed leaves and the launchers.  Mesh x solid distance() is hfcl_k_bvhs.hip.
#include "hfcl_mesh_collide.hpp"

constexpr int MESH_UNIT_PART = 3;  // what this object's copy of a kernel two mesh objects launch carries (hfcl_mesh_collide.hpp); named once, passed explicitly below

// ---------------------------------------------------------------------------------------
// k_bvh_shape: BVHModel<OBBRSS> x convex solid collide(), either operand order.  One query per BS_W-lane
// group (hfcl_bvh_shape.hpp: sequential traversal, the group's lanes share support scans and EPA face
// work); DFS stack and the full-capacity polytope of each group in LDS.
// ---------------------------------------------------------------------------------------

template <typename T>
__global__ void __launch_bounds__(64) k_bvh_shape(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q, BvhParams bp,
                                                  T break_distance2) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<T, EPA_MAX_ITER> scratch[G];
  __shared__ uint32_t stacks[G][BS_STACK];  // 32-bit node ids: models of any size
  const uint32_t cnt = wk.counts[B_BVHSHAPE];
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint32_t it = blockIdx.x * G + grp; it < cnt; it += gridDim.x * G) {
    const uint32_t pair = wk.lists[size_t(B_BVHSHAPE) * wk.n + it];
    const DShape<T> a = lib.shapes[wk.shape1[pair]], b = lib.shapes[wk.shape2[pair]];
    const bool swapped = a.kind != K_BVH;  // (shape, BVH): collide(o2, o1) then swapObjects (collision.cpp:93-108)
    const DShape<T> ms = swapped ? b : a;
    GroupSolid<T> solid;
    solid.s = swapped ? a : b;
    solid.v = lib.verts + 3 * size_t(solid.s.vertex_offset);
    solid.lig = lig;
    if (solid.s.kind == K_CONVEX && solid.s.num_points <= uint32_t(HULL_MAX)) solid.h.load(solid.v, solid.s.num_points, lig);
    const Pose<T> tf1 = load_pose(io.tf1, pair), tf2 = load_pose(io.tf2, pair);
    const Pose<T> tfm = swapped ? tf2 : tf1, tfs = swapped ? tf1 : tf2;
    const DMesh m = bv.meshes[ms.bvh_index];
    MeshShapeState<T> st;
    auto on_contact = [&](int prim, T distance, const V3<T>& p1, const V3<T>& p2, const V3<T>& nn) {
      if (lig != 0 || !bp.contacts) return;
      const uint32_t slot = atomicAdd(bp.contacts_count, 1u);
      if (slot >= bp.contacts_cap) return;
      hfcl_contact c;
      c.pair = pair;
      c.b1 = swapped ? -1 : prim;
      c.b2 = swapped ? prim : -1;
      c._pad = 0;
      c.penetration_depth = double(distance);
      const V3<T> a1 = swapped ? p2 : p1, a2 = swapped ? p1 : p2, an = swapped ? -nn : nn;
      c.normal[0] = an.x; c.normal[1] = an.y; c.normal[2] = an.z;
      c.p1[0] = a1.x; c.p1[1] = a1.y; c.p1[2] = a1.z;
      c.p2[0] = a2.x; c.p2[1] = a2.y; c.p2[2] = a2.z;
      bp.contacts[slot] = c;
    };
    mesh_shape_collide<T, LaneGroup<BS_W>>(bv.nodes + m.node_off, bv.verts + 3 * size_t(m.vert_off), bv.tris + 3 * size_t(m.tri_off),
                                           tfm, solid.s, lib.verts, tfs, solid, q, bp.num_max_contacts, break_distance2,
                                           stacks[grp], BS_STACK, &scratch[grp], initial_guess<T>(io, q, pair), on_contact, st);
    if (lig == 0) {
      if (st.unsupported) {
        auto r = io.out[pair];
        memset(&r, 0, sizeof(r));
        r.status = 0x80000000u;
        io.out[pair] = r;
      } else {
        PairOut<T> o;
        o.distance = st.rec_dist;
        o.normal = (swapped && st.nn.x == st.nn.x) ? -st.nn : st.nn;  // (no witness: the one NaN of every form, not its negative)
        o.p1 = swapped ? st.np2 : st.np1;
        o.p2 = swapped ? st.np1 : st.np2;
        o.gjk_status = GJK_DID_NOT_RUN;
        o.epa_status = EPA_DID_NOT_RUN;
        o.gjk_iters = o.epa_iters = 0;
        store_bvh_record(io, pair, o, st.ncontacts, swapped ? -1 : st.first_prim, swapped ? st.first_prim : -1, st.overflow);
        write_guess<T>(io, pair, st.guess, 0, 0);
      }
    }
    LaneGroup<BS_W>::sync();
  }
}

// ---------------------------------------------------------------------------------------
// Mesh x solid, one query per lane (k_bvh_collide<T, false, false, SOLID>): the two kernels around the walk.
// k_shape_obb: computeBV<OBBRSS, S>(solid, tf) per query -- the reference's PCA fit of the solid's bound vertices in
// world frame (Jacobi sweeps; hfcl_bvh_shape.hpp: shape_obb) -- and its products with the mesh pose (ObbQuery), by
// pair, so that the walk (and every task a long query is cut into) starts from 15 loaded numbers.
// k_bvh_shape_finish: the leaves that needed EPA, one per BS_W-lane group with the full-capacity polytope in LDS, after
// the walk and its fold-back: a leaf whose unit was not overtaken by an earlier contact (bvh_moot) is the query's contact;
// its depth is compared with the bound the record holds (updateDistanceLowerBoundFromLeaf) and patched in.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_shape_obb(Work wk, LibView<T> lib, IO<T> io) {
  const uint32_t cnt = wk.counts[B_BVHSHAPE];
  ObbQuery<T>* const table = reinterpret_cast<ObbQuery<T>*>(wk.shape_oq);
  for (uint32_t it = blockIdx.x * blockDim.x + threadIdx.x; it < cnt; it += gridDim.x * blockDim.x) {
    const uint32_t pair = wk.lists[size_t(B_BVHSHAPE) * wk.n + it];
    const uint32_t id1 = wk.shape1[pair], id2 = wk.shape2[pair];
    const bool swapped = lib.kinds[id1] != uint8_t(K_BVH);
    const DShape<T> shape = lib.shapes[swapped ? id1 : id2];
    const Pose<T> tf1 = load_pose(io.tf1, pair), tf2 = load_pose(io.tf2, pair);
    DNode<T> bv2;
    ObbQuery<T> oq;
    if (shape_obb(shape, lib.verts, swapped ? tf1 : tf2, bv2)) {
      oq = make_obb_query(swapped ? tf2 : tf1, bv2);
    } else {
      const T nanv = Lim<T>::nan();
      oq.M.r0 = oq.M.r1 = oq.M.r2 = oq.V = oq.ext = mk<T>(nanv, nanv, nanv);
    }
    table[pair] = oq;
  }
}

// ---------------------------------------------------------------------------------------
// k_bvh_shape_coop: the long walks of a mesh x solid batch, ONE LANE GROUP PER QUERY, COOP_W entries of the stack at a time.
// k_bvh_collide<SOLID> suspends a query after its step budget and leaves its stack (DFS order) and its state (bounds, witness)
// behind; here a group of COOP_W lanes takes the query over and goes on with the SAME sequential walk, COOP_W entries wide:
// the top entries of the (ordered, LDS) stack are popped together, each lane tests its entry's box or runs its triangle's
// leaf, and the results are applied in stack order by scans over the group --
//   * the bound after entry i is the minimum of the bound before the window and the values of entries <= i (exclusive
//     prefix minimum): "this leaf lowered the bound when it was visited" is val_i < that, the witness is the LAST such leaf,
//     the recorded distance belongs to the FIRST entry that reaches the window's minimum (later ties do not lower it);
//   * the first entry with a contact ends the walk, entries behind it are void (their EPA items are marked so);
//   * the children of the overlapping boxes take their parents' places, in order -- and only the entries in FRONT of the
//     window's first overlapping box are visited in a trip (what the others do to the state depends on that box's subtree).
// So the walk visits exactly the reference's sequence, up to COOP_W steps per trip instead of one, and ends with the query's
// record: no task levels, no fold-back.  A step of a lone lane costs ~2 us and a level of tasks its budget times that; a
// trip of this kernel costs one step's latency for COOP_W of them.  Groups take the next suspended query as they finish.
// ---------------------------------------------------------------------------------------
#ifndef HFCL_WPE_SHAPE_COOP
#define HFCL_WPE_SHAPE_COOP 2
#endif
// What a walk of k_bvh_shape_coop and the leaf it calls share, in LDS (round 6).  The leaf's GJK takes 248 registers, so whatever the
// walk holds across the call goes to scratch memory and back: as first built -- the walk's state in registers, the leaf's arguments a
// by-value block, its result a block behind a pointer, the request's parameters behind another -- that was 608 B per lane, and 100 000
// queries moved 6.4 GB through it (a read-only tree walk whose records are 9.6 MB; profiles/r05 traffic_cfg4s.json): more than the
// XCD's L2 holds for its resident waves, so the kernel ran at half the chip's memory bandwidth.  Here the call passes two words per lane
// (the triangle, a flag) and returns three; everything that is the same for the lanes of a walk -- where the model's arrays are, the
// query, the solid, the request, the solid's OBB products, the witness of the walk's bound -- is in this block, and a leaf's witness
// goes to a lane-minor slab beside it.
template <typename T>
struct ShapeCoopCtx {
  const T* mesh_verts;      // of the walk's model
  const uint32_t* tris;
  const DShape<T>* shapes;
  const T* lib_verts;
  decltype(IO<T>::tf1) pose_m;  // pose arrays of the mesh / the solid
  decltype(IO<T>::tf1) pose_s;
  ShapeDeferItem<T>* defer;
  uint32_t* defer_count;
  T* wit;                   // [9][64]: p1, p2, n of the leaf each lane ran last
  uint32_t defer_cap;
  uint32_t pair, solid_id, parent, order;
  V3<T> guess0;
  QParams<T> q;
  ObbQuery<T> oq;
  V3<T> np1, np2, nn;       // witness of the walk's bound (record orientation)
};
template <typename T>
struct CoopLeafRet {
  T distance;
  uint32_t to_epa, slot;
};
// (not_tail_called: LLVM marks a call that hands no pointer into the caller's frame as a possible tail call, and a function with such a call
// site keeps the convention's callee-saved registers -- 50 of them here, saved and restored around every leaf, 200 B of scratch per lane;
// without the mark the register allocation is interprocedural and the callee saves nothing the walk does not hold)
template <typename T, class PS>
__device__ __noinline__ __attribute__((not_tail_called)) CoopLeafRet<T> coop_solid_leaf(const ShapeCoopCtx<T>* c, const PS ps, uint32_t prim, uint32_t push) {
  const QParams<T> q = c->q;
  const T* const mv = c->mesh_verts;
  const uint32_t* const tri = c->tris + 3 * size_t(prim);
  auto vtx = [&](uint32_t i) { return mk<T>(mv[3 * size_t(i)], mv[3 * size_t(i) + 1], mv[3 * size_t(i) + 2]); };
  const V3<T> ta = vtx(tri[0]), tb = vtx(tri[1]), tc = vtx(tri[2]);
  LaneSolid<T> solid;
  solid.s = c->shapes[c->solid_id];
  solid.v = c->lib_verts + 3 * size_t(solid.s.vertex_offset);
  const uint32_t pair = c->pair;
  auto tfm_of = [&]() { return load_pose(c->pose_m, pair); };
  auto tfs_of = [&]() { return load_pose(c->pose_s, pair); };
  const MDiff<T> sMt = make_mdiff(tfs_of(), tfm_of());
  V3<T> guess = c->guess0;
  ShapeDeferItem<T> item;
  CoopLeafRet<T> r;
  r.distance = Lim<T>::max();
  r.slot = 0u;
  V3<T> p1 = mk<T>(T(0), T(0), T(0)), p2 = p1, n = p1;
  const bool to_epa = mesh_shape_leaf_lane(ta, tb, tc, sMt, tfm_of, tfs_of, solid.s, solid, swept_radius(solid.s), q, guess, ps, r.distance, p1, p2, n, item);
  r.to_epa = to_epa ? 1u : 0u;
  if (to_epa) {
    r.distance = Lim<T>::max();
    if (push) {
      item.seed.pair = pair;
      item.prim = prim;
      item.parent = c->parent;
      item.order = c->order;
      item.bound = T(0);
      item.prev_prim = -1;
      const uint32_t slot = atomicAdd(c->defer_count, 1u);
      if (slot < c->defer_cap) c->defer[slot] = item;  // (the host sizes the queue for one item per unit of the batch; never past its end)
      r.slot = slot;
    }
  } else {
    T* const w = c->wit + (threadIdx.x & 63);
    w[0 * 64] = p1.x; w[1 * 64] = p1.y; w[2 * 64] = p1.z;
    w[3 * 64] = p2.x; w[4 * 64] = p2.y; w[5 * 64] = p2.z;
    w[6 * 64] = n.x;  w[7 * 64] = n.y;  w[8 * 64] = n.z;
  }
  return r;
}
template <typename T>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HFCL_WPE_SHAPE_COOP, 8)))
k_bvh_shape_coop(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q, BvhParams bp, T break_distance2, BvhSplit split) {
  constexpr int W = COOP_W, G = 64 / W;
  __shared__ uint32_t stacks[G][COOP_CAP + COOP_SLACK];
  __shared__ T values[G][COOP_CAP + COOP_SLACK];
  __shared__ T w0_slab[W0Lds<T, 64>::WORDS];
  __shared__ ShapeCoopCtx<T> ctxs[G];
  __shared__ T wit_slab[9 * 64];
  const W0Lds<T, 64> leaf_ps{w0_slab + threadIdx.x};
  const int lane = threadIdx.x, grp = lane / W, lig = lane & (W - 1);
  uint32_t* const stack = stacks[grp];
  T* const value = values[grp];
  ShapeCoopCtx<T>& ctx = ctxs[grp];
  const uint64_t gbits = W == 64 ? ~uint64_t(0) : ((uint64_t(1) << (W & 63)) - 1);
  auto gballot = [&](bool x) -> uint64_t { return (__ballot(x) >> (grp * W)) & gbits; };  // the group's lanes, bit 0 = its first lane
  if (lig == 0) {  // what does not change from walk to walk
    ctx.shapes = lib.shapes;
    ctx.lib_verts = lib.verts;
    ctx.defer = reinterpret_cast<ShapeDeferItem<T>*>(wk.shape_defer);
    ctx.defer_count = &wk.counts[CTR_SHAPE_DEFER];
    ctx.defer_cap = wk.shape_defer_cap;
    ctx.wit = wit_slab;
    ctx.q = q;
  }
  // the units of this launch: the suspended queries (level 0), or the chunks the launch before cut its long walks into
  const uint32_t level = split.level;
  const uint32_t unit0 = level ? min(split.ctr[BVH_CTR_LEVEL0 + level - 1], split.cap) : 0u;
  const uint32_t n_units = level ? min(split.ctr[BVH_CTR_LEVEL0 + level], split.cap) - unit0 : min(split.ctr[BVH_CTR_SUSPENDED], split.n_queries);
  if (n_units == 0u) return;  // (nothing suspended / no chunk cut: no wave draws a ticket)
  const unsigned long long cut_ticks = split.can_suspend ? split.cut_ticks : 0u;
  uint32_t* const ticket = &wk.counts[CTR_SHAPE_TICKET];  // (k_bvh_collide<SOLID> is through with it; k_bvh_level_mark has reset it)
  T* const cut_vals = reinterpret_cast<T*>(split.cut_vals);
  const T big = Lim<T>::max();
  // per-group state of the query being walked (uniform over the group's lanes)
  bool have = false, exhausted = false;
  uint32_t pair = 0, solid_id = 0, ncontacts = 0;
  uint32_t unit = 0, my_parent = 0xFFFFFFFFu, my_order = 0;  // where the unit hangs (a chunk: the cut walk's summary slot, its place among the chunks)
  unsigned long long t_begin = 0, t_wave = __builtin_readcyclecounter();
  unsigned n_walks = 0, trip_no = 0;
  (void)t_wave; (void)n_walks;
  bool swapped = false, overflow = false;
  COOP_PROF_DECL;  // [0] trips [1] box-test ticks [2] boxes tested [3] leaf batches [4] their ticks [5] their lanes [6] ticks from the scans to the end of a trip that ends in a contact [7] ticks drawing and loading units
  uint32_t node_off = 0;
  int sp = 0, fb = -1;
  T dlb = big, rec_dist = big, cand_val = big;
  // the witness of lane `l`'s last leaf, from the slab (record orientation)
  auto slab_witness = [&](int l, V3<T>& a1, V3<T>& a2, V3<T>& an) {
    const T* const w = wit_slab + l;
    const int o1 = swapped ? 3 * 64 : 0, o2 = swapped ? 0 : 3 * 64;  // (rows, not a select between two structs: that one goes through an indexed stack slot)
    const T sg = swapped ? T(-1) : T(1);
    a1 = mk<T>(w[o1], w[o1 + 64], w[o1 + 128]);
    a2 = mk<T>(w[o2], w[o2 + 64], w[o2 + 128]);
    an = mk<T>(sg * w[6 * 64], sg * w[7 * 64], sg * w[8 * 64]);
  };
  for (;;) {
    if (!have && !exhausted) {
      COOP_PROF_T0;
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
      pair = wave_uniform<W>(u.pair);
      unit = wave_uniform<W>(u.index);
      my_parent = wave_uniform<W>(u.parent);
      my_order = wave_uniform<W>(u.order);
      const uint32_t id1 = wave_uniform<W>(wk.shape1[pair]), id2 = wave_uniform<W>(wk.shape2[pair]);
      swapped = wave_uniform<W>(int(lib.kinds[id1] != uint8_t(K_BVH))) != 0;
      solid_id = swapped ? id1 : id2;
      {
        const DMesh mm = bv.meshes[wave_uniform<W>(lib.shapes[swapped ? id2 : id1].bvh_index)];
        node_off = wave_uniform<W>(mm.node_off);
        if (lig == 0) {
          ctx.mesh_verts = bv.verts + 3 * size_t(mm.vert_off);
          ctx.tris = bv.tris + 3 * size_t(mm.tri_off);
          ctx.pose_m = swapped ? io.tf2 : io.tf1;
          ctx.pose_s = swapped ? io.tf1 : io.tf2;
          ctx.pair = pair;
          ctx.solid_id = solid_id;
          ctx.parent = u.parent;
          ctx.order = u.order;
          ctx.oq = reinterpret_cast<const ObbQuery<T>*>(wk.shape_oq)[pair];
          ctx.np1 = s.np1;
          ctx.np2 = s.np2;
          ctx.nn = s.nn;
          ctx.guess0 = initial_guess<T>(io, q, pair);  // (walks whose leaves hand a cached guess on are not split)
        }
      }
      if (level) {  // the chunk's entries, with what is known about them
        for (uint32_t j = uint32_t(lig); j < s.n_child; j += uint32_t(W)) {
          stack[s.n_child - 1u - j] = split.cut_words[s.first_child + j];
          value[s.n_child - 1u - j] = cut_vals[s.first_child + j];
        }
      } else {
        for (uint32_t j = uint32_t(lig); j < s.n_child; j += uint32_t(W)) stack[s.n_child - 1u - j] = split.tasks[s.first_child + j].entry;  // child 0 on top
      }
      sp = wave_uniform<W>(int(s.n_child));
      dlb = wave_uniform<W>(s.dlb);
      rec_dist = wave_uniform<W>(s.rec_dist);
      cand_val = wave_uniform<W>(s.cand_val);
      t_begin = __builtin_readcyclecounter();
      ++n_walks;
      fb = -1;
      ncontacts = 0;
      overflow = wave_uniform<W>(int((s.flags & BVH_SUM_OVERFLOW) != 0)) != 0 || sp > COOP_CAP;
      if (overflow) sp = 0;
      have = true;
      }
      COOP_PROF_DT(7);
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
      const uint32_t ew = act ? stack[sp - 1 - lig] : 0u;
      T val = act ? value[sp - 1 - lig] : big;  // (meaningful for tagged entries only)
      sp -= w;
      const uint32_t e = ew & COOP_NODE;
      uint32_t tag = ew & ~COOP_NODE;
      // (1) entries nothing is known about yet: a box is tested -- an overlapping one only refines the stack (its children
      // take its place, at any position), a disjoint one keeps its bound; a triangle waits for the leaf batch
      const DNode<T>* const np = bv.nodes + node_off + e;
      int32_t fc = 0;
      bool overlap = false, pending = false;
      COOP_PROF_ADD(0, 1);
      COOP_PROF_ADD(2, __popcll(__ballot(act && tag == 0u)));
      COOP_PROF_ADD(12, __popcll(__ballot(act)));                          // window entries
      COOP_PROF_ADD(13, __popcll(__ballot(act && tag == COOP_DISJOINT)));  // ... boxes found disjoint, waiting for their visit
      COOP_PROF_ADD(14, __popcll(__ballot(act && (tag == COOP_LEAF || tag == COOP_LEAF_EPA))));  // ... evaluated triangles, waiting
      COOP_PROF_ADD(15, sp + w);                                           // stack depth
      COOP_PROF_T0;
      if (act && tag == 0u) {
        const DNode<T> n1 = *np;  // (the whole record at once: a leaf's box is read for nothing, an inner node's not a latency later)
        fc = n1.first_child;
        if (fc >= 0) {
          T sq;
          const ObbQuery<T> oq = ctx.oq;
          if (obb_disjoint_q(oq, n1, q.security_margin, break_distance2, sq)) {
            val = hsqrt(sq);
            tag = COOP_DISJOINT;
          } else {
            overlap = true;
          }
        } else {
          pending = true;
        }
      }
      COOP_PROF_DT(1);
      // (2) the triangles, when enough of them wait or the window has nothing left to split
      bool fresh = false;  // this lane ran its leaf in this trip (the slab holds its witness)
      {
        const uint64_t pmask = gballot(pending);
        if (pmask && (__popcll(pmask) >= HFCL_COOP_LEAF_BATCH || !gballot(overlap))) {
          COOP_PROF_ADD(3, 1);
          COOP_PROF_ADD(5, __popcll(pmask));
          COOP_PROF_T0;
          if (pending) {
            const CoopLeafRet<T> r = coop_solid_leaf<T>(&ctx, leaf_ps, uint32_t(-(fc + 1)), 0u);
            val = r.distance;
            tag = r.to_epa ? COOP_LEAF_EPA : COOP_LEAF;
            pending = false;
            fresh = true;
          }
          COOP_PROF_DT(4);
        }
      }
      // (3) what an entry does to the walk's state depends on everything before it in DFS order -- which includes the subtrees of
      // overlapping boxes and the triangles still waiting ahead of it: the entries in front of the first of those are visited now
      COOP_PROF_T0;
      const uint64_t block = gballot(overlap || pending);
      const int f = block ? __ffsll((unsigned long long)block) - 1 : W;
      COOP_PROF_ADD(16, __popcll(gballot(pending)));  // unevaluated triangles left waiting for a batch
      COOP_PROF_ADD(17, min(f, w));                   // entries visited
      bool visit = act && lig < f;
      const bool is_leaf = tag == COOP_LEAF || tag == COOP_LEAF_EPA;
      T bnd = big, recv = big;  // what this entry sets the bound to, and the recorded distance that goes with it
      bool contact = false;
      if (visit) {
        if (tag == COOP_DISJOINT) {  // updateDistanceLowerBoundFromBV
          bnd = val;
          recv = val + q.security_margin;
        } else if (tag == COOP_LEAF) {  // updateDistanceLowerBoundFromLeaf
          bnd = val - q.security_margin;
          recv = val;
          contact = bnd <= q.collision_distance_threshold;
        } else {
          contact = true;  // (needs EPA: a contact on the host's word)
        }
      }
      const uint64_t cmask = gballot(contact);
      const int c = cmask ? __ffsll((unsigned long long)cmask) - 1 : W;  // the first contact in stack order ends the walk
      visit = visit && lig <= c;
      if (!visit) bnd = big;
      const T before = hmin(dlb, group_min_excl_scan<T, W>(bnd, lig, big));  // the bound as entry `lig` found it
      const bool lowered = visit && bnd < before;
      const T wmin = group_min_all<T, W>(bnd);
      if (gballot(lowered)) {
        // the bound ends at the minimum of the visited entries, set by the first of them that reaches it
        const int src = __ffsll((unsigned long long)gballot(visit && bnd == wmin)) - 1;
        dlb = wave_uniform<W>(wmin);
        rec_dist = wave_uniform<W>(__shfl(recv, src, W));
      }
      // the witness: the last triangle that lowered the bound on its visit (its points, if it was evaluated in an earlier trip,
      // by running its leaf once more); the contact's points likewise
      const uint64_t wmask = gballot(lowered && tag == COOP_LEAF);
      const int L = wmask ? 63 - __clzll((unsigned long long)wmask) : -1;
      if (L >= 0) cand_val = wave_uniform<W>(__shfl(bnd, L, W));
      const bool is_contact_lane = c < W && lig == c;
      COOP_PROF_DT(8);
      COOP_PROF_T0;
      if (act && is_leaf && !fresh && ((lig == L) || (is_contact_lane && tag == COOP_LEAF && bp.contacts))) {
        fc = np->first_child;
        coop_solid_leaf<T>(&ctx, leaf_ps, uint32_t(-(fc + 1)), 0u);  // (for its witness: the slab)
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (L >= 0 && lig == 0) slab_witness(grp * W + L, ctx.np1, ctx.np2, ctx.nn);
      if (c < W) {  // canStop()
        if (act && is_leaf && fc == 0) fc = np->first_child;
        const int prim_c = wave_uniform<W>(__shfl(int(-(fc + 1)), c, W));
        fb = prim_c;
        ncontacts = 1;
        bool lost = false;
        if (is_contact_lane) {
          if (tag == COOP_LEAF_EPA) {  // its leaf once more, this time with the EPA item (k_bvh_shape_finish patches the record)
            const CoopLeafRet<T> r = coop_solid_leaf<T>(&ctx, leaf_ps, uint32_t(prim_c), 1u);
            lost = r.slot >= wk.shape_defer_cap;
          } else if (bp.contacts) {
            const T* const w = wit_slab + lane;  // (its leaf ran in this trip, above at the latest)
            emit_shape_contact(bp, pair, swapped, prim_c, val, mk<T>(w[0 * 64], w[1 * 64], w[2 * 64]), mk<T>(w[3 * 64], w[4 * 64], w[5 * 64]),
                               mk<T>(w[6 * 64], w[7 * 64], w[8 * 64]));
          }
        }
        // (the host sizes the queue of EPA items for the units it expects -- one and a half per query once walks are cut into chunks --;
        // a contact whose item found it full says so in its record instead of keeping a depth nobody computed)
        if (gballot(lost)) overflow = true;
        sp = 0;
        COOP_PROF_DT(6);
      } else {
        // (4) the stack again, in order (entry 0's successors on top): visited entries are gone, an overlapping box is its two
        // children (left above right), everything else stays with what is known about it
        COOP_PROF_DT(9);  // (the witness part of a trip without a contact)
        COOP_PROF_T0;
        const int cnt = !act || lig < f ? 0 : (overlap ? 2 : 1);
        const uint64_t m2 = gballot(cnt == 2), m1b = gballot(cnt == 1);
        const uint64_t deeper = ~((uint64_t(2) << lig) - 1);  // window entries behind this one (pushed first)
        const int pos = sp + 2 * __popcll(m2 & deeper) + __popcll(m1b & deeper);
        if (cnt == 2) {
          stack[pos] = uint32_t(fc) + 1u;
          stack[pos + 1] = uint32_t(fc);
        } else if (cnt == 1) {
          stack[pos] = e | tag;
          value[pos] = val;
        }
        sp += 2 * __popcll(m2) + __popcll(m1b);
        if (sp > COOP_CAP + COOP_SLACK - 2) {  // a tree deeper than the slack on top of a full stack: flagged, never written past the block
          overflow = true;
          sp = 0;
        }
      }
      done = sp == 0;
      if (done) COOP_PROF_T0; else COOP_PROF_DT(10);
      // (cutting sooner once the launch's ticket has run out -- nothing left to draw, idle slots waiting -- was measured: 3.10 -> 5.9 / 7.2 / 8.0 ms
      // with 150k / 80k / 40k ticks: the three launches are all the levels there are, and what the early cuts leave for the last one is long)
      if (cut_ticks && sp > COOP_CHUNK && __builtin_readcyclecounter() - t_begin > cut_ticks) {
        // ---- the walk has had its time: what is left of it becomes chunks for the next launch (coop_cut)
        if (coop_cut<T, W>(split, level ? split.n_queries + unit0 + unit : unit, pair, my_parent, my_order, stack, value, sp, lig, dlb, rec_dist, cand_val,
                           ctx.np1, ctx.np2, ctx.nn, overflow)) {
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
        coop_write_sum<T>(split, split.n_queries + unit0 + unit, dlb, rec_dist, cand_val, ctx.np1, ctx.np2, ctx.nn, swapped ? -1 : fb, swapped ? fb : -1, ncontacts, 0u, 0u,
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
        o.normal = ctx.nn;
        o.p1 = ctx.np1;
        o.p2 = ctx.np2;
        o.gjk_status = GJK_DID_NOT_RUN;
        o.epa_status = EPA_DID_NOT_RUN;
        o.gjk_iters = o.epa_iters = 0;
        store_bvh_record(io, pair, o, ncontacts, swapped ? -1 : fb, swapped ? fb : -1, overflow);
      }
      COOP_WALK_END(lig == 0, t_begin);
      have = false;
      COOP_PROF_DT(11);
    }
  }
  COOP_PROF_FLUSH;
  COOP_WAVE_END(t_wave, n_walks);
}

// k_shape_leaves: k_tri_leaves (hfcl_k_bvh.hip) for mesh x solid -- every triangle the round's walks listed against its solid, one per lane, through the
// solid_leaf_call of k_bvh_collide's SOLID form (internal/traversal_node_bvh_shape.h:139-188).  A leaf whose GJK ends inside the solid
// (it needs EPA: a contact whatever EPA finds, mesh_shape_lane_request) is marked by its distance (WALK_LEAF_EPA) -- nothing else of it is
// read --; redo = 1: the leaves k_bvh_resolve found to END their walks that way (wa.redo, their number at ctr[5]) once more, this time with
// the EPA item queued for k_bvh_shape_finish (as k_bvh_shape_coop does with the leaf that ends a walk of its own).
// The listed leaves ordered by the kind of their solid (WalkArgs::perm: position -> item), so that the 64 leaves of a wave of k_shape_leaves run ONE
// support function: in the order the walks listed them a wave held all six kinds of cfg4s and ran their GJK loops one after the other (953 waves:
// 440 us; profiles/r06_g).  Two launches: the kinds and their histogram (hist[16], zeroed by the host), then the scatter (cursor = hist + 16).
template <typename T>
__device__ __forceinline__ uint32_t item_kind(const Work& wk, const LibView<T>& lib, const WalkRec<T>* recs, uint32_t code) {
  const uint32_t pair = recs[code & 0x0FFFFFFFu].pair;
  const uint32_t id1 = wk.shape1[pair], id2 = wk.shape2[pair];
  const uint32_t k1 = lib.kinds[id1];
  return (k1 != uint32_t(K_BVH) ? k1 : uint32_t(lib.kinds[id2])) & 15u;
}
template <typename T>
__global__ void __launch_bounds__(256) k_item_kinds(Work wk, LibView<T> lib, WalkArgs wa, int redo) {
  __shared__ uint32_t h[16];
  const WalkRec<T>* const recs = reinterpret_cast<const WalkRec<T>*>(wa.recs);
  const uint32_t n_items = redo ? min(wa.ctr[8 * wa.round + 5], wa.list_stride) : min(wa.ctr[8 * wa.round + 1], wa.item_cap);
  uint32_t* const hist = wa.hist + (redo ? 32 : 0);
  if (threadIdx.x < 16) h[threadIdx.x] = 0u;
  __syncthreads();
  for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < n_items; it += gridDim.x * 256u) atomicAdd(&h[item_kind(wk, lib, recs, redo ? wa.redo[it] : wa.items[it])], 1u);
  __syncthreads();
  if (threadIdx.x < 16 && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
template <typename T>
__global__ void __launch_bounds__(256) k_item_scatter(Work wk, LibView<T> lib, WalkArgs wa, int redo) {
  __shared__ uint32_t h[16], base[16];
  const WalkRec<T>* const recs = reinterpret_cast<const WalkRec<T>*>(wa.recs);
  const uint32_t n_items = redo ? min(wa.ctr[8 * wa.round + 5], wa.list_stride) : min(wa.ctr[8 * wa.round + 1], wa.item_cap);
  uint32_t* const hist = wa.hist + (redo ? 32 : 0);
  uint32_t* const cursor = hist + 16;
  uint32_t* const perm = redo ? wa.perm + wa.item_cap : wa.perm;
  for (uint32_t it0 = blockIdx.x * 256u; it0 < n_items; it0 += gridDim.x * 256u) {
    if (threadIdx.x < 16) h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t it = it0 + threadIdx.x;
    uint32_t kind = 0, rank = 0;
    if (it < n_items) {
      kind = item_kind(wk, lib, recs, redo ? wa.redo[it] : wa.items[it]);
      rank = atomicAdd(&h[kind], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 16) {
      uint32_t start = 0;
      for (uint32_t k = 0; k < threadIdx.x; ++k) start += hist[k];
      base[threadIdx.x] = start + (h[threadIdx.x] ? atomicAdd(&cursor[threadIdx.x], h[threadIdx.x]) : 0u);
    }
    __syncthreads();
    if (it < n_items) perm[base[kind] + rank] = it;
    __syncthreads();
  }
}
template <typename T, bool REDO>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 8)))
k_shape_leaves(Work wk, LibView<T> lib, BvhView<T> bv, IO<T> io, QParams<T> q, WalkArgs wa) {
  __shared__ T w0_slab[W0Lds<T, 64>::WORDS];
  const W0Lds<T, 64> leaf_ps{w0_slab + threadIdx.x};
  const WalkRec<T>* const recs = reinterpret_cast<const WalkRec<T>*>(wa.recs);
  TriLeafOut<T>* const res = reinterpret_cast<TriLeafOut<T>*>(wa.res);
  const uint32_t n_items = REDO ? min(wa.ctr[8 * wa.round + 5], wa.list_stride) : min(wa.ctr[8 * wa.round + 1], wa.item_cap);
  for (uint32_t base = blockIdx.x * 64u; base < n_items; base += gridDim.x * 64u) {
    if (base + threadIdx.x < n_items) {
      const uint32_t it = wa.perm ? (REDO ? wa.perm + wa.item_cap : wa.perm)[base + threadIdx.x] : base + threadIdx.x;
      const uint32_t item_code = REDO ? wa.redo[it] : wa.items[it];
      const WalkRec<T>* const r = recs + (item_code & 0x0FFFFFFFu);
      const uint32_t s2 = item_code >> 28, pair = r->pair, prim = r->leaf1[s2];
      const uint32_t id1 = wk.shape1[pair], id2 = wk.shape2[pair];
      const bool swapped = lib.kinds[id1] != uint8_t(K_BVH);
      const uint32_t solid_id = swapped ? id1 : id2;
      const DMesh m1 = bv.meshes[lib.shapes[swapped ? id2 : id1].bvh_index];
      // the leaf INLINE (the same mesh_shape_leaf_lane as solid_leaf_call's: here no walk shares the lane's registers with it, and a call's
      // argument block and saved registers were 320 B of scratch per lane -- 230 MB written per 100k cfg4s queries)
      const uint32_t* const t3 = bv.tris + 3 * size_t(m1.tri_off + prim);
      const T* const mv = bv.verts + 3 * size_t(m1.vert_off);
      auto vtx = [&](uint32_t i) { return mk<T>(mv[3 * size_t(i)], mv[3 * size_t(i) + 1], mv[3 * size_t(i) + 2]); };
      const V3<T> ta = vtx(t3[0]), tb = vtx(t3[1]), tc = vtx(t3[2]);
      LaneSolid<T> solid;
      solid.s = lib.shapes[solid_id];
      solid.v = lib.verts + 3 * size_t(solid.s.vertex_offset);
      auto tfm_of = [&]() { return load_pose(swapped ? io.tf2 : io.tf1, pair); };
      auto tfs_of = [&]() { return load_pose(swapped ? io.tf1 : io.tf2, pair); };
      const MDiff<T> sMt = make_mdiff(tfs_of(), tfm_of());  // Transform3f::inverseTimes: the mesh frame in the solid's frame
      V3<T> guess = initial_guess<T>(io, q, pair);  // (split walks start every leaf from the request's guess)
      ShapeDeferItem<T> item;
      TriLeafOut<T> tlo;
      const bool to_epa = mesh_shape_leaf_lane(ta, tb, tc, sMt, tfm_of, tfs_of, solid.s, solid, swept_radius(solid.s), q, guess, leaf_ps, tlo.distance, tlo.p1, tlo.p2, tlo.n, item);
      if constexpr (REDO) {
        if (to_epa) {  // (always: the resolve kernel listed the leaf because this run's twin said so)
          item.seed.pair = pair;
          item.prim = prim;
          item.parent = 0xFFFFFFFFu;
          item.order = 0u;
          item.bound = T(0);
          item.prev_prim = -1;
          const uint32_t slot = atomicAdd(&wk.counts[CTR_SHAPE_DEFER], 1u);
          if (slot < wk.shape_defer_cap) reinterpret_cast<ShapeDeferItem<T>*>(wk.shape_defer)[slot] = item;
        }
      } else {
        if (to_epa) tlo.distance = walk_leaf_epa<T>();
        res[it] = tlo;
      }
    }
  }
}

// =======================================================================================
// launchers (hfcl_launch.hpp), over the level launches of hfcl_mesh_collide.hpp
// =======================================================================================
template <typename T>
void launch_bvh_shape(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, const BvhParams& bp, T break_distance2) {
  hipLaunchKernelGGL((k_bvh_shape<T>), dim3(grid), dim3(64), 0, st, wk, lv, bv, io, q, bp, break_distance2);
}
// one launch of the lane walk: the narrow form, 32-bit node ids in the entry
template <typename T>
static void launch_collide_solid(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, const BvhParams& bp, T break_distance2, const BvhSplit& split, const BvhSpill& spill) {
  hipLaunchKernelGGL((k_bvh_collide<T, false, false, true>), dim3(grid), dim3(BVH_BLOCK), 0, st, wk, lv, bv, io, q, bp, break_distance2, split, spill);
}
// mesh x solid collide(), one query per lane: the solids' OBBs, the walk (split as `split` says), the EPA leaves
template <typename T>
void launch_bvh_shape_fast(int grid, int grid_finish, int coop_grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, const BvhParams& bp, T break_distance2, BvhSplit split, BvhSpill spill, const AsideStream* aside) {
  hipLaunchKernelGGL((k_shape_obb<T>), dim3(std::max(1, grid / 2)), dim3(256), 0, st, wk, lv, io);
  spill.wide = 0;
  spill.slab = nullptr;
  const bool splitting = bvh_splitting(split, bp);
  if (!splitting) split.tasks = nullptr;
  if (splitting && split.coop) {
    // the queries for their step budget, one per lane; then the suspended ones, one per wave and 64 entries at a time
    BvhSplit s0 = split;
    s0.level = 0;
    s0.budget = split.budget0;
    s0.can_suspend = 1;
    if (split.walk.recs && split.walk_rounds) {
      // the queries' own phase as walk (its leaves listed) / leaves (one per lane, dense) / resolve (hfcl_dev.hpp: WalkRec), as mesh x mesh;
      // then the leaves that ended a walk needing EPA once more, for their items
      WalkArgs wa = split.walk;
      wa.round = 0;
      wa.k = std::min<uint32_t>(split.walk_k[0], uint32_t(WALK_K));
      wa.budget = split.walk_budget[0];
      wa.last = 1u;
      wa.list_out = wa.list_in + wa.list_stride;
      const int lgrid = std::max(1, std::min(grid * 2, 2048));
      const int sgrid = std::max(1, std::min(grid, 512));
      hipLaunchKernelGGL((k_bvh_walk<T, true>), dim3(grid), dim3(BVH_BLOCK), 0, st, wk, lv, bv, io, q, break_distance2, wa);
      if (wa.perm) {
        hipLaunchKernelGGL((k_item_kinds<T>), dim3(sgrid), dim3(256), 0, st, wk, lv, wa, 0);
        hipLaunchKernelGGL((k_item_scatter<T>), dim3(sgrid), dim3(256), 0, st, wk, lv, wa, 0);
      }
      hipLaunchKernelGGL((k_shape_leaves<T, false>), dim3(lgrid), dim3(64), 0, st, wk, lv, bv, io, q, wa);
      hipLaunchKernelGGL((k_bvh_resolve<T, true>), dim3(std::max(1, std::min(grid, 1024))), dim3(256), 0, st, wk, lv, io, q, s0, wa);
      if (wa.perm) {
        hipLaunchKernelGGL((k_item_kinds<T>), dim3(std::max(1, sgrid / 8)), dim3(256), 0, st, wk, lv, wa, 1);
        hipLaunchKernelGGL((k_item_scatter<T>), dim3(std::max(1, sgrid / 8)), dim3(256), 0, st, wk, lv, wa, 1);
      }
      hipLaunchKernelGGL((k_shape_leaves<T, true>), dim3(lgrid), dim3(64), 0, st, wk, lv, bv, io, q, wa);
    } else {
      launch_collide_solid<T>(grid, st, wk, lv, bv, io, q, bp, break_distance2, s0, spill);
    }
    // (the EPA item of a chunk that stands behind another chunk's contact is skipped: bvh_moot over the summaries; items of whole walks
    // hang under no summary)
    BvhSplit fin = s0;
    fin.level = 0;
    // The items of whole walks -- all that k_bvh_collide<SOLID> and the first launch of k_bvh_shape_coop queue -- are final when that launch
    // ends: their EPA runs on the helper stream beside the two launches that walk the chunks (few waves, as long as their longest chains:
    // 0.54 ms of cfg4s's 3.45, and k_bvh_shape_finish another 0.52 behind them before; profiles/r05_f).
    bool forked = false;
    const bool cut = launch_coop_levels<T, MESH_UNIT_PART>(grid, st, wk, io, s0, int(CTR_SHAPE_TICKET), [&](const BvhSplit& s) {
      hipLaunchKernelGGL((k_bvh_shape_coop<T>), dim3(coop_grid), dim3(64), 0, st, wk, lv, bv, io, q, bp, break_distance2, s);
    }, [&] {
      if (!aside || !wk.shape_finish_over) return;
      if (hipEventRecord(aside->fork, st) != hipSuccess || hipStreamWaitEvent(aside->stream, aside->fork, 0) != hipSuccess) return;
      launch_shape_finish<T, MESH_UNIT_PART>(grid_finish, aside->stream, wk, lv, io, q, bp, fin, 0, 1);
      forked = hipEventRecord(aside->join, aside->stream) == hipSuccess;
    });
    (void)cut;
    launch_shape_finish<T, MESH_UNIT_PART>(grid_finish, st, wk, lv, io, q, bp, fin, 0, forked ? 2 : 0);
    if (forked) hipStreamWaitEvent(st, aside->join, 0);
    return;
  }
  // the walk in task levels (or unsplit)
  bvh_collide_levels<T, MESH_UNIT_PART>(grid, st, wk, io, bp, split, int(CTR_SHAPE_TICKET), [&](const BvhSplit& s) {
    launch_collide_solid<T>(grid, st, wk, lv, bv, io, q, bp, break_distance2, s, spill);
  });
  split.level = 0;
  launch_shape_finish<T, MESH_UNIT_PART>(grid_finish, st, wk, lv, io, q, bp, split, 0);
}
#define HFCL_INST(T)                                                                                                             \
  template void launch_bvh_shape<T>(int, hipStream_t, const Work&, const LibView<T>&, const BvhView<T>&, const IO<T>&, const QParams<T>&, const BvhParams&, T);   \
  template void launch_bvh_shape_fast<T>(int, int, int, hipStream_t, const Work&, const LibView<T>&, const BvhView<T>&, const IO<T>&, const QParams<T>&, const BvhParams&, T, BvhSplit, BvhSpill, const AsideStream*);
HFCL_INST(float)
HFCL_INST(double)
#undef HFCL_INST
