// hfcl_mesh.hpp -- what the three mesh objects share as templates: hfcl_k_bvh.hip (hfcl_k_bvh.o, mesh x mesh collide() and triangle
// pairs), hfcl_k_bvhc.hip (hfcl_k_bvhc.o, mesh x solid collide()) and hfcl_k_bvhs.hip (hfcl_k_bvhs.o, mesh x solid distance()).  Only
// these include it, the two collide() sources through hfcl_mesh_collide.hpp, which holds what those two alone share.  Here: the task
// summaries' accessors, the solid of a lane and of a lane group, the mesh x solid leaf as a call, and the leaves that needed EPA
// (k_bvh_shape_finish), which both solid objects launch.
//
// The three objects are built under two contraction settings, so no kernel and no non-inlined device function may be instantiated with
// the same arguments in two of them: hfcl_mesh_collide.hpp's opening comment says why and how that is kept.  What it means here:
// k_bvh_shape_finish carries the launching object's part (its source's MESH_UNIT_PART) as a template argument.
#pragma once
#include <algorithm>

#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"

// the summary of a suspended query or of a task (hfcl_dev.hpp: BvhSum)
template <typename T>
__device__ __forceinline__ BvhSum<T>* bvh_sum(const BvhSplit& sp, uint32_t slot) { return reinterpret_cast<BvhSum<T>*>(sp.sums) + slot; }

// ---------------------------------------------------------------------------------------
// Mesh x solid with one query per LANE: pieces of the SOLID form of k_bvh_collide (hfcl_mesh_collide.hpp) and of k_bvh_shape_finish (below).
// ---------------------------------------------------------------------------------------
#ifndef HFCL_LANE_SOLID_BATCH
#define HFCL_LANE_SOLID_BATCH 4
#endif
template <typename T>
struct LaneSolid {  // support of the solid in its own frame, by one lane (ConvexBase: serial scan, first maximum wins)
  DShape<T> s;
  const T* v;
  __device__ __forceinline__ V3<T> operator()(const V3<T>& d) const {
    if (s.kind != K_CONVEX) return prim_support(s, d);
    uint32_t best = 0;
    T bd = v[0] * d.x + v[1] * d.y + v[2] * d.z;
    uint32_t i = 1;
#if HFCL_LANE_SOLID_BATCH
    // HFCL_LANE_SOLID_BATCH vertices (four: 96 consecutive bytes in fp64) fetched together, then their products in the scan's order: one vertex per trip of a loop
    // of unknown length was one exposed load latency per vertex, 32 per support call of a convex solid
    constexpr uint32_t LB = HFCL_LANE_SOLID_BATCH;
    for (; i + LB <= s.num_points; i += LB) {
      T a[3 * LB];
#pragma unroll
      for (int j = 0; j < int(3 * LB); ++j) a[j] = v[3 * size_t(i) + size_t(j)];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < int(LB); ++j) {
        const T x = a[3 * j] * d.x + a[3 * j + 1] * d.y + a[3 * j + 2] * d.z;
        if (x > bd) {
          bd = x;
          best = i + uint32_t(j);
        }
      }
    }
#endif
    for (; i < s.num_points; ++i) {
      const T x = v[3 * size_t(i)] * d.x + v[3 * size_t(i) + 1] * d.y + v[3 * size_t(i) + 2] * d.z;
      if (x > bd) {
        bd = x;
        best = i;
      }
    }
    return mk<T>(v[3 * size_t(best)], v[3 * size_t(best) + 1], v[3 * size_t(best) + 2]);
  }
};
template <typename T>
__device__ __forceinline__ void emit_shape_contact(const BvhParams& bp, uint32_t pair, bool swapped, int prim, T distance,
                                                   const V3<T>& p1, const V3<T>& p2, const V3<T>& nn) {
  if (!bp.contacts) return;
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
}
template <typename T>
__device__ __forceinline__ void store_unsupported(const IO<T>& io, uint32_t pair) {
  auto r = io.out[pair];
  memset(&r, 0, sizeof(r));
  r.status = 0x80000000u;
  io.out[pair] = r;
}
// Is the work of the task (parent slot p, position o) still needed?  Not if an earlier sibling -- of it or of any of its
// ancestors -- has found a contact: the sequential walk would have ended there.
template <typename T>
__device__ __forceinline__ bool bvh_moot(const BvhSplit& split, uint32_t p, uint32_t o) {
  for (int hop = 0; hop < BVH_MAX_LEVELS + 1 && p != 0xFFFFFFFFu; ++hop) {
    const BvhSum<T>* ps = bvh_sum<T>(split, p);
    if (__hip_atomic_load(&ps->contact_order, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < o) return true;
    o = ps->order;
    p = ps->parent;
  }
  return false;
}
template <typename T>
struct SolidLeafOut {
  T distance;
  V3<T> p1, p2, n, guess;
};
template <typename T>
struct SolidLeafIn {
  const T* mesh_verts;      // of this model
  const uint32_t* tri;      // the triangle's three vertex ids
  const DShape<T>* shapes;
  const T* lib_verts;
  const decltype(IO<T>::tf1) pose_m;  // pose arrays of the mesh / the solid
  const decltype(IO<T>::tf1) pose_s;
  ShapeDeferItem<T>* defer;
  uint32_t* defer_count;
  uint32_t defer_cap;
  uint32_t pair, solid_id, prim, parent, order;
  T bound;            // distance(): min_distance before this leaf, and the triangle it belongs to
  int32_t prev_prim;
};
template <typename T, class PS>
__device__ __noinline__ bool solid_leaf_call(const SolidLeafIn<T> in, const QParams<T>* qp, const PS ps, const V3<T> guess_in, SolidLeafOut<T>* out,
                                             uint32_t* slot_out = nullptr) {
  const QParams<T> q = *qp;
  auto vtx = [&](uint32_t i) { return mk<T>(in.mesh_verts[3 * size_t(i)], in.mesh_verts[3 * size_t(i) + 1], in.mesh_verts[3 * size_t(i) + 2]); };
  const V3<T> ta = vtx(in.tri[0]), tb = vtx(in.tri[1]), tc = vtx(in.tri[2]);
  LaneSolid<T> solid;
  solid.s = in.shapes[in.solid_id];
  solid.v = in.lib_verts + 3 * size_t(solid.s.vertex_offset);
  auto tfm_of = [&]() { return load_pose(in.pose_m, in.pair); };
  auto tfs_of = [&]() { return load_pose(in.pose_s, in.pair); };
  const MDiff<T> sMt = make_mdiff(tfs_of(), tfm_of());
  V3<T> guess = guess_in;
  ShapeDeferItem<T> item;
  const bool to_epa = mesh_shape_leaf_lane(ta, tb, tc, sMt, tfm_of, tfs_of, solid.s, solid, swept_radius(solid.s), q, guess, ps, out->distance,
                                           out->p1, out->p2, out->n, item);
  if (to_epa && in.defer) {  // (defer == nullptr: the caller only asks whether the leaf needs EPA)
    item.seed.pair = in.pair;
    item.prim = in.prim;
    item.parent = in.parent;
    item.order = in.order;
    item.bound = in.bound;
    item.prev_prim = in.prev_prim;
    const uint32_t slot = atomicAdd(in.defer_count, 1u);
    if (slot < in.defer_cap) in.defer[slot] = item;  // (the host sizes the queue for one item per unit of the batch; never past its end)
    if (slot_out) *slot_out = slot;
  }
  out->guess = guess;
  return to_epa;
}

// One query per BS_W-lane group (k_bvh_shape, k_bvh_shape_distance, k_bvh_shape_finish, k_triangle): the solid of such a group.
template <typename T>
struct GroupSolid {  // support of the solid in its own frame, evaluated by the lane group
  DShape<T> s;
  HullRegs<T, BS_W> h;
  const T* v;
  int lig;
  __device__ __forceinline__ V3<T> operator()(const V3<T>& d) const {
    if (s.kind != K_CONVEX) return prim_support(s, d);
    if (s.num_points > uint32_t(HULL_MAX)) return scan_support<T, BS_W>(v, s.num_points, d, lig);
    return h.support(d, lig);
  }
};

// k_bvh_shape_finish: the leaves that needed EPA, one per BS_W-lane group with the full-capacity polytope in LDS, after the walk and
// its fold-back: a leaf whose unit was not overtaken by an earlier contact (bvh_moot) is the query's contact; its depth is compared
// with the bound the record holds (updateDistanceLowerBoundFromLeaf) and patched in.
// Two tiers (HFCL_SHAPE_FINISH_TIERS, default on), as k_epa's: CAP = SHAPE_FINISH_FAST_CAP first -- a block a third the size, two waves
// per SIMD where the full-capacity block admits one -- and the polytopes that outgrow it listed in Work::shape_finish_over for a second
// launch at EPA_MAX_ITER that starts them again (tier: 0 the only launch, 1 the fast one, 2 the one over the list).  What a polytope that
// fits computes does not depend on the block's capacity (tests/test_gpu_parity.py: test_epa_hand_over_equals_restart is the same property of
// k_epa's tiers), so the records are those of the one-tier form.
#ifndef HFCL_SHAPE_FINISH_FAST_CAP
#define HFCL_SHAPE_FINISH_FAST_CAP 21
#endif
constexpr int SHAPE_FINISH_FAST_CAP = HFCL_SHAPE_FINISH_FAST_CAP;
template <typename T, int PART, int CAP = EPA_MAX_ITER>  // PART: the launching object's identity only (head of this file); the body does not read it
// range: 0 every item; 1 the items in front of CTR_SHAPE_DEFER_MARK (whole walks: final once the first launch of k_bvh_shape_coop is over); 2 the
// items behind it (those of chunks).  Ranges 1 and 2 run on two streams and list their second tier in the two halves of shape_finish_over.
__global__ void __launch_bounds__(64) k_bvh_shape_finish(Work wk, LibView<T> lib, IO<T> io, QParams<T> q, BvhParams bp, BvhSplit split, int distance_mode, int tier, int range) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<T, CAP> scratch[G];
  const int half = range == 2 ? 1 : 0;
  uint32_t* const over = wk.shape_finish_over + size_t(half) * wk.shape_defer_cap;
  const uint32_t first = tier != 2 && range == 2 ? wk.counts[CTR_SHAPE_DEFER_MARK] : 0u;
  const uint32_t cnt = tier == 2 ? min(wk.counts[CTR_SHAPE_FINISH_OVER + half], wk.shape_defer_cap)
                                 : (range == 1 ? wk.counts[CTR_SHAPE_DEFER_MARK] : min(wk.counts[CTR_SHAPE_DEFER], wk.shape_defer_cap));
  const ShapeDeferItem<T>* const items = reinterpret_cast<const ShapeDeferItem<T>*>(wk.shape_defer);
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint32_t k = first + blockIdx.x * G + grp; k < cnt; k += gridDim.x * G) {
    const uint32_t it = tier == 2 ? over[k] : k;
    const ShapeDeferItem<T> item = items[it];
    if (split.tasks && bvh_moot<T>(split, item.parent, item.order)) continue;  // (group-uniform) an earlier contact ended the walk
    const uint32_t pair = item.seed.pair;
    const DShape<T> a = lib.shapes[wk.shape1[pair]], b = lib.shapes[wk.shape2[pair]];
    const bool swapped = a.kind != K_BVH;
    GroupSolid<T> solid;
    solid.s = swapped ? a : b;
    solid.v = lib.verts + 3 * size_t(solid.s.vertex_offset);
    solid.lig = lig;
    if (solid.s.kind == K_CONVEX && solid.s.num_points <= uint32_t(HULL_MAX)) solid.h.load(solid.v, solid.s.num_points, lig);
    const Pose<T> tfs = load_pose(swapped ? io.tf1 : io.tf2, pair);
    V3<T> p1, p2, n, guess;
    bool done = true;
    const T distance = mesh_shape_leaf_finish<T, LaneGroup<BS_W>, GroupSolid<T>, CAP>(item, tfs, solid, swept_radius(solid.s), q, &scratch[grp], p1, p2, n, guess, &done);
    if (CAP != EPA_MAX_ITER && !done) {  // (group-uniform) to the full-capacity launch
      if (lig == 0) over[atomicAdd(&wk.counts[CTR_SHAPE_FINISH_OVER + half], 1u)] = it;
      LaneGroup<BS_W>::sync();
      continue;
    }
    if (lig == 0 && distance_mode) {
      // distance(): the walk ended at this leaf (every bound left on the stack is >= 0); DistanceResult::update
      T mind = item.bound;
      int prim = item.prev_prim;
      if (mind > distance) {
        mind = distance;
        prim = int(item.prim);
        store_witness(io, pair, swapped ? p2 : p1, swapped ? p1 : p2, swapped ? -n : n);
      }
      store_bvh_record_head(io, pair, mind, mind <= T(0) ? 0x80000000u : 0u, prim, -1, false);
      write_guess<T>(io, pair, guess, 0, 0);
    } else if (lig == 0) {
      // the record holds the walk's result without this leaf: recorded distance = bound + margin where a leaf set it (the
      // same subtraction as updateDistanceLowerBoundFromLeaf's), a positive OBB bound otherwise (always above a penetration)
      auto* r = &io.out[pair];
      const T dtc = distance - q.security_margin;
      if (dtc < T(r->distance) - q.security_margin) {
        r->distance = distance;
        store_witness(io, pair, swapped ? p2 : p1, swapped ? p1 : p2, swapped ? -n : n);
      }
      emit_shape_contact(bp, pair, swapped, int(item.prim), distance, p1, p2, n);
      write_guess<T>(io, pair, guess, 0, 0);
    }
    LaneGroup<BS_W>::sync();
  }
}

template <typename T, int PART>
static void launch_shape_finish(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q, const BvhParams& bp, const BvhSplit& split,
                                int distance_mode, int range = 0) {
  if (wk.shape_finish_over && q.epa_max_iterations > SHAPE_FINISH_FAST_CAP) {
    hipLaunchKernelGGL((k_bvh_shape_finish<T, PART, SHAPE_FINISH_FAST_CAP>), dim3(grid), dim3(64), 0, st, wk, lv, io, q, bp, split, distance_mode, 1, range);
    hipLaunchKernelGGL((k_bvh_shape_finish<T, PART, EPA_MAX_ITER>), dim3(std::max(1, grid / 4)), dim3(64), 0, st, wk, lv, io, q, bp, split, distance_mode, 2, range);
  } else {
    hipLaunchKernelGGL((k_bvh_shape_finish<T, PART, EPA_MAX_ITER>), dim3(grid), dim3(64), 0, st, wk, lv, io, q, bp, split, distance_mode, 0, range);
  }
}
