// hfcl_listed.hpp -- the listed-leaf pipeline that the containers of convex solids share: height fields (hfcl_hfield.hpp,
// hfcl_k_hfield.hip) and octrees (hfcl_octree.hpp, hfcl_k_octree.hip).  A lane per query counts the leaves its walk reaches, a scan
// turns the counts into offsets, a second walk lists the leaves; a BS_W-lane group solves each listed item; a lane per query folds its
// items in order into the record, the bound and the contacts.  Here: the part of the kernels' parameter block every kind has
// (ListedArgs; builds with g++ too) and, for hipcc, the kernels and their launches once, as templates over a kind.  The arithmetic --
// walk, leaf, fold -- stays in the kind's header; a kind is a struct of types, names and static __forceinline__ functions defined in its
// kernel unit (HfKind, OctKind), so nothing of it is left to run time.
#pragma once
#include "../../include/hppfcl_amd.h"
#include "hfcl_pair.hpp"

namespace hfcl {

// A chunk of m queries of a call: the per-query arrays point at the chunk's first query.  A kind's block (HfArgs, OctArgs) adds its
// tables, the array of its container ids and its typed items / leaves.
struct ListedArgs {
  const DShape<double>* shapes;
  const double* verts;
  uint32_t n_shapes;
  const uint32_t* shape;
  const double* tf_c;      // the containers' poses (the height fields', the octrees')
  const double* tf_s;
  const uint8_t* swapped;  // nullptr: none
  uint32_t m, pair0;       // queries of the chunk; index of its first query in the call (hfcl_contact::pair)
  QParams<double> q;       // of the request (height fields: hf_leaf_params of it)
  double bd2;              // break_distance^2
  uint32_t num_max_contacts;
  int skip_all;            // security_margin == -inf
  uint32_t* counts;        // m: listed leaves of a query
  uint64_t* offsets;       // m + 1: where a query's items start
  double* box_total;       // m: the minimum over all box bounds of a query's walk
  uint64_t n_items;
  uint32_t* ccounts;       // m: contacts of a query
  uint64_t* coffsets;      // m + 1: where they go in the call's contact list
  uint64_t* running;       // contacts of the chunks before this one, then of this one too
  hfcl_result* out;
  double* dlb;             // nullptr or m
  hfcl_contact* contacts;  // nullptr or contacts_cap records
  uint64_t contacts_cap;
};

}  // namespace hfcl

#if defined(__HIPCC__)
#include "hfcl_dev.hpp"

constexpr int LISTED_TIMED_KERNELS = 5;  // the entries of a kind's timer_names: walk<emit>, leaf, fold, scan<contacts>, fold<contacts>
// hfcl_k_hfield.hip: one workgroup -- the exclusive scan of m counts (on top of *running where given), offsets[m] = the total
__global__ void k_hf_scan(const uint32_t* __restrict__ counts, uint64_t* __restrict__ offsets, uint32_t m, uint64_t* running);
void launch_hf_scan(hipStream_t st, const uint32_t* counts, uint64_t* offsets, uint32_t m, uint64_t* running);

namespace hfcl {

// support of the solid in its own frame, evaluated by the lane group (NoSweptSphere): what k_bvh_shape / k_triangle plug into the solver
struct GroupSolid {
  DShape<double> s;
  HullRegs<double, BS_W> h;
  const double* v;
  int lig;
  // the solid of query i of the chunk, its hull in the group's registers where it fits
  template <class Args>
  __device__ __forceinline__ void load(const Args& a, uint32_t i, int lane_in_group) {
    s = a.shapes[a.shape[i]];
    v = a.verts + 3 * size_t(s.vertex_offset);
    lig = lane_in_group;
    if (s.kind == K_CONVEX && s.num_points <= uint32_t(HULL_MAX)) h.load(v, s.num_points, lig);
  }
  __device__ __forceinline__ V3<double> operator()(const V3<double>& d) const {
    if (s.kind != K_CONVEX) return prim_support(s, d);
    if (s.num_points > uint32_t(HULL_MAX)) return scan_support<double, BS_W>(v, s.num_points, d, lig);
    return h.support(d, lig);
  }
};

// A lane per query of a chunk: the kind's walk (its stack in LDS, a column per lane).  EMIT = false counts the reached leaves;
// EMIT = true, after the scan, lists them in walk order -- the kind fills an item's own fields -- and writes the walk's overall box
// minimum.  Two walks and a scan: no atomics.
template <class Kind, bool EMIT>
__global__ void __launch_bounds__(64) k_listed_walk(typename Kind::Args a) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= a.m) return;
  uint32_t cnt = 0;
  double total = Lim<double>::max();
  if (Kind::valid(a, i)) {
    uint64_t pos = EMIT ? a.offsets[i] : 0u;
    const uint64_t end = EMIT ? a.offsets[i + 1u] : 0u;
    total = Kind::walk(a, i, [&](auto fill) {
      if (EMIT && pos < end && pos < a.n_items) {  // (the second walk visits what the first one counted)
        typename Kind::Item it;
        it.query = i;
        fill(it);
        a.items[pos] = it;
      }
      ++pos;
      ++cnt;
    });
  }
  if (EMIT) a.box_total[i] = total;
  else a.counts[i] = cnt;
}

// A listed (query, leaf) item per BS_W-lane group: the kind's leaf against the solid (the group's lanes share a hull's support scan and
// EPA's face work; the full-capacity polytope in LDS, as k_triangle)
template <class Kind>
__global__ void __launch_bounds__(64) k_listed_leaf(typename Kind::Args a) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<double, EPA_MAX_ITER> scratch[G];
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint64_t it = uint64_t(blockIdx.x) * G + grp; it < a.n_items; it += uint64_t(gridDim.x) * G) {
    const typename Kind::Item item = a.items[it];
    GroupSolid solid;
    solid.load(a, item.query, lig);
    typename Kind::Leaf out;
    Kind::leaf(a, item, solid, &scratch[grp], grp, out);
    if (lig == 0) a.leaves[it] = out;
    LaneGroup<BS_W>::sync();
  }
}

// A lane per query: the replay of its items in order.  CONTACTS = false writes the record, the bound and the query's contact count;
// CONTACTS = true, after the scan of the counts, writes the contacts at their offsets.
template <class Kind, bool CONTACTS>
__global__ void __launch_bounds__(256) k_listed_fold(typename Kind::Args a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.m) return;
  const bool swapped = a.swapped && a.swapped[i];
  if (!Kind::valid(a, i)) {
    if (!CONTACTS) {
      Kind::skipped_record(&a.out[i], a.dlb ? &a.dlb[i] : nullptr, swapped);
      if (a.ccounts) a.ccounts[i] = 0u;
    }
    return;
  }
  const uint64_t begin = a.offsets[i], end = a.offsets[i + 1u];
  const uint64_t n_items = end > begin && end <= a.n_items ? end - begin : 0u;
  if (CONTACTS) {
    const uint64_t at = a.coffsets[i];
    Kind::fold(a, begin, n_items, i, swapped,
               [&](uint32_t k, uint32_t node, const typename Kind::Leaf& lf) {
                 if (at + k < a.contacts_cap) Kind::fill_contact(a.contacts[at + k], a.pair0 + i, node, lf, swapped);
               },
               static_cast<hfcl_result*>(nullptr), static_cast<double*>(nullptr));
  } else {
    const uint32_t nc = Kind::fold(a, begin, n_items, i, swapped, [](uint32_t, uint32_t, const typename Kind::Leaf&) {}, &a.out[i],
                                   a.dlb ? &a.dlb[i] : nullptr);
    if (a.ccounts) a.ccounts[i] = nc;
  }
}

// Launches of one chunk, in stream order; no atomics, no kernel waits for another workgroup.
// the counting walk and the scan: a.counts, a.offsets (a.offsets[m] = the items)
template <class Kind>
void launch_listed_count(hipStream_t st, const typename Kind::Args& a) {
  if (!a.m) return;
  hipLaunchKernelGGL((k_listed_walk<Kind, false>), dim3((a.m + 63u) / 64u), dim3(64), 0, st, a);
  launch_hf_scan(st, a.counts, a.offsets, a.m, nullptr);
}

// ... the listing walk, the leaves, the fold and the contacts.  names / e0 / e1: timing slots (e0 == nullptr: none)
template <class Kind>
void launch_listed_solve(hipStream_t st, const typename Kind::Args& a, int max_blocks, bool want_contacts, const char** names, hipEvent_t* e0,
                         hipEvent_t* e1) {
  for (int k = 0; k < LISTED_TIMED_KERNELS; ++k) names[k] = Kind::timer_names[k];
  if (!a.m) return;
  auto begin = [&](int k) { if (e0) (void)hipEventRecord(e0[k], st); };
  auto end = [&](int k) { if (e1) (void)hipEventRecord(e1[k], st); };
  begin(0);
  hipLaunchKernelGGL((k_listed_walk<Kind, true>), dim3((a.m + 63u) / 64u), dim3(64), 0, st, a);
  end(0);
  begin(1);
  if (a.n_items) {
    constexpr uint64_t G = 64 / BS_W;
    const uint32_t grid = uint32_t(std::min<uint64_t>((a.n_items + G - 1u) / G, uint64_t(std::max(max_blocks, 1))));
    hipLaunchKernelGGL((k_listed_leaf<Kind>), dim3(grid), dim3(64), 0, st, a);
  }
  end(1);
  begin(2);
  hipLaunchKernelGGL((k_listed_fold<Kind, false>), dim3((a.m + 255u) / 256u), dim3(256), 0, st, a);
  end(2);
  begin(3);
  if (want_contacts) launch_hf_scan(st, a.ccounts, a.coffsets, a.m, a.running);
  end(3);
  begin(4);
  if (want_contacts && a.contacts) hipLaunchKernelGGL((k_listed_fold<Kind, true>), dim3((a.m + 255u) / 256u), dim3(256), 0, st, a);
  end(4);
}

}  // namespace hfcl
#endif
