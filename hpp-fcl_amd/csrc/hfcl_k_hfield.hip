// hfcl_k_hfield.hip -- HeightField<AABB> x convex solid collide() on the device (hfcl_hfield_collide_batch*; the arithmetic:
// hfcl_hfield.hpp).  Built without contraction (FLAGS_k_hfield): the records are the bits of the header's host build (tests/hfield_harness).
//   k_hf_walk<EMIT>     a lane per query of a chunk: the solid's world box, then the walk of the stored tree (stack in LDS, a column per
//                       lane).  EMIT = false counts the visited leaves; EMIT = true, after the scan, lists them in walk order with the
//                       running minimum of the box bounds and writes the walk's overall box minimum.  Two walks and a scan: no atomics.
//   k_hf_scan           one workgroup: exclusive scan of m counts (on top of *running where given)
//   k_hf_leaf           a listed (query, leaf) item per BS_W-lane group: the two prisms (vertices in LDS), each through GJK / EPA against
//                       the solid (the group's lanes share a hull's support scan and EPA's face work; the full-capacity polytope in LDS, as
//                       k_triangle), binCorrection, the combination and the gate
//   k_hf_fold<CONTACTS> a lane per query: the replay of its items in order.  CONTACTS = false writes the record, the bound and the
//                       query's contact count; CONTACTS = true, after the scan of the counts, writes the contacts at their offsets.
// Every loop is bounded by what its comment names: a field's node count, HF_STACK, a hull's vertices, gjk_max_iterations /
// epa_max_iterations (hfcl_gjk.hpp / hfcl_epa.hpp), a query's item count.
#include "hfcl_dev.hpp"
#include "hfcl_hfield.hpp"

using namespace hfcl;

// a query the kernels evaluate: ids inside the tables, a solid with an evaluator, not skipped by the request
static __device__ __forceinline__ bool hf_query_valid(const HfArgs& a, uint32_t i) {
  if (a.skip_all) return false;
  const uint32_t f = a.hfield[i], s = a.shape[i];
  if (f >= a.n_fields || s >= a.n_shapes) return false;
  return hf_kind_supported(a.shapes[s].kind);
}

template <bool EMIT>
__global__ void __launch_bounds__(64) k_hf_walk(HfArgs a) {
  __shared__ uint32_t stack[HF_STACK][64];
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= a.m) return;
  uint32_t cnt = 0;
  double total = Lim<double>::max();
  if (hf_query_valid(a, i)) {
    const DHfield f = a.fields[a.hfield[i]];
    const DShape<double> s = a.shapes[a.shape[i]];
    const Pose<double> tfh = load_pose(a.tf_h, i), tfs = load_pose(a.tf_s, i);
    V3<double> blo, bhi;
    hf_solid_world_box(s, a.verts, tfs, blo, bhi);
    uint64_t pos = EMIT ? a.offsets[i] : 0u;
    const uint64_t end = EMIT ? a.offsets[i + 1u] : 0u;
    bool overflow;
    total = hf_walk(a.nodes + f.node_off, f.n_nodes, tfh, blo, bhi, a.q.security_margin, a.bd2, &stack[0][threadIdx.x], 64,
                    [&](uint32_t node, double box_min) {
                      if (EMIT && pos < end && pos < a.n_items) {  // (the second walk visits what the first one counted)
                        HfItem<double> it;
                        it.node = node;
                        it.query = i;
                        it.box_min = box_min;
                        a.items[pos] = it;
                      }
                      ++pos;
                      ++cnt;
                    },
                    overflow);
  }
  if (EMIT) a.box_total[i] = total;
  else a.counts[i] = cnt;
}

// One workgroup.  Thread t owns the counts [t * share, (t + 1) * share): their sum, a scan of the 256 sums, then the offsets.
__global__ void __launch_bounds__(256) k_hf_scan(const uint32_t* __restrict__ counts, uint64_t* __restrict__ offsets, uint32_t m, uint64_t* running) {
  __shared__ uint64_t wave_sum[4];
  const uint32_t share = (m + 255u) / 256u;
  const uint32_t lo = threadIdx.x * share < m ? threadIdx.x * share : m;
  const uint32_t hi = lo + share < m ? lo + share : m;
  const uint64_t before = running ? *running : 0u;
  uint64_t mine = 0;
  for (uint32_t b = lo; b < hi; ++b) mine += counts[b];
  uint64_t incl = mine;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t up = __shfl_up(incl, off, 64);
    if (lane >= uint32_t(off)) incl += up;
  }
  if (lane == 63u) wave_sum[wave] = incl;
  __syncthreads();  // (every thread has read *running by now)
  uint64_t run = before + incl - mine;
  for (uint32_t w = 0; w < wave; ++w) run += wave_sum[w];
  for (uint32_t b = lo; b < hi; ++b) {
    offsets[b] = run;
    run += counts[b];
  }
  if (threadIdx.x == 255u) {
    offsets[m] = run;
    if (running) *running = run;
  }
}

// support of the solid in its own frame, evaluated by the lane group (NoSweptSphere): what k_bvh_shape / k_triangle plug into the solver
struct HfGroupSolid {
  DShape<double> s;
  HullRegs<double, BS_W> h;
  const double* v;
  int lig;
  __device__ __forceinline__ V3<double> operator()(const V3<double>& d) const {
    if (s.kind != K_CONVEX) return prim_support(s, d);
    if (s.num_points > uint32_t(HULL_MAX)) return scan_support<double, BS_W>(v, s.num_points, d, lig);
    return h.support(d, lig);
  }
};

__global__ void __launch_bounds__(64) k_hf_leaf(HfArgs a) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<double, EPA_MAX_ITER> scratch[G];
  __shared__ HfPrisms<double> prisms[G];
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint64_t it = uint64_t(blockIdx.x) * G + grp; it < a.n_items; it += uint64_t(gridDim.x) * G) {
    const HfItem<double> item = a.items[it];
    const uint32_t i = item.query;
    const DHfield f = a.fields[a.hfield[i]];
    HfGroupSolid solid;
    solid.s = a.shapes[a.shape[i]];
    solid.v = a.verts + 3 * size_t(solid.s.vertex_offset);
    solid.lig = lig;
    if (solid.s.kind == K_CONVEX && solid.s.num_points <= uint32_t(HULL_MAX)) solid.h.load(solid.v, solid.s.num_points, lig);
    HfSweptSupport<double, HfGroupSolid> ssup;
    ssup.s = solid.s;
    ssup.solid = &solid;
    const Pose<double> tfh = load_pose(a.tf_h, i), tfs = load_pose(a.tf_s, i);
    HfLeafOut<double> out;
    hf_leaf<double, LaneGroup<BS_W>>(a.nodes[f.node_off + item.node], a.heights + f.height_off, f.nx, a.xgrid + f.xg_off, a.ygrid + f.yg_off,
                                     f.min_height, tfh, tfs, solid, ssup, solid.s.kind == K_CONVEX, swept_radius(solid.s), a.q, &scratch[grp],
                                     prisms[grp], out);
    if (lig == 0) a.leaves[it] = out;
    LaneGroup<BS_W>::sync();
  }
}

template <bool CONTACTS>
__global__ void __launch_bounds__(256) k_hf_fold(HfArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.m) return;
  const bool swapped = a.swapped && a.swapped[i];
  if (!hf_query_valid(a, i)) {
    if (!CONTACTS) {
      hf_skipped_record(&a.out[i], a.dlb ? &a.dlb[i] : nullptr, swapped);
      if (a.ccounts) a.ccounts[i] = 0u;
    }
    return;
  }
  const uint64_t begin = a.offsets[i], end = a.offsets[i + 1u];
  const uint64_t n_items = end > begin && end <= a.n_items ? end - begin : 0u;
  if (CONTACTS) {
    const uint64_t at = a.coffsets[i];
    hf_fold(a.items + begin, a.leaves + begin, n_items, a.box_total[i], a.q.security_margin, a.q.collision_distance_threshold, a.num_max_contacts,
            swapped,
            [&](uint32_t k, uint32_t node, const HfLeafOut<double>& lf) {
              if (at + k < a.contacts_cap) hf_fill_contact(a.contacts[at + k], a.pair0 + i, node, lf, swapped);
            },
            static_cast<hfcl_result*>(nullptr), static_cast<double*>(nullptr));
  } else {
    const uint32_t nc = hf_fold(a.items + begin, a.leaves + begin, n_items, a.box_total[i], a.q.security_margin, a.q.collision_distance_threshold,
                                a.num_max_contacts, swapped, [](uint32_t, uint32_t, const HfLeafOut<double>&) {}, &a.out[i],
                                a.dlb ? &a.dlb[i] : nullptr);
    if (a.ccounts) a.ccounts[i] = nc;
  }
}

void launch_hf_count(hipStream_t st, const HfArgs& a) {
  if (!a.m) return;
  hipLaunchKernelGGL(k_hf_walk<false>, dim3((a.m + 63u) / 64u), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_hf_scan, dim3(1), dim3(256), 0, st, a.counts, a.offsets, a.m, static_cast<uint64_t*>(nullptr));
}

// the scan on its own, for the units that list items the same way (hfcl_k_octree.hip)
void launch_hf_scan(hipStream_t st, const uint32_t* counts, uint64_t* offsets, uint32_t m, uint64_t* running) {
  hipLaunchKernelGGL(k_hf_scan, dim3(1), dim3(256), 0, st, counts, offsets, m, running);
}

void launch_hf_solve(hipStream_t st, const HfArgs& a, int max_blocks, bool want_contacts, const char** names, hipEvent_t* e0, hipEvent_t* e1) {
  static const char* const kn[HF_TIMED_KERNELS] = {"k_hf_walk<emit>", "k_hf_leaf", "k_hf_fold", "k_hf_scan<contacts>", "k_hf_fold<contacts>"};
  for (int k = 0; k < HF_TIMED_KERNELS; ++k) names[k] = kn[k];
  if (!a.m) return;
  auto begin = [&](int k) { if (e0) (void)hipEventRecord(e0[k], st); };
  auto end = [&](int k) { if (e1) (void)hipEventRecord(e1[k], st); };
  begin(0);
  hipLaunchKernelGGL(k_hf_walk<true>, dim3((a.m + 63u) / 64u), dim3(64), 0, st, a);
  end(0);
  begin(1);
  if (a.n_items) {
    constexpr uint64_t G = 64 / BS_W;
    const uint32_t grid = uint32_t(std::min<uint64_t>((a.n_items + G - 1u) / G, uint64_t(std::max(max_blocks, 1))));
    hipLaunchKernelGGL(k_hf_leaf, dim3(grid), dim3(64), 0, st, a);
  }
  end(1);
  begin(2);
  hipLaunchKernelGGL(k_hf_fold<false>, dim3((a.m + 255u) / 256u), dim3(256), 0, st, a);
  end(2);
  begin(3);
  if (want_contacts) hipLaunchKernelGGL(k_hf_scan, dim3(1), dim3(256), 0, st, a.ccounts, a.coffsets, a.m, a.running);
  end(3);
  begin(4);
  if (want_contacts && a.contacts) hipLaunchKernelGGL(k_hf_fold<true>, dim3((a.m + 255u) / 256u), dim3(256), 0, st, a);
  end(4);
}
