// hfcl_k_hfield.hip -- HeightField<AABB> x convex solid collide() on the device (hfcl_hfield_collide_batch*; the arithmetic:
// hfcl_hfield.hpp).  Built without contraction (FLAGS_k_hfield): the records are the bits of the header's host build (tests/hfield_harness).
// The kernels are the listed-leaf pipeline's (hfcl_listed.hpp: k_listed_walk<EMIT>, k_listed_leaf, k_listed_fold<CONTACTS>) for HfKind,
// which plugs in:
//   the walk   the solid's world box, then the walk of the stored tree (stack in LDS, a column per lane); an item is the leaf's node and
//              the running minimum of the box bounds
//   the leaf   the two prisms (vertices in LDS), each through GJK / EPA against the solid, binCorrection, the combination and the gate
//   the fold   hf_fold, hf_fill_contact, hf_skipped_record
// and k_hf_scan, the pipeline's scan for every kind: one workgroup, the exclusive scan of m counts (on top of *running where given).
// Every loop is bounded by what its comment names: a field's node count, HF_STACK, a hull's vertices, gjk_max_iterations /
// epa_max_iterations (hfcl_gjk.hpp / hfcl_epa.hpp), a query's item count.
#include "hfcl_dev.hpp"
#include "hfcl_hfield.hpp"

using namespace hfcl;

struct HfKind {
  using Args = HfArgs;
  using Item = HfItem<double>;
  using Leaf = HfLeafOut<double>;
  static constexpr const char* timer_names[LISTED_TIMED_KERNELS] = {"k_hf_walk<emit>", "k_hf_leaf", "k_hf_fold", "k_hf_scan<contacts>",
                                                                    "k_hf_fold<contacts>"};
  // a query the kernels evaluate: ids inside the tables, a solid with an evaluator, not skipped by the request
  static __device__ __forceinline__ bool valid(const Args& a, uint32_t i) {
    if (a.skip_all) return false;
    const uint32_t f = a.hfield[i], s = a.shape[i];
    if (f >= a.n_fields || s >= a.n_shapes) return false;
    return hf_kind_supported(a.shapes[s].kind);
  }
  template <class Emit>
  static __device__ __forceinline__ double walk(const Args& a, uint32_t i, Emit emit) {
    __shared__ uint32_t stack[HF_STACK][64];
    const DHfield f = a.fields[a.hfield[i]];
    const DShape<double> s = a.shapes[a.shape[i]];
    const Pose<double> tfh = load_pose(a.tf_c, i), tfs = load_pose(a.tf_s, i);
    V3<double> blo, bhi;
    hf_solid_world_box(s, a.verts, tfs, blo, bhi);
    bool overflow;
    return hf_walk(a.nodes + f.node_off, f.n_nodes, tfh, blo, bhi, a.q.security_margin, a.bd2, &stack[0][threadIdx.x], 64,
                   [&](uint32_t node, double box_min) {
                     emit([&](Item& it) {
                       it.node = node;
                       it.box_min = box_min;
                     });
                   },
                   overflow);
  }
  static __device__ __forceinline__ void leaf(const Args& a, const Item& item, const GroupSolid& solid, EpaScratch<double, EPA_MAX_ITER>* scratch,
                                              int grp, Leaf& out) {
    __shared__ HfPrisms<double> prisms[64 / BS_W];
    const uint32_t i = item.query;
    const DHfield f = a.fields[a.hfield[i]];
    HfSweptSupport<double, GroupSolid> ssup;
    ssup.s = solid.s;
    ssup.solid = &solid;
    const Pose<double> tfh = load_pose(a.tf_c, i), tfs = load_pose(a.tf_s, i);
    hf_leaf<double, LaneGroup<BS_W>>(a.nodes[f.node_off + item.node], a.heights + f.height_off, f.nx, a.xgrid + f.xg_off, a.ygrid + f.yg_off,
                                     f.min_height, tfh, tfs, solid, ssup, solid.s.kind == K_CONVEX, swept_radius(solid.s), a.q, scratch,
                                     prisms[grp], out);
  }
  template <class OnContact>
  static __device__ __forceinline__ uint32_t fold(const Args& a, uint64_t begin, uint64_t n_items, uint32_t i, bool swapped, OnContact on_contact,
                                                  hfcl_result* rec, double* dlb_out) {
    return hf_fold(a.items + begin, a.leaves + begin, n_items, a.box_total[i], a.q.security_margin, a.q.collision_distance_threshold,
                   a.num_max_contacts, swapped, on_contact, rec, dlb_out);
  }
  static __device__ __forceinline__ void fill_contact(hfcl_contact& c, uint32_t pair, uint32_t node, const Leaf& lf, bool swapped) {
    hf_fill_contact(c, pair, node, lf, swapped);
  }
  static __device__ __forceinline__ void skipped_record(hfcl_result* rec, double* dlb_out, bool swapped) { hf_skipped_record(rec, dlb_out, swapped); }
};

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

void launch_hf_scan(hipStream_t st, const uint32_t* counts, uint64_t* offsets, uint32_t m, uint64_t* running) {
  hipLaunchKernelGGL(k_hf_scan, dim3(1), dim3(256), 0, st, counts, offsets, m, running);
}

void launch_hf_count(hipStream_t st, const HfArgs& a) { launch_listed_count<HfKind>(st, a); }
void launch_hf_solve(hipStream_t st, const HfArgs& a, int max_blocks, bool want_contacts, const char** names, hipEvent_t* e0, hipEvent_t* e1) {
  launch_listed_solve<HfKind>(st, a, max_blocks, want_contacts, names, e0, e1);
}
