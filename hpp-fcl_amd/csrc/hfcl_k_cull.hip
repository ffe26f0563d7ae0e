// hfcl_k_cull.hip -- culling a scene's pair list per configuration on the device (hfcl_scene_cull*), and the scene calls on the list of
// surviving queries (hfcl_scene_*_listed*).  Bandwidth and latency kernels: no geometry loop, no scratch, LDS only for a workgroup's sums.
// Built without contraction (FLAGS_k_cull): the boxes are the bits hfcl_world_aabbs computes on the host (hfcl_cull.hpp).
//   k_cull_aabbs<F32>     a lane per (configuration, object): the pose row (96 B / 28 B) and the 48 B local box of the object's shape in,
//                         the 48 B world box out
//   k_cull_mark           a lane per query of a chunk of the flat range: 8 B of pair list, two boxes of a table that sits in L2; a wave
//                         writes its ballot as one 64-bit word, a workgroup its count
//   k_cull_scan           one workgroup: exclusive scan of the chunk's workgroup counts on top of the survivors of the chunks before
//   k_cull_emit           the geometry of k_cull_mark again: a survivor's rank = its workgroup's offset + the waves before it + the
//                         lanes below it; writes q at its rank (below the capacity) and conf_begin of every configuration whose first
//                         query is in the chunk
//                         Three launches in stream order; no atomics, no kernel waits for another workgroup, the list is ascending
//                         and the same bytes however the range is cut.
//   k_scene_expand_listed64<ALIGNED> / 32   k_scene_expand64 / 32 (hfcl_k_scene.hip) with q read from the list: same lanes, same vectors
//   k_scene_expand_pairs64<ALIGNED> / 32    the same with (i, j) read from a list of explicit pairs (hfcl_scene_*_pairs_device*); the
//                         configuration of an entry is the span of conf_begin that holds it: found once per wave for its first row, a few
//                         steps forward per lane, the search again for a lane whose entry lies further on (hfcl_pairs.hpp)
//   k_scene_summary_init  every configuration's summary to the value of a configuration without records
//   k_scene_fold_listed<R, RANKED>  a wave per (configuration the chunk touches, piece of SCENE_FOLD_SHARE of its records), lanes stride the
//                         piece, butterfly, then lane 0 merges into the stored summary (lists of at most one piece per configuration)
//                         or writes a partial for.  RANKED (lists of explicit pairs): a record's pair index is its rank in its configuration
//   k_scene_fold_listed_combine   a wave per configuration folds its pieces' partials and merges into the stored summary.
//                         The merge is commutative and associative on disjoint sets of pairs: the summaries do not depend on the chunks.
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_cull.hpp"
#include "hfcl_pairs.hpp"

template <bool F32>
__global__ void __launch_bounds__(256) k_cull_aabbs(const void* __restrict__ object_tf, const uint32_t* __restrict__ object_shape,
                                                    const double* __restrict__ local_boxes, uint64_t n_objects, uint64_t n_rows,
                                                    double* __restrict__ boxes) {
  for (uint64_t r = uint64_t(blockIdx.x) * 256u + threadIdx.x; r < n_rows; r += uint64_t(gridDim.x) * 256u) {
    const uint32_t o = uint32_t(r % n_objects);
    const double* lb = local_boxes + 6u * size_t(object_shape[o]);
    double L[6], w[6];
    for (int k = 0; k < 6; ++k) L[k] = lb[k];
    if (F32) {
      const float* p = static_cast<const float*>(object_tf) + 7u * r;
      float q[7];
      for (int k = 0; k < 7; ++k) q[k] = p[k];
      cull_world_box_quat(q, L, w);
    } else {
      const double* p = static_cast<const double*>(object_tf) + 12u * r;
      double t[12];
      for (int k = 0; k < 12; ++k) t[k] = p[k];
      cull_world_box(t, t + 9, L, w);
    }
    double* o6 = boxes + 6u * r;
    for (int k = 0; k < 6; ++k) o6[k] = w[k];
  }
}

void launch_cull_aabbs(hipStream_t st, const void* object_tf, bool f32, const uint32_t* object_shape, const double* local_boxes,
                       uint64_t n_objects, uint64_t n_rows, double* boxes) {
  if (!n_rows) return;
  const uint32_t grid = uint32_t(std::min<uint64_t>((n_rows + 255u) / 256u, 65536u));
  if (f32)
    hipLaunchKernelGGL(k_cull_aabbs<true>, dim3(grid), dim3(256), 0, st, object_tf, object_shape, local_boxes, n_objects, n_rows, boxes);
  else
    hipLaunchKernelGGL(k_cull_aabbs<false>, dim3(grid), dim3(256), 0, st, object_tf, object_shape, local_boxes, n_objects, n_rows, boxes);
}

// ---- mark, scan, emit -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CULL_BLOCK) k_cull_mark(CullArgs a) {
  __shared__ uint32_t wave_count[CULL_WAVES];
  const uint32_t row = blockIdx.x * CULL_BLOCK + threadIdx.x, wave = threadIdx.x >> 6;
  bool keep = false;
  if (row < a.m) {
    uint64_t c;
    uint32_t p;
    scene_query_from(a.c0, a.p0, row, a.n_pairs, c, p);
    const uint2 ij = reinterpret_cast<const uint2*>(a.pairs)[p];
    const double* base = a.boxes + 6u * ((c - a.c_box0) * a.n_objects);
    const double* b1 = base + 6u * size_t(ij.x);
    const double* b2 = base + 6u * size_t(ij.y);
    double x[6], y[6];
    for (int k = 0; k < 6; ++k) {
      x[k] = b1[k];
      y[k] = b2[k];
    }
    keep = cull_keep(x, y, a.inflate);
  }
  const uint64_t ballot = __ballot(keep);
  if ((threadIdx.x & 63u) == 0u) {
    if (row < a.m) a.words[row >> 6] = ballot;
    wave_count[wave] = cull_popcount(ballot);
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t n = 0;
    for (uint32_t w = 0; w < CULL_WAVES; ++w) n += wave_count[w];
    a.block_counts[blockIdx.x] = n;
  }
}

// One workgroup.  Thread t owns the counts [t * share, (t + 1) * share): their sum, a scan of the 256 sums, then the offsets.
__global__ void __launch_bounds__(256) k_cull_scan(CullArgs a, uint32_t n_blocks) {
  __shared__ uint64_t wave_sum[4];
  const uint32_t share = (n_blocks + 255u) / 256u;
  const uint32_t lo = threadIdx.x * share < n_blocks ? threadIdx.x * share : n_blocks;
  const uint32_t hi = lo + share < n_blocks ? lo + share : n_blocks;
  const uint64_t before = a.first ? 0u : *a.running;
  uint64_t mine = 0;
  for (uint32_t b = lo; b < hi; ++b) mine += a.block_counts[b];
  uint64_t incl = mine;  // inclusive scan over the wave, then over the four waves
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
    a.block_offsets[b] = run;
    run += a.block_counts[b];
  }
  if (threadIdx.x == 255u) *a.running = run;
}

__global__ void __launch_bounds__(CULL_BLOCK) k_cull_emit(CullArgs a) {
  const uint32_t row = blockIdx.x * CULL_BLOCK + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (row >= a.m) return;  // (the words of a wave that starts past the chunk were never written)
  const uint64_t* words = a.words + size_t(blockIdx.x) * CULL_WAVES;
  uint64_t pos = a.block_offsets[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) pos += cull_popcount(words[w]);
  const uint64_t ballot = words[wave];
  pos += cull_rank(ballot, lane);
  const bool keep = (ballot >> lane) & 1u;
  const uint64_t q = a.q0 + row;
  if (keep && pos < a.capacity) a.ids[pos] = q;
  if (a.conf_begin) {
    uint64_t c;
    uint32_t p;
    scene_query_from(a.c0, a.p0, row, a.n_pairs, c, p);
    if (p == 0u) a.conf_begin[c] = pos;
  }
  if (q == a.total - 1u) {
    if (a.conf_begin) a.conf_begin[a.n_conf] = pos + (keep ? 1u : 0u);
    if (a.n_listed) *a.n_listed = pos + (keep ? 1u : 0u);
  }
}

void launch_cull_chunk(hipStream_t st, const CullArgs& a) {
  const uint32_t n_blocks = uint32_t((uint64_t(a.m) + CULL_BLOCK - 1u) / CULL_BLOCK);
  hipLaunchKernelGGL(k_cull_mark, dim3(n_blocks), dim3(CULL_BLOCK), 0, st, a);
  launch_cull_scan_emit(st, a);
}

void launch_cull_scan_emit(hipStream_t st, const CullArgs& a) {
  const uint32_t n_blocks = uint32_t((uint64_t(a.m) + CULL_BLOCK - 1u) / CULL_BLOCK);
  hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(256), 0, st, a, n_blocks);
  hipLaunchKernelGGL(k_cull_emit, dim3(n_blocks), dim3(CULL_BLOCK), 0, st, a);
}

// ---- the expansion of a list ------------------------------------------------------------------------------------------------------
// scene_query with one 32-bit division where q allows it
static __device__ __forceinline__ void listed_query(uint64_t q, uint32_t n_pairs, uint64_t& c, uint32_t& p) {
  if (q <= 0xFFFFFFFFull) {
    const uint32_t k = uint32_t(q) / n_pairs;
    c = k;
    p = uint32_t(q) - k * n_pairs;
  } else {
    scene_query(q, n_pairs, c, p);
  }
}

template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_scene_expand_listed64(SceneExpandArgs a, const uint64_t* __restrict__ ids) {
  const uint64_t total = uint64_t(a.m) * 6u;
  const double* __restrict__ table = static_cast<const double*>(a.object_tf);
  double2* __restrict__ o1 = static_cast<double2*>(a.tf1);
  double2* __restrict__ o2 = static_cast<double2*>(a.tf2);
  for (uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x; t < total; t += uint64_t(gridDim.x) * 256u) {
    const uint32_t row = uint32_t(t / 6u), part = uint32_t(t - uint64_t(row) * 6u);
    uint64_t c;
    uint32_t p;
    listed_query(ids[row], a.n_pairs, c, p);
    const uint2 ij = reinterpret_cast<const uint2*>(a.pairs)[p];
    const double* r1 = table + scene_pose_row(c, a.n_objects, ij.x, 12u) + 2u * part;
    const double* r2 = table + scene_pose_row(c, a.n_objects, ij.y, 12u) + 2u * part;
    double2 v1, v2;
    if (ALIGNED) {
      v1 = *reinterpret_cast<const double2*>(r1);
      v2 = *reinterpret_cast<const double2*>(r2);
    } else {
      v1.x = r1[0]; v1.y = r1[1];
      v2.x = r2[0]; v2.y = r2[1];
    }
    o1[t] = v1;
    o2[t] = v2;
    if (part == 0u) {
      a.s1[row] = a.object_shape[ij.x];
      a.s2[row] = a.object_shape[ij.y];
    }
  }
}

__global__ void __launch_bounds__(256) k_scene_expand_listed32(SceneExpandArgs a, const uint64_t* __restrict__ ids) {
  const uint64_t total = uint64_t(a.m) * 7u;
  const float* __restrict__ table = static_cast<const float*>(a.object_tf);
  float* __restrict__ o1 = static_cast<float*>(a.tf1);
  float* __restrict__ o2 = static_cast<float*>(a.tf2);
  for (uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x; t < total; t += uint64_t(gridDim.x) * 256u) {
    const uint32_t row = uint32_t(t / 7u), part = uint32_t(t - uint64_t(row) * 7u);
    uint64_t c;
    uint32_t p;
    listed_query(ids[row], a.n_pairs, c, p);
    const uint2 ij = reinterpret_cast<const uint2*>(a.pairs)[p];
    o1[t] = table[scene_pose_row(c, a.n_objects, ij.x, 7u) + part];
    o2[t] = table[scene_pose_row(c, a.n_objects, ij.y, 7u) + part];
    if (part == 0u) {
      a.s1[row] = a.object_shape[ij.x];
      a.s2[row] = a.object_shape[ij.y];
    }
  }
}

// the configuration of list entry k0 + row; c_wave: that of the wave's first row (the same in every lane)
static __device__ __forceinline__ uint64_t pairs_entry_conf(const uint64_t* __restrict__ conf_begin, uint64_t n_conf, uint64_t c_wave, uint64_t k) {
  return pairs_conf_from(conf_begin, n_conf, c_wave, k);
}
// ... of the first row any lane of this wave has in this trip: lane 0's row (the rows ascend with the lanes)
// (HFCL_PAIRS_LANE_SEARCH: a variant build in which every lane searches for itself -- the form this one was measured against,
// profiles/r14_a_scene_pairs.md)
static __device__ __forceinline__ uint64_t pairs_wave_conf(const uint64_t* __restrict__ conf_begin, uint64_t n_conf, uint64_t k_lane) {
#ifdef HFCL_PAIRS_LANE_SEARCH
  return pairs_conf_of(conf_begin, n_conf, k_lane);
#endif
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(k_lane)), hi = __builtin_amdgcn_readfirstlane(uint32_t(k_lane >> 32));
  return pairs_conf_of(conf_begin, n_conf, (uint64_t(hi) << 32) | lo);
}

template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_scene_expand_pairs64(SceneExpandArgs a, const uint32_t* __restrict__ pairs,
                                                              const uint64_t* __restrict__ conf_begin, uint64_t n_conf, uint64_t k0) {
  const uint64_t total = uint64_t(a.m) * 6u;
  const double* __restrict__ table = static_cast<const double*>(a.object_tf);
  double2* __restrict__ o1 = static_cast<double2*>(a.tf1);
  double2* __restrict__ o2 = static_cast<double2*>(a.tf2);
  for (uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x; t < total; t += uint64_t(gridDim.x) * 256u) {
    const uint32_t row = uint32_t(t / 6u), part = uint32_t(t - uint64_t(row) * 6u);
    const uint64_t k = k0 + row;
    const uint64_t c = pairs_entry_conf(conf_begin, n_conf, pairs_wave_conf(conf_begin, n_conf, k), k);
    const uint2 ij = reinterpret_cast<const uint2*>(pairs)[k];
    const double* r1 = table + scene_pose_row(c, a.n_objects, ij.x, 12u) + 2u * part;
    const double* r2 = table + scene_pose_row(c, a.n_objects, ij.y, 12u) + 2u * part;
    double2 v1, v2;
    if (ALIGNED) {
      v1 = *reinterpret_cast<const double2*>(r1);
      v2 = *reinterpret_cast<const double2*>(r2);
    } else {
      v1.x = r1[0]; v1.y = r1[1];
      v2.x = r2[0]; v2.y = r2[1];
    }
    o1[t] = v1;
    o2[t] = v2;
    if (part == 0u) {
      a.s1[row] = a.object_shape[ij.x];
      a.s2[row] = a.object_shape[ij.y];
    }
  }
}

__global__ void __launch_bounds__(256) k_scene_expand_pairs32(SceneExpandArgs a, const uint32_t* __restrict__ pairs,
                                                              const uint64_t* __restrict__ conf_begin, uint64_t n_conf, uint64_t k0) {
  const uint64_t total = uint64_t(a.m) * 7u;
  const float* __restrict__ table = static_cast<const float*>(a.object_tf);
  float* __restrict__ o1 = static_cast<float*>(a.tf1);
  float* __restrict__ o2 = static_cast<float*>(a.tf2);
  for (uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x; t < total; t += uint64_t(gridDim.x) * 256u) {
    const uint32_t row = uint32_t(t / 7u), part = uint32_t(t - uint64_t(row) * 7u);
    const uint64_t k = k0 + row;
    const uint64_t c = pairs_entry_conf(conf_begin, n_conf, pairs_wave_conf(conf_begin, n_conf, k), k);
    const uint2 ij = reinterpret_cast<const uint2*>(pairs)[k];
    o1[t] = table[scene_pose_row(c, a.n_objects, ij.x, 7u) + part];
    o2[t] = table[scene_pose_row(c, a.n_objects, ij.y, 7u) + part];
    if (part == 0u) {
      a.s1[row] = a.object_shape[ij.x];
      a.s2[row] = a.object_shape[ij.y];
    }
  }
}

void launch_scene_expand_pairs(hipStream_t st, const SceneExpandArgs& a, const uint32_t* pairs, const uint64_t* conf_begin, uint64_t n_conf,
                               uint64_t k0, bool f32, int max_blocks) {
  const uint64_t lanes = uint64_t(a.m) * (f32 ? 7u : 6u);
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((lanes + 255u) / 256u, uint64_t(max_blocks))));
  if (f32)
    hipLaunchKernelGGL(k_scene_expand_pairs32, dim3(grid), dim3(256), 0, st, a, pairs, conf_begin, n_conf, k0);
  else if ((reinterpret_cast<uintptr_t>(a.object_tf) & 15u) == 0)
    hipLaunchKernelGGL(k_scene_expand_pairs64<true>, dim3(grid), dim3(256), 0, st, a, pairs, conf_begin, n_conf, k0);
  else
    hipLaunchKernelGGL(k_scene_expand_pairs64<false>, dim3(grid), dim3(256), 0, st, a, pairs, conf_begin, n_conf, k0);
}

void launch_scene_expand_listed(hipStream_t st, const SceneExpandArgs& a, const uint64_t* ids, bool f32, int max_blocks) {
  const uint64_t lanes = uint64_t(a.m) * (f32 ? 7u : 6u);
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((lanes + 255u) / 256u, uint64_t(max_blocks))));
  if (f32)
    hipLaunchKernelGGL(k_scene_expand_listed32, dim3(grid), dim3(256), 0, st, a, ids);
  else if ((reinterpret_cast<uintptr_t>(a.object_tf) & 15u) == 0)
    hipLaunchKernelGGL(k_scene_expand_listed64<true>, dim3(grid), dim3(256), 0, st, a, ids);
  else
    hipLaunchKernelGGL(k_scene_expand_listed64<false>, dim3(grid), dim3(256), 0, st, a, ids);
}

// ---- the fold of a list -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_scene_summary_init(hfcl_scene_summary* summary, uint64_t n_conf) {
  hfcl_scene_summary s;
  scene_summary_init(s);
  for (uint64_t c = uint64_t(blockIdx.x) * 256u + threadIdx.x; c < n_conf; c += uint64_t(gridDim.x) * 256u) summary[c] = s;
}
void launch_scene_summary_init(hipStream_t st, hfcl_scene_summary* summary, uint64_t n_conf, int max_blocks) {
  if (!n_conf) return;
  const uint32_t grid = uint32_t(std::min<uint64_t>((n_conf + 255u) / 256u, uint64_t(max_blocks)));
  hipLaunchKernelGGL(k_scene_summary_init, dim3(grid), dim3(256), 0, st, summary, n_conf);
}

static __device__ __forceinline__ double listed_record_value(const hfcl_result& r, const SceneFoldListedArgs& a) {
  return scene_value(r.distance, a.margin, a.collide != 0);
}
static __device__ __forceinline__ double listed_record_value(const hfcl_result_f32& r, const SceneFoldListedArgs& a) {
  return scene_value(r.distance, float(a.margin), a.collide != 0);
}
// lane 0: a part of configuration c into its summary (plain read-modify-write: one wave per configuration and launch, launches in order)
static __device__ __forceinline__ void listed_store(const SceneFoldListedArgs& a, uint64_t c, const hfcl_scene_summary& part) {
  hfcl_scene_summary s = a.summary[c];
  scene_fold_merge(s, part);
  a.summary[c] = s;
}
// the configurations the chunk [k0, k1) of the list spans (hfcl_cull.hpp: scene_listed_span)
template <bool RANKED>
static __device__ __forceinline__ void listed_conf_range(const SceneFoldListedArgs& a, uint64_t& c_lo, uint64_t& n_conf) {
  if (RANKED) {  // (the spans of conf_begin that hold the chunk's first and last entry)
    c_lo = pairs_conf_of(a.conf_begin, a.n_conf, a.k0);
    n_conf = pairs_conf_of(a.conf_begin, a.n_conf, a.k1 - 1u) - c_lo + 1u;
  } else {
    scene_listed_span(a.ids[a.k0], a.ids[a.k1 - 1u], a.n_pairs, a.n_conf, c_lo, n_conf);
  }
}

template <typename R, bool RANKED>
__global__ void __launch_bounds__(256) k_scene_fold_listed(SceneFoldListedArgs a) {
  const R* __restrict__ rec = static_cast<const R*>(a.rec);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t shares = RANKED ? a.shares : scene_shares(a.n_pairs);
  uint64_t c_lo, n_conf;
  listed_conf_range<RANKED>(a, c_lo, n_conf);
  const uint64_t n_items = n_conf * shares;
  for (uint64_t w = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); w < n_items; w += uint64_t(gridDim.x) * 4u) {
    const uint64_t c = c_lo + w / shares;
    const uint32_t piece = uint32_t(w % shares);
    uint64_t lo, hi;
    scene_listed_piece(a.conf_begin[c], a.conf_begin[c + 1u], piece, a.k0, a.k1, lo, hi);
    hfcl_scene_summary s;
    scene_summary_init(s);
    for (uint64_t k = lo + lane; k < hi; k += 64u) {
      const R& r = rec[k - a.k0];
      scene_fold_record(s, listed_record_value(r, a), r.status, RANKED ? uint32_t(k - a.conf_begin[c]) : uint32_t(a.ids[k] - c * a.n_pairs));
    }
    scene_wave_reduce(s);
    if (lane == 0u) {
      if (a.partials)
        a.partials[w] = s;
      else if (hi > lo)
        listed_store(a, c, s);
    }
  }
}

template <bool RANKED>
__global__ void __launch_bounds__(256) k_scene_fold_listed_combine(SceneFoldListedArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t shares = RANKED ? a.shares : scene_shares(a.n_pairs);
  uint64_t c_lo, n_conf;
  listed_conf_range<RANKED>(a, c_lo, n_conf);
  for (uint64_t w = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); w < n_conf; w += uint64_t(gridDim.x) * 4u) {
    hfcl_scene_summary s;
    scene_summary_init(s);
    for (uint32_t g = lane; g < shares; g += 64u) scene_fold_merge(s, a.partials[w * shares + g]);
    scene_wave_reduce(s);
    if (lane == 0u) listed_store(a, c_lo + w, s);
  }
}

template <bool RANKED>
static void launch_fold_listed(hipStream_t st, const SceneFoldListedArgs& a, uint32_t shares, bool f32, int max_blocks) {
  const uint64_t items = a.n_conf * shares;  // (a bound: the span of the chunk is known on the device only; the waves stride it)
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((items + 3u) / 4u, uint64_t(max_blocks))));
  if (f32)
    hipLaunchKernelGGL((k_scene_fold_listed<hfcl_result_f32, RANKED>), dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((k_scene_fold_listed<hfcl_result, RANKED>), dim3(grid), dim3(256), 0, st, a);
  if (!a.partials) return;
  const uint32_t grid2 = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((a.n_conf + 3u) / 4u, uint64_t(max_blocks))));
  hipLaunchKernelGGL(k_scene_fold_listed_combine<RANKED>, dim3(grid2), dim3(256), 0, st, a);
}
void launch_scene_fold_listed(hipStream_t st, const SceneFoldListedArgs& a, bool f32, int max_blocks) {
  launch_fold_listed<false>(st, a, scene_shares(a.n_pairs), f32, max_blocks);
}
void launch_scene_fold_ranked(hipStream_t st, const SceneFoldListedArgs& a, uint32_t shares, bool f32, int max_blocks) {
  SceneFoldListedArgs r = a;
  r.shares = shares;
  launch_fold_listed<true>(st, r, shares, f32, max_blocks);
}
