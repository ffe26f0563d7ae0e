// hfcl_k_nearest.hip -- the per-configuration minimum distance of a scene with box-bound pruning (hfcl_scene_nearest*): the kernels around
// the two narrow-phase passes, which themselves run through the listed scene path (hfcl_k_cull.hip).  Bandwidth and latency kernels as those
// of the cull: no geometry loop, no scratch, no atomics.  Built without contraction (FLAGS_k_nearest): the bounds are the bits of the
// host build of hfcl_nearest.hpp.
//   k_nearest_seed          a wave per (configuration, piece of SCENE_FOLD_SHARE pairs): a lane computes L of its pairs from the box table,
//                           butterfly over the 64 lanes, lane 0 writes seed[c] (pair lists of one piece) or a partial for
//   k_nearest_seed_combine  a wave per configuration folds its pieces' partials
//   k_nearest_mark<PASS>    k_cull_mark's geometry, ballots and counts with the predicate of pass 1 / pass 2; L is recomputed from the
//                           boxes (no per-query array of bounds); k_cull_scan and k_cull_emit follow unchanged
//   k_nearest_threshold     a lane per configuration: thr[c] = min(D, min_distance of pass 1)
//   k_nearest_gather<R>     a lane per configuration: binary search of c * n_pairs + min_pair in the configuration's two list segments,
//                           one record copied
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_nearest.hpp"

static __device__ __forceinline__ double nearest_query_bound(const CullArgs& a, uint64_t c, uint32_t p, double r) {
  const uint2 ij = reinterpret_cast<const uint2*>(a.pairs)[p];
  const double* base = a.boxes + 6u * ((c - a.c_box0) * a.n_objects);
  const double* b1 = base + 6u * size_t(ij.x);
  const double* b2 = base + 6u * size_t(ij.y);
  double x[6], y[6];
  for (int k = 0; k < 6; ++k) {
    x[k] = b1[k];
    y[k] = b2[k];
  }
  return nearest_bound(x, y, r);
}

static __device__ __forceinline__ void nearest_seed_wave_reduce(NearestSeed& s) {
  for (int off = 32; off > 0; off >>= 1) {
    const double L = __shfl_xor(s.L, off, 64);
    const uint32_t p = __shfl_xor(s.p, off, 64);
    nearest_seed_merge(s, L, p);
  }
}

__global__ void __launch_bounds__(256) k_nearest_seed(NearestArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n_pairs = a.c.n_pairs, shares = scene_shares(n_pairs);
  const uint64_t n_items = a.c.n_conf * shares;
  NearestSeed* partials = static_cast<NearestSeed*>(a.seed_partials);
  for (uint64_t w = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); w < n_items; w += uint64_t(gridDim.x) * 4u) {
    const uint64_t c = w / shares;
    const uint32_t piece = uint32_t(w - c * shares);
    const uint32_t lo = piece * SCENE_FOLD_SHARE;
    const uint32_t hi = n_pairs - lo > SCENE_FOLD_SHARE ? lo + SCENE_FOLD_SHARE : n_pairs;
    NearestSeed s;
    nearest_seed_init(s);
    for (uint32_t p = lo + lane; p < hi; p += 64u) nearest_seed_merge(s, nearest_query_bound(a.c, c, p, a.r), p);
    nearest_seed_wave_reduce(s);
    if (lane == 0u) {
      if (partials) partials[w] = s;
      else a.seed[c] = s.p;
    }
  }
}

__global__ void __launch_bounds__(256) k_nearest_seed_combine(NearestArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t shares = scene_shares(a.c.n_pairs);
  const NearestSeed* partials = static_cast<const NearestSeed*>(a.seed_partials);
  for (uint64_t c = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); c < a.c.n_conf; c += uint64_t(gridDim.x) * 4u) {
    NearestSeed s;
    nearest_seed_init(s);
    for (uint32_t g = lane; g < shares; g += 64u) {
      const NearestSeed o = partials[c * shares + g];
      nearest_seed_merge(s, o.L, o.p);
    }
    nearest_seed_wave_reduce(s);
    if (lane == 0u) a.seed[c] = s.p;
  }
}

void launch_nearest_seed(hipStream_t st, const NearestArgs& a, int max_blocks) {
  const uint32_t shares = scene_shares(a.c.n_pairs);
  const uint64_t items = a.c.n_conf * shares;
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((items + 3u) / 4u, uint64_t(max_blocks))));
  hipLaunchKernelGGL(k_nearest_seed, dim3(grid), dim3(256), 0, st, a);
  if (!a.seed_partials) return;
  const uint32_t grid2 = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((a.c.n_conf + 3u) / 4u, uint64_t(max_blocks))));
  hipLaunchKernelGGL(k_nearest_seed_combine, dim3(grid2), dim3(256), 0, st, a);
}

template <int PASS>
__global__ void __launch_bounds__(CULL_BLOCK) k_nearest_mark(NearestArgs n) {
  __shared__ uint32_t wave_count[CULL_WAVES];
  const CullArgs& a = n.c;
  const uint32_t row = blockIdx.x * CULL_BLOCK + threadIdx.x, wave = threadIdx.x >> 6;
  bool keep = false;
  if (row < a.m) {
    uint64_t c;
    uint32_t p;
    scene_query_from(a.c0, a.p0, row, a.n_pairs, c, p);
    const double L = nearest_query_bound(a, c, p, n.r);
    const uint32_t seed = n.seed[c];
    keep = PASS == 1 ? nearest_in_pass1(L, p, seed, n.upper) : nearest_in_pass2(L, p, seed, n.upper, n.thr[c]);
  }
  const uint64_t ballot = __ballot(keep);
  if ((threadIdx.x & 63u) == 0u) {
    if (row < a.m) a.words[row >> 6] = ballot;
    wave_count[wave] = cull_popcount(ballot);
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t k = 0;
    for (uint32_t w = 0; w < CULL_WAVES; ++w) k += wave_count[w];
    a.block_counts[blockIdx.x] = k;
  }
}

void launch_nearest_chunk(hipStream_t st, const NearestArgs& a, int pass) {
  const uint32_t n_blocks = uint32_t((uint64_t(a.c.m) + CULL_BLOCK - 1u) / CULL_BLOCK);
  if (pass == 1)
    hipLaunchKernelGGL(k_nearest_mark<1>, dim3(n_blocks), dim3(CULL_BLOCK), 0, st, a);
  else
    hipLaunchKernelGGL(k_nearest_mark<2>, dim3(n_blocks), dim3(CULL_BLOCK), 0, st, a);
  launch_cull_scan_emit(st, a.c);
}

__global__ void __launch_bounds__(256) k_nearest_threshold(NearestArgs a, const hfcl_scene_summary* __restrict__ summary) {
  const uint64_t c = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (c < a.c.n_conf) a.thr[c] = nearest_threshold(a.upper, summary[c].min_distance);
}
void launch_nearest_threshold(hipStream_t st, const NearestArgs& a, const hfcl_scene_summary* summary) {
  if (!a.c.n_conf) return;
  hipLaunchKernelGGL(k_nearest_threshold, dim3(uint32_t((a.c.n_conf + 255u) / 256u)), dim3(256), 0, st, a, summary);
}

template <typename R>
__global__ void __launch_bounds__(256) k_nearest_gather(NearestGatherArgs a) {
  const uint64_t c = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (c >= a.n_conf) return;
  R out;
  nearest_no_record(out);
  const uint32_t mp = a.summary[c].min_pair;
  if (mp != SCENE_NONE) {
    const uint64_t q = c * a.n_pairs + mp;
    for (int l = 0; l < 2; ++l) {
      const uint64_t lo = a.conf_begin[l][c], hi = a.conf_begin[l][c + 1u];
      const uint64_t k = nearest_find(a.ids[l], lo, hi, q);
      if (k < hi) {
        out = static_cast<const R*>(a.rec[l])[k];
        break;
      }
    }
  }
  static_cast<R*>(a.out)[c] = out;
}
void launch_nearest_gather(hipStream_t st, const NearestGatherArgs& a, bool f32) {
  if (!a.n_conf) return;
  const uint32_t grid = uint32_t((a.n_conf + 255u) / 256u);
  if (f32)
    hipLaunchKernelGGL(k_nearest_gather<hfcl_result_f32>, dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_nearest_gather<hfcl_result>, dim3(grid), dim3(256), 0, st, a);
}
