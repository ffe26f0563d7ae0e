// hfcl_k_scene.hip -- scene queries (hfcl_scene_*): pure data movement around the solvers (HBM bound, no geometry).
//   k_scene_expand64<ALIGNED> / k_scene_expand32
//                         a chunk [q0, q0 + m) of the flat query range -> the per-pair arrays run_batch takes: shape ids from the
//                         object table, the two pose rows of every query gathered from the configuration's pose table.  One lane
//                         per 16-byte vector of a 96-byte row (6 lanes per row; 8-byte loads when the caller's table is not
//                         16-byte aligned), one lane per float of a 28-byte row; the stores are lane-contiguous.  Reads 8 B of pair
//                         list and writes 2 x 96 B + 8 B per query; the pose rows it reads come from a table that fits the caches
//                         (pairs of one configuration share rows and sit on neighbouring workgroups).
//   k_scene_fold<R>       records of a chunk -> hfcl_scene_summary: one wave per piece of a configuration's pair list
//                         (hfcl_scene.hpp: SCENE_FOLD_SHARE pairs), lanes stride the piece reading distance and status only, keep a
//                         partial summary each, the wave reduces them by a butterfly (smaller value, then smaller pair index: the
//                         order of the merges does not matter).  Pair lists of at most one piece: lane 0 combines with the
//                         configuration's stored summary (an earlier chunk of the same call, same stream: plain read-modify-write).
//                         Longer lists: the wave writes its partial and
//   k_scene_fold_combine  one wave per configuration of the chunk folds its pieces' partials and combines as above.
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_scene.hpp"

template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_scene_expand64(SceneExpandArgs a) {
  const uint64_t total = uint64_t(a.m) * 6u;
  const double* __restrict__ table = static_cast<const double*>(a.object_tf);
  double2* __restrict__ o1 = static_cast<double2*>(a.tf1);
  double2* __restrict__ o2 = static_cast<double2*>(a.tf2);
  for (uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x; t < total; t += uint64_t(gridDim.x) * 256u) {
    const uint32_t row = uint32_t(t / 6u), part = uint32_t(t - uint64_t(row) * 6u);
    uint64_t c;
    uint32_t p;
    scene_query_from(a.c0, a.p0, row, a.n_pairs, c, p);
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

__global__ void __launch_bounds__(256) k_scene_expand32(SceneExpandArgs a) {
  const uint64_t total = uint64_t(a.m) * 7u;
  const float* __restrict__ table = static_cast<const float*>(a.object_tf);
  float* __restrict__ o1 = static_cast<float*>(a.tf1);
  float* __restrict__ o2 = static_cast<float*>(a.tf2);
  for (uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x; t < total; t += uint64_t(gridDim.x) * 256u) {
    const uint32_t row = uint32_t(t / 7u), part = uint32_t(t - uint64_t(row) * 7u);
    uint64_t c;
    uint32_t p;
    scene_query_from(a.c0, a.p0, row, a.n_pairs, c, p);
    const uint2 ij = reinterpret_cast<const uint2*>(a.pairs)[p];
    o1[t] = table[scene_pose_row(c, a.n_objects, ij.x, 7u) + part];
    o2[t] = table[scene_pose_row(c, a.n_objects, ij.y, 7u) + part];
    if (part == 0u) {
      a.s1[row] = a.object_shape[ij.x];
      a.s2[row] = a.object_shape[ij.y];
    }
  }
}

void launch_scene_expand(hipStream_t st, const SceneExpandArgs& a, bool f32, int max_blocks) {
  const uint64_t lanes = uint64_t(a.m) * (f32 ? 7u : 6u);
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((lanes + 255u) / 256u, uint64_t(max_blocks))));
  if (f32)
    hipLaunchKernelGGL(k_scene_expand32, dim3(grid), dim3(256), 0, st, a);
  else if ((reinterpret_cast<uintptr_t>(a.object_tf) & 15u) == 0)
    hipLaunchKernelGGL(k_scene_expand64<true>, dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_scene_expand64<false>, dim3(grid), dim3(256), 0, st, a);
}

// lane 0: the chunk's part of configuration c into its summary
static __device__ __forceinline__ void scene_store(const SceneFoldArgs& a, uint64_t c, const hfcl_scene_summary& part) {
  hfcl_scene_summary s = part;
  if (!scene_chunk_starts(c, a.n_pairs, a.q0)) {
    s = a.summary[c];
    scene_fold_merge(s, part);
  }
  a.summary[c] = s;
}

static __device__ __forceinline__ double scene_record_value(const hfcl_result& r, const SceneFoldArgs& a) {
  return scene_value(r.distance, a.margin, a.collide != 0);
}
static __device__ __forceinline__ double scene_record_value(const hfcl_result_f32& r, const SceneFoldArgs& a) {
  return scene_value(r.distance, float(a.margin), a.collide != 0);
}

template <typename R>
__global__ void __launch_bounds__(256) k_scene_fold(SceneFoldArgs a) {
  const R* __restrict__ rec = static_cast<const R*>(a.rec);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t w = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); w < a.n_pieces; w += uint64_t(gridDim.x) * 4u) {
    uint64_t c, lo, hi;
    scene_piece_range(a.g0 + w, a.n_pairs, a.q0, a.q1, c, lo, hi);
    hfcl_scene_summary s;
    scene_summary_init(s);
    for (uint64_t q = lo + lane; q < hi; q += 64u) {
      const R& r = rec[q - a.q0];
      scene_fold_record(s, scene_record_value(r, a), r.status, uint32_t(q - c * a.n_pairs));
    }
    scene_wave_reduce(s);
    if (lane == 0u) {
      if (a.partials)
        a.partials[w] = s;
      else
        scene_store(a, c, s);  // (one piece per configuration: piece id = configuration)
    }
  }
}

__global__ void __launch_bounds__(256) k_scene_fold_combine(SceneFoldArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t shares = scene_shares(a.n_pairs);
  const uint64_t c0 = a.g0 / shares, g_last = a.g0 + a.n_pieces - 1u;
  const uint64_t n_conf = g_last / shares - c0 + 1u;
  for (uint64_t w = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); w < n_conf; w += uint64_t(gridDim.x) * 4u) {
    const uint64_t c = c0 + w;
    const uint64_t lo = c * shares > a.g0 ? c * shares : a.g0, hi = c * shares + shares - 1u < g_last ? c * shares + shares - 1u : g_last;
    hfcl_scene_summary s;
    scene_summary_init(s);
    for (uint64_t g = lo + lane; g <= hi; g += 64u) scene_fold_merge(s, a.partials[g - a.g0]);
    scene_wave_reduce(s);
    if (lane == 0u) scene_store(a, c, s);
  }
}

void launch_scene_fold(hipStream_t st, const SceneFoldArgs& a, bool f32, int max_blocks) {
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((a.n_pieces + 3u) / 4u, uint64_t(max_blocks))));
  if (f32)
    hipLaunchKernelGGL(k_scene_fold<hfcl_result_f32>, dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_scene_fold<hfcl_result>, dim3(grid), dim3(256), 0, st, a);
  if (!a.partials) return;
  const uint32_t shares = scene_shares(a.n_pairs);
  const uint64_t n_conf = (a.g0 + a.n_pieces - 1u) / shares - a.g0 / shares + 1u;
  const uint32_t grid2 = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((n_conf + 3u) / 4u, uint64_t(max_blocks))));
  hipLaunchKernelGGL(k_scene_fold_combine, dim3(grid2), dim3(256), 0, st, a);
}
