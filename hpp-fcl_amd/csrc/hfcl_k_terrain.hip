// hfcl_k_terrain.hip -- a height-field terrain under a scene's moving objects (hfcl_scene_collide_terrain*; hfcl_terrain.hpp has the
// arithmetic): pure data movement around the height-field kernels of hfcl_k_hfield.hip, which run as they are.
//   k_terrain_expand<ALIGNED>  a chunk [q0, q0 + m) of the flat query range -> the per-query arrays hf_run takes: the field id, the shape
//                              id of the listed object, the terrain's pose row, the object's pose row gathered from the table.  One lane
//                              per 16-byte vector of a 96-byte row (6 lanes per row; 8-byte loads when the caller's table is not 16-byte
//                              aligned), lane-contiguous stores, as k_scene_expand64.
//   k_terrain_status           the status words of a chunk's records into the call's kept array (4 of 96 bytes a record)
//   k_terrain_fold             after the last chunk: one wave per configuration over its n_t kept (bound, status) entries, lanes stride
//                              them, a butterfly on the key (bound, object index) -- no atomics, no workgroup waits for another, and the
//                              chunks of the call do not show in the result.
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_terrain.hpp"

template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_terrain_expand(TerrainExpandArgs a) {
  const uint64_t total = uint64_t(a.m) * 6u;
  const double* __restrict__ table = a.table;
  const double2* __restrict__ terrain = reinterpret_cast<const double2*>(a.tf_terrain);
  double2* __restrict__ oh = reinterpret_cast<double2*>(a.out_tfh);
  double2* __restrict__ os = reinterpret_cast<double2*>(a.out_tfs);
  for (uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x; t < total; t += uint64_t(gridDim.x) * 256u) {
    uint32_t row, part, object;
    uint64_t src;
    terrain_expand_lane(a, t, row, part, object, src);
    double2 v;
    if (ALIGNED) {
      v = *reinterpret_cast<const double2*>(table + src);
    } else {
      v.x = table[src];
      v.y = table[src + 1u];
    }
    oh[t] = terrain[part];
    os[t] = v;
    if (part == 0u) {
      a.out_hfield[row] = a.hfield;
      a.out_shape[row] = a.object_shape[object];
    }
  }
}

void launch_terrain_expand(hipStream_t st, const TerrainExpandArgs& a, int max_blocks) {
  if (!a.m) return;
  const uint64_t lanes = uint64_t(a.m) * 6u;
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((lanes + 255u) / 256u, uint64_t(max_blocks))));
  if ((reinterpret_cast<uintptr_t>(a.table) & 15u) == 0)
    hipLaunchKernelGGL(k_terrain_expand<true>, dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_terrain_expand<false>, dim3(grid), dim3(256), 0, st, a);
}

__global__ void __launch_bounds__(256) k_terrain_status(const hfcl_result* __restrict__ rec, uint32_t* __restrict__ status, uint32_t m) {
  for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < m; i += uint64_t(gridDim.x) * 256u) status[i] = rec[i].status;
}

void launch_terrain_status(hipStream_t st, const hfcl_result* rec, uint32_t* status, uint32_t m, int max_blocks) {
  if (!m) return;
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((uint64_t(m) + 255u) / 256u, uint64_t(max_blocks))));
  hipLaunchKernelGGL(k_terrain_status, dim3(grid), dim3(256), 0, st, rec, status, m);
}

__global__ void __launch_bounds__(256) k_terrain_fold(TerrainFoldArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t c = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); c < a.n_conf; c += uint64_t(gridDim.x) * 4u) {
    hfcl_scene_summary s;
    terrain_fold_lane(s, a.bounds, a.status, a.objects, c, a.n_t, lane, 64u);
    scene_wave_reduce(s);
    if (lane == 0u) a.summary[c] = s;
  }
}

void launch_terrain_fold(hipStream_t st, const TerrainFoldArgs& a, int max_blocks) {
  if (!a.n_conf) return;
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((a.n_conf + 3u) / 4u, uint64_t(max_blocks))));
  hipLaunchKernelGGL(k_terrain_fold, dim3(grid), dim3(256), 0, st, a);
}
