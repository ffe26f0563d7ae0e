// hfcl_k_env.hip -- a static environment kept on the device (include/hppfcl_amd_env.h): the boxes of the environment's tiles, the pairs
// of the moving objects among themselves and against the environment per configuration (hfcl_scene_env_pairs*), and the expansion of such
// a list for the narrow phase.  hfcl_env.hpp has the arithmetic and the geometry of column tiles, spans and cells.  Built without
// contraction (FLAGS_k_env): the grown boxes are the bits of cull_keep, as in hfcl_k_pairs.hip.
//   k_env_tile_boxes      set time: a thread per (tile, coordinate) folds the tile's up to PAIRS_TILE member boxes in member order
//   k_env_sweep<EMIT> / k_env_sweep_groups<EMIT>   the tiled sweep of hfcl_k_pairs.hip with its parallelism from the columns as well: a
//                         workgroup owns a cell -- a block of PAIRS_ROWS consecutive moving rows of one configuration times a span of
//                         consecutive column tiles, the moving columns j > i of that configuration first, the environment's tiles behind
//                         them.  A tile comes in as 16-byte loads, is grown and stored component-major in LDS; a ballot per row.  A tile is
//                         skipped -- in front of the barriers, by a value the whole workgroup shares -- when none of its groups may pair with
//                         any row of the block (pairs_block_mask) or, an environment tile, when its grown box does not touch the union of
//                         the block's grown boxes (env_tile_skipped): it holds no listed pair.  Count: a uint32 per (row, span), row-major;
//                         the scan is launch_pairs_scan with rows x spans as its rows; emit takes the same decisions.
//   k_scene_expand_env64<ALIGNED> / 32   k_scene_expand_pairs64 / 32 (hfcl_k_cull.hip) with two tables: rows of i and of j < n_moving from
//                         the moving table, rows of j >= n_moving from the environment's
// No atomics, no scratch, no kernel waits for another workgroup; the list is the same bytes however the call is cut into chunks and spans.
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_env.hpp"

__global__ void __launch_bounds__(256) k_env_tile_boxes(const double* __restrict__ env_boxes, uint32_t n_env, double* __restrict__ tile_boxes) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x >= 6u * env_tiles(n_env)) return;
  tile_boxes[x] = env_tile_coord(env_boxes, n_env, x / 6u, x % 6u);
}
void launch_env_tile_boxes(hipStream_t st, const double* env_boxes, uint32_t n_env, double* tile_boxes) {
  const uint32_t n = 6u * env_tiles(n_env);
  if (!n) return;
  hipLaunchKernelGGL(k_env_tile_boxes, dim3((n + 255u) / 256u), dim3(256), 0, st, env_boxes, n_env, tile_boxes);
}

// a decision every lane took from the same values, as a scalar: what it guards lies in front of a workgroup barrier
static __device__ __forceinline__ bool env_uniform(bool x) { return __builtin_amdgcn_readfirstlane(int(x)) != 0; }

template <bool EMIT, bool GROUPS>
static __device__ __forceinline__ void env_sweep_body(const EnvArgs& a) {
  __shared__ double tile[6][PAIRS_TILE];
  __shared__ uint8_t tile_group[GROUPS ? PAIRS_TILE : 1u];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t nm = a.n_moving, n = nm + a.n_env;
  const uint32_t blk = blockIdx.x / a.n_spans, span = blockIdx.x - blk * a.n_spans;
  PairsGeometry geo;
  geo.n_objects = nm;
  geo.rows_per_block = PAIRS_ROWS;
  geo.blocks_per_conf = a.blocks_per_conf;
  EnvGeometry eg;
  eg.n_moving = nm;
  eg.n_env = a.n_env;
  eg.tiles_moving = a.tiles_moving;
  eg.tiles = a.tiles;
  eg.span_len = a.span_len;
  eg.n_spans = a.n_spans;
  uint64_t c;
  uint32_t i0, i1;
  pairs_block(geo, a.p.g0 + blk, c, i0, i1);
  const double* __restrict__ boxes = a.p.boxes + 6u * ((c - a.p.c_box0) * nm);  // the configuration's moving boxes
  const uint64_t chunk_row = c * nm + i0 - a.row0;                              // the block's first row in the chunk
  const double inflate = a.p.inflate;

  // what the whole workgroup shares: the groups any row of the block may pair with, the union of the block's grown boxes
  uint64_t block_mask = ~uint64_t(0);
  if (GROUPS) block_mask = pairs_block_mask(a.p.group, a.p.collides, i0, i1);
  double uni[6];
  env_union(boxes, i0, i1, inflate, uni);

  double row_box[PAIRS_WAVE_ROWS][6];
  uint32_t row_i[PAIRS_WAVE_ROWS], count[PAIRS_WAVE_ROWS];
  uint64_t pos[PAIRS_WAVE_ROWS];
  uint64_t row_mask[GROUPS ? PAIRS_WAVE_ROWS : 1u];
  for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
    const uint32_t i = i0 + wave * PAIRS_WAVE_ROWS + r;
    const bool there = i < i1;
    row_i[r] = there ? i : n;  // (no row: its tests fail on j > i)
    count[r] = 0u;
    if (GROUPS) {
      const uint64_t m = there ? a.p.collides[a.p.group[i] & 63u] : 0u;
      const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(m)))), hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(m >> 32))));
      row_mask[r] = (uint64_t(hi) << 32) | lo;
    }
    double raw[6];
    for (int k = 0; k < 6; ++k) raw[k] = boxes[6u * size_t(there ? i : i0) + k];
    pairs_grow(raw, inflate, row_box[r]);
    pos[r] = EMIT && there ? a.p.row_offsets[(chunk_row + wave * PAIRS_WAVE_ROWS + r) * a.n_spans + span] : 0u;
  }

  uint32_t u0 = span * a.span_len;
  const uint32_t u1 = a.tiles - u0 > a.span_len ? u0 + a.span_len : a.tiles;
  const uint32_t first = env_first_tile(i0, a.tiles_moving);
  if (u0 < first) u0 = first;
  if (GROUPS && block_mask == 0u) u0 = u1;  // (a block that may pair with nothing: zero counts)
  for (uint32_t u = u0; u < u1; ++u) {
    bool env;
    uint32_t base, j0, j_end;
    env_tile_columns(eg, u, env, base, j0, j_end);
    if (GROUPS && pairs_tile_skipped(a.col_tile_groups[u], block_mask)) continue;  // (workgroup-uniform: no loads, no barrier)
    if (env && env_uniform(env_tile_skipped(a.env_tile_boxes + 6u * size_t(base / PAIRS_TILE), inflate, uni))) continue;  // (the same)
    const uint32_t cols = j_end - j0 < PAIRS_TILE ? j_end - j0 : PAIRS_TILE;  // columns of the tile
    const double2* __restrict__ vec = reinterpret_cast<const double2*>(env ? a.env_boxes : boxes) + 3u * size_t(base);  // (48 B a box, 16-byte aligned tables)
    __syncthreads();  // (the tile before has been read)
    for (uint32_t v = threadIdx.x; v < 3u * PAIRS_TILE; v += 256u) {
      const uint32_t col = v / 3u, part = v - 3u * col;
      if (col < cols) {
        const double2 x = vec[v];
        tile[2u * part][col] = part < 2u ? x.x - inflate : x.x + inflate;
        tile[2u * part + 1u][col] = part < 1u ? x.y - inflate : x.y + inflate;
      }
    }
    if (GROUPS)
      for (uint32_t col = threadIdx.x; col < cols; col += 256u) tile_group[col] = a.p.group[j0 + col];
    __syncthreads();
    for (uint32_t step = 0; step < PAIRS_TILE; step += 64u) {
      const uint32_t j = j0 + step + lane;
      double col_box[6];
      for (int k = 0; k < 6; ++k) col_box[k] = tile[k][step + lane];  // (columns past the tile's: stale values, refused by j < j_end)
      const uint32_t col_group = GROUPS ? tile_group[step + lane] : 0u;
      for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
        const bool keep = pairs_keep(row_i[r], j, j_end, row_box[r], col_box) && (!GROUPS || pairs_allowed(row_mask[r], col_group));
        const uint64_t ballot = __ballot(keep);
        if (EMIT && ballot != 0u) {
          const uint64_t p = pos[r] + count[r] + cull_rank(ballot, lane);
          if (keep && p < a.p.capacity) reinterpret_cast<uint2*>(a.p.pairs)[p] = make_uint2(row_i[r], j);
        }
        count[r] += cull_popcount(ballot);
      }
    }
  }
  if (!EMIT && lane == 0u)
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r)
      if (row_i[r] < n) a.p.row_counts[(chunk_row + wave * PAIRS_WAVE_ROWS + r) * a.n_spans + span] = count[r];
}
template <bool EMIT>
__global__ void __launch_bounds__(256) k_env_sweep(EnvArgs a) {
  env_sweep_body<EMIT, false>(a);
}
template <bool EMIT>
__global__ void __launch_bounds__(256) k_env_sweep_groups(EnvArgs a) {
  env_sweep_body<EMIT, true>(a);
}

void launch_env_chunk(hipStream_t st, const EnvArgs& a) {
  const bool groups = a.p.group != nullptr;
  const dim3 grid(a.p.n_blocks * a.n_spans);
  void (*const count)(EnvArgs) = groups ? k_env_sweep_groups<false> : k_env_sweep<false>;
  void (*const emit)(EnvArgs) = groups ? k_env_sweep_groups<true> : k_env_sweep<true>;
  hipLaunchKernelGGL(count, grid, dim3(256), 0, st, a);
  launch_pairs_scan(st, a.p);
  if (!a.p.pairs || !a.p.capacity) return;  // count only
  hipLaunchKernelGGL(emit, grid, dim3(256), 0, st, a);
}

// ---- the expansion of an env list ---------------------------------------------------------------------------------------------------
// the configuration of list entry k; the wave's first row's is found once (hfcl_k_cull.hip: pairs_wave_conf)
static __device__ __forceinline__ uint64_t env_entry_conf(const uint64_t* __restrict__ conf_begin, uint64_t n_conf, uint64_t k) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(k)), hi = __builtin_amdgcn_readfirstlane(uint32_t(k >> 32));
  return pairs_conf_from(conf_begin, n_conf, pairs_conf_of(conf_begin, n_conf, (uint64_t(hi) << 32) | lo), k);
}

template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_scene_expand_env64(SceneExpandArgs a, const uint32_t* __restrict__ pairs,
                                                            const uint64_t* __restrict__ conf_begin, uint64_t n_conf, uint64_t k0,
                                                            const double* __restrict__ env) {
  const uint64_t total = uint64_t(a.m) * 6u;
  const double* __restrict__ table = static_cast<const double*>(a.object_tf);
  const uint32_t nm = uint32_t(a.n_objects);
  double2* __restrict__ o1 = static_cast<double2*>(a.tf1);
  double2* __restrict__ o2 = static_cast<double2*>(a.tf2);
  for (uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x; t < total; t += uint64_t(gridDim.x) * 256u) {
    const uint32_t row = uint32_t(t / 6u), part = uint32_t(t - uint64_t(row) * 6u);
    const uint64_t k = k0 + row;
    const uint64_t c = env_entry_conf(conf_begin, n_conf, k);
    const uint2 ij = reinterpret_cast<const uint2*>(pairs)[k];
    const double* r1 = table + scene_pose_row(c, nm, ij.x, 12u) + 2u * part;
    const bool from_env = ij.y >= nm;
    const double* r2 = (from_env ? env + 12u * size_t(ij.y - nm) : table + scene_pose_row(c, nm, ij.y, 12u)) + 2u * part;
    double2 v1, v2;
    if (ALIGNED) {
      v1 = *reinterpret_cast<const double2*>(r1);
      v2 = *reinterpret_cast<const double2*>(r2);
    } else {  // (the caller's table is not 16-byte aligned; the environment's is)
      v1.x = r1[0]; v1.y = r1[1];
      if (from_env) {
        v2 = *reinterpret_cast<const double2*>(r2);
      } else {
        v2.x = r2[0]; v2.y = r2[1];
      }
    }
    o1[t] = v1;
    o2[t] = v2;
    if (part == 0u) {
      a.s1[row] = a.object_shape[ij.x];
      a.s2[row] = a.object_shape[ij.y];
    }
  }
}

__global__ void __launch_bounds__(256) k_scene_expand_env32(SceneExpandArgs a, const uint32_t* __restrict__ pairs,
                                                            const uint64_t* __restrict__ conf_begin, uint64_t n_conf, uint64_t k0,
                                                            const float* __restrict__ env) {
  const uint64_t total = uint64_t(a.m) * 7u;
  const float* __restrict__ table = static_cast<const float*>(a.object_tf);
  const uint32_t nm = uint32_t(a.n_objects);
  float* __restrict__ o1 = static_cast<float*>(a.tf1);
  float* __restrict__ o2 = static_cast<float*>(a.tf2);
  for (uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x; t < total; t += uint64_t(gridDim.x) * 256u) {
    const uint32_t row = uint32_t(t / 7u), part = uint32_t(t - uint64_t(row) * 7u);
    const uint64_t k = k0 + row;
    const uint64_t c = env_entry_conf(conf_begin, n_conf, k);
    const uint2 ij = reinterpret_cast<const uint2*>(pairs)[k];
    o1[t] = table[scene_pose_row(c, nm, ij.x, 7u) + part];
    o2[t] = ij.y >= nm ? env[7u * size_t(ij.y - nm) + part] : table[scene_pose_row(c, nm, ij.y, 7u) + part];
    if (part == 0u) {
      a.s1[row] = a.object_shape[ij.x];
      a.s2[row] = a.object_shape[ij.y];
    }
  }
}

void launch_scene_expand_env(hipStream_t st, const SceneExpandArgs& a, const uint32_t* pairs, const uint64_t* conf_begin, uint64_t n_conf,
                             uint64_t k0, const void* env_tf, bool f32, int max_blocks) {
  const uint64_t lanes = uint64_t(a.m) * (f32 ? 7u : 6u);
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((lanes + 255u) / 256u, uint64_t(max_blocks))));
  if (f32)
    hipLaunchKernelGGL(k_scene_expand_env32, dim3(grid), dim3(256), 0, st, a, pairs, conf_begin, n_conf, k0, static_cast<const float*>(env_tf));
  else if ((reinterpret_cast<uintptr_t>(a.object_tf) & 15u) == 0)
    hipLaunchKernelGGL(k_scene_expand_env64<true>, dim3(grid), dim3(256), 0, st, a, pairs, conf_begin, n_conf, k0, static_cast<const double*>(env_tf));
  else
    hipLaunchKernelGGL(k_scene_expand_env64<false>, dim3(grid), dim3(256), 0, st, a, pairs, conf_begin, n_conf, k0, static_cast<const double*>(env_tf));
}
